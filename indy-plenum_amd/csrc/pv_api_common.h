// What the translation units of the C-ABI layer share (pv_api.cpp and
// pv_api_{merkle,state,trie}.cpp): error reporting, device buffers, the
// per-device state, the scope of an entry point, the helpers of the host
// forms and the handle table of the resident objects.  Internal: everything
// here is hidden from the library's dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/plenum_verify.h"
#include "pv_kernels.h"

namespace pvapi __attribute__((visibility("hidden"))) {

// records the message for pv_last_error() and returns `code` (pv_api.cpp)
int fail(int code, const char* fmt, ...);
const std::string& last_error();   // the calling thread's message

// host-buffer pipeline (pv_verify_batch): a shard runs as leading ramp
// chunks and then at most PV_HOST_CHUNKS chunks of at least PV_HOST_CHUNK_MIN
// signatures
#define PV_HOST_CHUNKS 8
#define PV_HOST_CHUNK_MIN 32768
// ramp: leading chunks of 32768, 65536, ... signatures (below a regular
// chunk), so the first grid starts after a ~12 MB DMA (C2 end to end with
// fused chunks 11.6 vs 12.1 ms, profiles/r02_ab_fused_chunking.jsonl)
#define PV_HOST_RAMP 32768
// generic batches of at most this many signatures run the latency-mode curve
// kernel (k_verify_quad: one launch, lane quads per point); tuning.lat_max (0 disables)
#define PV_LAT_MAX 32768
// keyed batches (prepared keys) of at most this many signatures run the keyed
// latency kernel (k_verify_quad_keyed); tuning.lat_keyed_max (0 disables)
#define PV_LAT_KEYED_MAX 8192
// BLS calls of at most this many checks run the lane-quad check kernel
// (pv_bls.hip; the same default as its PV_BLS_QUAD_MAX); tuning.bls_quad_max
#define PV_BLS_QUAD_MAX_DEFAULT 32768
// ... and calls of at most this many the lane-octet kernel; tuning.bls_oct_max
#define PV_BLS_OCT_MAX_DEFAULT 4096
// host-buffer calls of at most this many signatures skip the H2D / D2H copies:
// the latency kernel reads the gathered inputs from, and writes the verdicts
// to, fine-grained page-locked host memory (one launch per call instead of
// copy + launch + copy); tuning.small_zc_max (0 = always copy)
#define PV_SMALL_ZC_MAX 2048
// shards of at least this many signatures decide PV_FLAG_DEDUP_KEYS from a sample
#define PV_DEDUP_SAMPLE_MIN 262144
// chunk gathers into the pinned staging ring use up to this many host threads
// (tuning.host_copy_threads); gathers under PV_HOST_PAR_MIN bytes stay on
// the calling thread
#define PV_HOST_COPY_THREADS 8
#define PV_HOST_PAR_MIN (4u << 20)
// largest page-locked staging slot (two per device, plus the shard's verdicts):
// at most ~1 GiB of locked host memory per device while pinned staging is on
#define PV_HOST_PIN_MAX (size_t(512) << 20)

#define HIP_OK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return fail(e_ == hipErrorOutOfMemory ? PV_ENOMEM : PV_EIO, "%s failed: %s (%s:%d)", #expr, \
                  hipGetErrorString(e_), __FILE__, __LINE__);                                 \
  } while (0)

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  hipError_t ensure(size_t n) {
    if (n <= cap && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n < 64 ? 64 : n;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// page-locked host buffer (one slot of the host-buffer staging ring)
struct PinBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;  // bytes
  unsigned flags = hipHostMallocDefault;
  uint8_t* dev = nullptr;  // device address of a mapped buffer (looked up once per allocation)
  hipError_t ensure(size_t n) {
    if (n <= cap && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    dev = nullptr;
    cap = 0;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), n, flags);
    if (e == hipSuccess && (flags & hipHostMallocMapped)) {
      void* a = nullptr;
      e = hipHostGetDevicePointer(&a, p, 0);
      if (e != hipSuccess) {
        (void)hipHostFree(p);
        p = nullptr;
        return e;
      }
      dev = static_cast<uint8_t*>(a);
    }
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    dev = nullptr;
    cap = 0;
  }
};

// host -> host copies of one chunk's inputs, split over `threads` threads by
// byte range of the concatenated jobs.  A job with `rebase` set copies u64
// values minus `rebase` (the chunk's message offsets made shard-relative while
// they are gathered: no separate pass over all offsets before the first DMA);
// it must be the FIRST job, so that the 8-byte-multiple piece boundaries never
// split one of its values between two threads.
struct CopyJob {
  uint8_t* dst;
  const uint8_t* src;
  size_t n;            // bytes (a multiple of 8 for rebased jobs)
  uint64_t rebase = 0;
  bool u64 = false;
};

// rebased u64 jobs also check that the values never decrease (message
// offsets): *bad is set, the caller refuses the chunk before any kernel reads it
inline void copy_part(const CopyJob& j, size_t lo, size_t hi, std::atomic<bool>* bad) {
  if (!j.u64) {
    memcpy(j.dst + lo, j.src + lo, hi - lo);
    return;
  }
  const uint64_t* a = reinterpret_cast<const uint64_t*>(j.src + lo);
  uint64_t* b = reinterpret_cast<uint64_t*>(j.dst + lo);
  uint64_t prev = lo ? a[-1] : a[0];
  bool dec = false;
  for (size_t k = 0; k < (hi - lo) / 8; ++k) {
    dec |= a[k] < prev;
    prev = a[k];
    b[k] = a[k] - j.rebase;
  }
  if (dec && bad) bad->store(true, std::memory_order_relaxed);
}

inline void gather_range(const CopyJob* jobs, int nj, size_t a, size_t b, std::atomic<bool>* bad) {
  size_t base = 0;
  for (int j = 0; j < nj && base < b; base += jobs[j].n, ++j) {
    const size_t lo = std::max(a, base) - base, hi = std::min(b, base + jobs[j].n) - base;
    if (lo < hi) copy_part(jobs[j], lo, hi, bad);
  }
}

// Persistent gather threads of one device (the host pipeline gathers every
// chunk: starting threads per chunk cost ~20 us each).  run() splits the
// concatenated jobs into `threads` pieces of 8-byte multiples; piece 0 runs on
// the caller.  Threads are started lazily; one that cannot be started leaves
// its pieces to the caller (no exception crosses the ABI).  Used by one
// thread at a time (a device's shard worker).
struct GatherPool {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv, cv_done;
  const CopyJob* jobs = nullptr;
  int nj = 0, pieces = 0;
  size_t total = 0, piece = 0;
  std::atomic<bool>* bad = nullptr;
  uint64_t gen = 0;
  int pending = 0;
  bool stop = false;

  void worker(int t) {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return stop || gen != seen; });
      if (stop) return;
      seen = gen;
      const bool mine = t < pieces;
      const size_t a = std::min(total, piece * t), b = std::min(total, piece * (t + 1));
      const CopyJob* J = jobs;
      const int n = nj;
      std::atomic<bool>* flag = bad;
      lk.unlock();
      if (mine) gather_range(J, n, a, b, flag);
      lk.lock();
      if (--pending == 0) cv_done.notify_one();
    }
  }

  void run(const CopyJob* js, int n, int threads, std::atomic<bool>* flag) {
    size_t tot = 0;
    for (int j = 0; j < n; ++j) tot += js[j].n;
    if (threads <= 1 || tot < PV_HOST_PAR_MIN) {
      gather_range(js, n, 0, tot, flag);
      return;
    }
    while ((int)th.size() < threads - 1) {
      try {
        th.emplace_back(&GatherPool::worker, this, (int)th.size() + 1);
      } catch (...) {
        break;
      }
    }
    const int p = (int)th.size() + 1;
    const size_t pc = ((tot + p - 1) / p + 7) & ~size_t(7);
    {
      std::lock_guard<std::mutex> lk(mu);
      jobs = js;
      nj = n;
      total = tot;
      piece = pc;
      pieces = p;
      bad = flag;
      pending = (int)th.size();
      ++gen;
    }
    cv.notify_all();
    gather_range(js, n, 0, std::min(tot, pc), flag);
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return pending == 0; });
  }

  void shutdown() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv.notify_all();
    for (auto& t : th) t.join();
    th.clear();
    stop = false;
  }
  ~GatherPool() { shutdown(); }  // idle threads never outlive the pool (process exit included)
};

// PV_CURVE_MODE (read at pv_init): "half" (default) = half-size scalars with
// full-length tasks for deferred records; "full" = every record deferred
// (full-length verdicts through the same kernel: A/B timing and tests);
// "grouped" = the previous generic kernel (k_curve, 8 signatures per lane
// sharing one inversion).  Verdicts are identical in every mode.
enum class CurveMode { Half, Full, Grouped };

// Verify workspaces and the compute stream they are used on.  Device-pointer
// calls use ws[0] (stream = the device stream or the caller's; pv_*_async:
// ws[slot]); the host-buffer pipeline alternates chunks over ws[0] and ws[1]
// on their two streams, so the kernels of chunk c + 1 fill the tail of chunk
// c's persistent grid
// instead of waiting for it (the scratch of concurrently running curve grids
// must not alias: one per workspace).
struct Workspace {
  hipStream_t stream = nullptr;
  DevBuf<uint32_t> scratch;            // per-lane A / -R tables for the persistent curve grid
  DevBuf<uint32_t> h;                  // SHA-512 digest, 16 words per signature
  DevBuf<unsigned long long> counter;  // hash-kernel work queue
  DevBuf<uint8_t> pre;
  DevBuf<uint64_t> bitmap;
  DevBuf<uint32_t> hrec, dlist;        // lattice records, deferred indices (half-size path)
  DevBuf<unsigned long long> qc;       // [0] deferred count, [1] curve task queue
  bool half_ran = false;               // qc[0] holds the last generic batch's deferred count
  // last use: recorded after every enqueue on this workspace (whatever stream
  // it ran on); the next use on another stream waits for it, so an async batch
  // still running on a caller's stream never shares scratch / h / hrec / qc /
  // counter / bitmap with a later sync, host-buffer or async call
  hipEvent_t done = nullptr;
  hipStream_t done_on = nullptr;
  void release() {
    scratch.release(); h.release(); counter.release(); pre.release(); bitmap.release();
    hrec.release(); dlist.release(); qc.release();
    if (done) (void)hipEventDestroy(done);
    done = nullptr;
    done_on = nullptr;
  }
};

// order a use of workspace w on stream s after its previous use
inline int ws_begin(Workspace& w, hipStream_t s) {
  if (w.done_on && w.done_on != s) HIP_OK(hipStreamWaitEvent(s, w.done, 0));
  return PV_OK;
}

inline int ws_end(Workspace& w, hipStream_t s) {
  HIP_OK(hipEventRecord(w.done, s));
  w.done_on = s;
  return PV_OK;
}

// One use of workspace w on stream s: ordered after the previous use on
// construction (`rc`), recorded as the last use by end().  An early (error)
// return records it from the destructor, so later users of the workspace still
// wait for whatever was queued; after fork(), stream s first waits for the
// side stream (its tail recorded in `join`), whose work uses the workspace too.
struct WsUse {
  Workspace& w;
  hipStream_t s;
  const int rc;
  bool open;
  hipStream_t side = nullptr;
  hipEvent_t join = nullptr;
  WsUse(Workspace& w_, hipStream_t s_) : w(w_), s(s_), rc(ws_begin(w_, s_)), open(rc == PV_OK) {}
  WsUse(const WsUse&) = delete;
  WsUse& operator=(const WsUse&) = delete;
  void fork(hipStream_t side_, hipEvent_t join_) {
    side = side_;
    join = join_;
  }
  int end() {
    open = false;
    return ws_end(w, s);
  }
  ~WsUse() {   // no fail() here: the first error stays in pv_last_error()
    if (!open) return;
    if (join && hipEventRecord(join, side) == hipSuccess) (void)hipStreamWaitEvent(s, join, 0);
    if (hipEventRecord(w.done, s) == hipSuccess) w.done_on = s;
  }
};

struct Device {
  int id = -1;   // engine device id: the device_mask bit and the `device` argument
  int ord = -1;  // HIP ordinal (== id, except under pv_test_init_dup)
  hipStream_t stream = nullptr;
  hipStream_t copy = nullptr;   // host-buffer calls: H2D of chunk c+1 overlaps the kernels of chunk c
  hipEvent_t copied = nullptr;  // recorded on `copy` after each chunk's inputs, waited on by `stream`
  // tuning.host_staging: PV_STAGING_PINNED (default) gathers chunk c of a
  // host-buffer call into page-locked slot c & 1 and DMAs it from there;
  // PV_STAGING_PAGEABLE hands the caller's buffers to hipMemcpyAsync (runtime staging)
  bool pinned = true;
  int copy_threads = PV_HOST_COPY_THREADS;
  int host_chunks = PV_HOST_CHUNKS;  // tuning.host_chunks (1..256)
  int first_pct = 50;                // first chunk, % of a regular one; tuning.host_first_pct (10..100)
  // leading chunks r, 2r, 4r, ... below a regular chunk instead of one first
  // chunk (tuning.host_ramp; 0 = off, first_pct then sizes the first chunk)
  uint64_t ramp = PV_HOST_RAMP;
  size_t pin_max = PV_HOST_PIN_MAX;  // largest page-locked slot; tuning.host_pin_max_mb (16..4096)
  uint64_t lat_max = PV_LAT_MAX;     // generic batches up to this size use the latency kernel; tuning.lat_max (0 = off)
  uint64_t lat_keyed_max = PV_LAT_KEYED_MAX;  // keyed batches up to this size: k_verify_quad_keyed
  uint64_t zc_max = PV_SMALL_ZC_MAX;          // host calls up to this size: zero-copy (tuning.small_zc_max)
  PinBuf zc_in, zc_out;                       // fine-grained page-locked image / verdicts of zero-copy calls
  PinBuf zc_flag;                             // completion word of zero-copy calls, polled by the host
  uint32_t zc_seq = 0;
  DevBuf<uint32_t> zc_done;                   // block counter of a keyed kernel that writes the word itself
  bool zc_done_armed = false;                 // zc_done zeroed (the kernel's last block re-arms it)
  bool lat_quad = true;              // latency kernel: k_verify_quad (lane quads); PV_LAT_PAIR: k_curve_lat
  // host-buffer chunks of generic batches: one k_chunk_half launch per chunk
  // + one k_verify_quad_list pass for the deferred records; tuning.host_fused 0:
  // k_hash + k_lattice + k_curve_half per chunk (the device-resident schedule)
  bool chunk_fused = true;
  DevBuf<uint32_t> dl;               // shard indices deferred by k_chunk_half
  DevBuf<unsigned long long> dlc;    // their count
  hipEvent_t joined = nullptr;       // ws[1] drained into ws[0] (deferred pass)
  PinBuf pin[2];
  std::shared_ptr<GatherPool> pool = std::make_shared<GatherPool>();  // host gather threads
  PinBuf vout;  // page-locked verdicts of the shard (D2H target; copied to the caller after the drain)
  hipEvent_t staged[2] = {nullptr, nullptr};  // slot i's H2D has finished
  hipEvent_t keys_ready = nullptr;            // prepared-key table built (host pipeline, ws[0] -> ws[1])
  // pv_verify_keys_device_async: slot i's key preparation runs on kside[i],
  // forked from the caller's stream after the workspace's previous use (kfork)
  // and joined back before the curve kernel (kjoin), so it overlaps the hash stage
  hipStream_t kside[2] = {nullptr, nullptr};
  hipEvent_t kfork[2] = {nullptr, nullptr}, kjoin[2] = {nullptr, nullptr};
  int cu_count = 0;
  int curve_blocks = 0;
  int hash_blocks = 0;
  DevBuf<uint32_t> btab;
  DevBuf<uint32_t> bw;        // radix-2^16 base-point chunk tables (half-size path, keyed comb)
  Workspace ws[2];
  int last_ws = 0;            // workspace of the last generic verify (pv_curve_stats)
  size_t scratch_words = 0;   // per-workspace curve scratch
  DevBuf<unsigned long long> counter;  // SHA-256 work queue
  // staging for host-memory calls
  DevBuf<uint8_t> pk, sig, blob, verdict, tamper;
  DevBuf<uint8_t> stage;      // small host-buffer calls: device image of pinned slot 0 (run_small)
  DevBuf<uint64_t> off, batch_off;
  DevBuf<uint32_t> sender, votes;
  DevBuf<uint32_t> tflag, tbits;  // tally: out-of-range sender flag; staged voter bitmaps
  DevBuf<uint8_t> reached;
  DevBuf<uint64_t> scan;      // block sums of the device prefix scan
  DevBuf<uint64_t> vsrc;      // pv_state_store_get_device: where each value lies in the store's blob
  DevBuf<uint32_t> ktab, kidx;  // prepared keys + per-signature key index (deduplicated host batches)
  DevBuf<uint32_t> kscr, kscr2;  // key-preparation scratch (kscr2: async slot 1)
  DevBuf<uint32_t> mk0, mk1;    // Merkle level ping-pong / leaf digests
  DevBuf<uint32_t> kc;          // persistent key cache: slot j = comb tables of g_kc key j
  uint64_t kc_count = 0;        // slots prepared on this device
  DevBuf<uint8_t> kcpk;         // staging of keys being added
  int sha256_blocks = 0;
  int sha3_blocks = 0;
  int curve_blocks_keyed = 0;
  int curve_half_blocks = 0;
  CurveMode mode = CurveMode::Half;
  // pv_kernel_timing: HIP-event times of every verify launch while enabled
  bool live_timing = false;
  float live_hash = 0, live_curve = 0;
  float live_sha = 0;   // the SHA-512 part of the hash interval (pre-checks + k_hash, no k_lattice)
  uint64_t live_launches = 0;
  // live timing records four events per launch without waiting (pipelined
  // callers keep launches in flight); they are resolved when the pool fills
  // up and when timing stops
  struct LiveRec {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};   // start, prep end, curve end, k_hash end
  };
  std::vector<LiveRec> live_pool;
  size_t live_used = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
};

// restores the caller's current HIP device on scope exit (torch shares it)
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() { (void)hipGetDevice(&prev); }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

extern std::mutex g_mu;             // the library lock (pv_api.cpp)
extern std::vector<Device> g_devs;
void release_trees();   // resident Merkle trees (pv_merkle_tree_*), pv_api_merkle.cpp
void release_stores();  // resident trie node stores (pv_state_store_*), pv_api_state.cpp

inline Device* find_dev(int id) {
  for (auto& d : g_devs)
    if (d.id == id) return &d;
  return nullptr;
}

// Scope of one entry point: holds the library lock, restores the caller's
// current HIP device on exit and resolves the engine device -- `device` (and
// the workspace slot) of a device-pointer form, device 0 of a host-buffer form.
// check() is the refusal every form starts with; begin() makes the device
// current and picks the stream; finish() is the tail of a synchronous form.
struct Entry {
  std::lock_guard<std::mutex> lk{g_mu};
  DeviceGuard dg;
  const bool host;
  const int id, slot;
  Device* d;
  hipStream_t s = nullptr;
  explicit Entry(int device, int slot_ = 0) : host(false), id(device), slot(slot_), d(find_dev(device)) {}
  Entry() : host(true), id(0), slot(0), d(g_devs.empty() ? nullptr : &g_devs[0]) {}
  int check() const {
    if (!d)
      return host ? fail(PV_ENOTINIT, "pv_init has not been called")
                  : fail(PV_ENOTINIT, "device %d not initialised (call pv_init)", id);
    if (slot < 0 || slot > 1) return fail(PV_EINVAL, "slot must be 0 or 1");
    return PV_OK;
  }
  // the caller's stream, else the slot's (slot 0: the device stream)
  int begin(void* stream = nullptr) {
    HIP_OK(hipSetDevice(d->ord));
    s = stream ? reinterpret_cast<hipStream_t>(stream) : d->ws[slot].stream;
    return PV_OK;
  }
  int finish(int rc = PV_OK) {
    if (rc) return rc;
    HIP_OK(hipStreamSynchronize(s));
    return PV_OK;
  }
};

// ------------------------------------------------ shared by the entry points
inline const uint32_t* w32(const uint8_t* p) { return reinterpret_cast<const uint32_t*>(p); }
inline uint32_t* w32(uint8_t* p) { return reinterpret_cast<uint32_t*>(p); }
inline bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

// call-scoped device buffer of the host-buffer entry points
template <typename T>
struct TmpBuf {
  T* p = nullptr;
  TmpBuf() = default;
  TmpBuf(const TmpBuf&) = delete;
  TmpBuf& operator=(const TmpBuf&) = delete;
  ~TmpBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), (n ? n : 1) * sizeof(T)); }
  // allocate and start the upload of n elements on s
  hipError_t put(const T* host, size_t n, hipStream_t s) {
    hipError_t e = alloc(n);
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpyAsync(p, host, n * sizeof(T), hipMemcpyHostToDevice, s);
  }
};

// Declared after the TmpBufs of a host form: once work may be queued on s,
// every return drains s before the buffers are freed (hipFree would wait too;
// this says so), and the first error stays the one reported.
struct StreamDrain {
  hipStream_t s;
  bool done = false;
  int finish() {
    done = true;
    HIP_OK(hipStreamSynchronize(s));
    return PV_OK;
  }
  ~StreamDrain() {
    if (!done) (void)hipStreamSynchronize(s);
  }
};

inline int offsets_ok(const uint64_t* off, uint64_t n, const char* what) {
  for (uint64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return fail(PV_EINVAL, "%s not monotone at %llu", what, (unsigned long long)i);
  return PV_OK;
}

// bytes of src, then the 16 zero bytes the hash kernels read past the last message
inline int upload_padded(uint8_t* dst, const uint8_t* src, uint64_t bytes, hipStream_t s) {
  if (bytes) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemsetAsync(dst + bytes, 0, 16, s));
  return PV_OK;
}

// The slice [off[0], off[n]) of a ragged host array (off = NULL with n = 0:
// empty).  The device gets the slice alone, so its offsets are rebased to
// zero; rebased() is read by the copy in flight and lives as long as this.
struct Ragged {
  const uint64_t* off;
  const uint64_t n, b0, len;
  std::vector<uint64_t> offs;
  Ragged(const uint64_t* off_, uint64_t n_) : off(off_), n(n_), b0(n_ ? off_[0] : 0), len(n_ ? off_[n_] - b0 : 0) {}
  int check(const char* what) const { return offsets_ok(off, n, what); }
  const uint64_t* rebased() {
    offs.resize(n + 1);
    for (uint64_t k = 0; k <= n; ++k) offs[k] = n ? off[k] - b0 : 0;
    return offs.data();
  }
  // a byte blob and its offsets, into the device's persistent staging buffers ...
  int stage(const uint8_t* blob, Device& d, hipStream_t s) {
    HIP_OK(d.blob.ensure(len + 16));
    HIP_OK(d.off.ensure(n + 1));
    return upload(blob, d.blob.p, d.off.p, s);
  }
  // ... or into call-scoped ones
  int stage(const uint8_t* blob, TmpBuf<uint8_t>& dblob, TmpBuf<uint64_t>& doff, hipStream_t s) {
    HIP_OK(dblob.alloc(len + 16));
    HIP_OK(doff.alloc(n + 1));
    return upload(blob, dblob.p, doff.p, s);
  }
  int upload(const uint8_t* blob, uint8_t* dblob, uint64_t* doff, hipStream_t s) {
    if (const int rc = upload_padded(dblob, len ? blob + b0 : nullptr, len, s)) return rc;
    HIP_OK(hipMemcpyAsync(doff, rebased(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    return PV_OK;
  }
};

inline int merkle_blocks(const Device& d) { return d.cu_count * 32; }

// HIP events at the phase boundaries of a timed call (pv_time_state_store_prune, pv_time_state_sort_device)
struct PhaseEvents {
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool on = false;
  hipError_t create() {
    on = true;
    for (auto& e : ev)
      if (const hipError_t rc = hipEventCreate(&e)) return rc;
    return hipSuccess;
  }
  hipError_t mark(int i, hipStream_t s) { return on ? hipEventRecord(ev[i], s) : hipSuccess; }
  ~PhaseEvents() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// *p holds at least `need` elements afterwards (+ `pad` elements never counted
// in the capacity): the capacity, `first_cap` for an empty buffer, doubles until
// it does; the `used` elements in use move device-to-device on s, which is
// synchronised before the old buffer is freed
template <typename T>
int grow_device(T** p, uint64_t* cap, uint64_t need, uint64_t used, uint64_t pad, uint64_t first_cap, hipStream_t s) {
  if (*p && need <= *cap) return PV_OK;
  uint64_t nc = *cap ? *cap : first_cap;
  while (nc < need) nc *= 2;
  T* np = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&np), (nc + pad) * sizeof(T)));
  if (*p) {
    hipError_t e = hipSuccess;
    if (used) e = hipMemcpyAsync(np, *p, used * sizeof(T), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      (void)hipFree(np);
      HIP_OK(e);
    }
    (void)hipFree(*p);
  }
  *p = np;
  *cap = nc;
  return PV_OK;
}

// The handles of one kind of resident object (Merkle trees, trie node stores):
// id = index + 1, and a freed slot is the next one given out.  T has `live` and
// `dev` (Device::id); `drop` frees the device memory of a live object; `noun`
// and `key` word the refusals.  Used under the library lock.
template <typename T>
struct HandleTable {
  void (*const drop)(T&);
  const char *const noun, *const key;
  std::vector<T> v;
  // a fresh live object of device `dev` in the lowest free slot, or in a new one
  int alloc(int dev, int32_t* id, T** t) {
    size_t i = 0;
    while (i < v.size() && v[i].live) ++i;
    if (i == v.size()) {
      if (v.size() >= 0x7fffffffull) return fail(PV_ENOMEM, "too many %ss", noun);
      v.emplace_back();
    }
    v[i] = T();
    v[i].live = true;
    v[i].dev = dev;
    *id = (int32_t)(i + 1);
    *t = &v[i];
    return PV_OK;
  }
  T* find(int32_t id) {
    if (id < 1 || (size_t)id > v.size() || !v[id - 1].live) return nullptr;
    return &v[id - 1];
  }
  // resolve an id to its object and point the (host-form) entry scope at the
  // object's device; en.begin() then makes it current
  int enter(Entry& en, int32_t id, T** t) {
    if (const int rc = en.check()) return rc;
    *t = find(id);
    if (!*t) return fail(PV_EINVAL, "no %s with %s %d", noun, key, (int)id);
    en.d = find_dev((*t)->dev);
    if (!en.d) return fail(PV_EINVAL, "the device of %s %d is gone", noun, (int)id);
    return PV_OK;
  }
  // once the object's device is idle: its memory freed, its slot free
  void release(T& t) {
    if (!t.live) return;
    if (Device* d = find_dev(t.dev)) {
      (void)hipSetDevice(d->ord);
      (void)hipStreamSynchronize(d->stream);
    }
    drop(t);
    t = T();
  }
  // the pv_*_free entry point (takes the library lock itself)
  int free(int32_t id) {
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceGuard dg;
    T* t = find(id);
    if (!t) return fail(PV_EINVAL, "no %s with %s %d", noun, key, (int)id);
    release(*t);
    return PV_OK;
  }
  void release_all() {   // pv_shutdown
    for (auto& t : v) release(t);
    v.clear();
  }
};

// A resident node store (pv_trie_store.h): the nodes' bytes, ranges, digests
// and duplicate flags, the digest-keyed table and the device count of nodes
// that hold a table slot.  Every buffer doubles on overflow with a
// device-to-device copy on the call's stream, as the resident Merkle tree does.
struct StateStore {
  bool live = false;
  int dev = -1;              // Device::id
  uint64_t n_nodes = 0, n_unique = 0, n_bytes = 0;
  uint32_t slots = 0;
  uint8_t* blob = nullptr;   // cap_bytes + 16 bytes
  uint64_t cap_bytes = 0;
  uint64_t *beg = nullptr, *end = nullptr;   // cap_nodes each
  uint32_t* dig = nullptr;                   // cap_nodes x 8 words
  uint8_t* dup = nullptr;                    // cap_nodes
  uint64_t cap_nodes = 0;
  uint32_t* table = nullptr;                 // slots
  unsigned int* unique = nullptr;            // device copy of n_unique (k_trie_store_insert adds to it)
};

extern HandleTable<StateStore> g_stores;   // store id = index + 1 (pv_api_state.cpp, as the two functions below)
inline StateStore* find_store(int32_t id) { return g_stores.find(id); }
inline int store_enter(Entry& en, int32_t id, StateStore** st) { return g_stores.enter(en, id, st); }
int store_reserve(StateStore& st, uint64_t nodes, uint64_t bytes, hipStream_t s);
int store_rehash(StateStore& st, uint32_t slots, const Device& d, hipStream_t s);

}  // namespace pvapi
