// C-ABI layer of libplenum_verify.so (include/plenum_verify.h).
//
// Owns per-device state (stream, base-point table, workspaces), shards host
// batches over the devices in a mask (contiguous index ranges, SURVEY.md
// §8(e)), and launches the kernels in pv_kernels.hip.  No exceptions cross
// the ABI: every entry point returns 0 or a negative code and records a
// message for pv_last_error().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <random>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/plenum_verify.h"
#include "pv_kernels.h"
#include "pv_trie_proof.h"
#include "pv_trie_store.h"
#include "pv_trie_prune.h"
#include "pv_trie_build.h"
#include "pv_trie_update.h"
#include "pv_trie_sort.h"

static_assert(pv::SP_OK == PV_SP_OK && pv::SP_VALUE_MISMATCH == PV_SP_VALUE_MISMATCH &&
                  pv::SP_NODE_MISSING == PV_SP_NODE_MISSING && pv::SP_MALFORMED == PV_SP_MALFORMED,
              "public state-proof status codes");
static_assert(PV_KEY_WORDS == (unsigned)pv::KEYTAB_WORDS, "prepared-key layout");
static_assert(PV_KEY_WORDS_WIDE == (unsigned)pv::KEYTAB_WIDE_WORDS, "wide prepared-key layout");

namespace pvbls {
void set_quad_max(uint64_t n);   // pv_bls.hip
void set_oct_max(uint64_t n);
}

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

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
void copy_part(const CopyJob& j, size_t lo, size_t hi, std::atomic<bool>* bad) {
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

void gather_range(const CopyJob* jobs, int nj, size_t a, size_t b, std::atomic<bool>* bad) {
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

// Distinct 32-byte keys of a host batch (PV_FLAG_DEDUP_KEYS): open addressing
// with linear probing over 32-bit slots (0 = empty, else 1 + distinct index),
// hashed from the key's first 16 bytes; no per-key allocation.
struct KeyIndex {
  std::vector<uint32_t> slot;
  uint64_t mask = 0;
  const uint8_t* base = nullptr;  // key j at base + 32 * first[j]
  std::vector<uint64_t> first;    // position of each distinct key's first use
  void reset(const uint8_t* keys, uint64_t n) {
    uint64_t cap = 64;
    while (cap < 2 * n) cap <<= 1;
    slot.assign(cap, 0);
    mask = cap - 1;
    base = keys;
    first.clear();
  }
  // distinct index of key i (inserted on first sight)
  uint32_t insert(uint64_t i) {
    const uint8_t* k = base + 32 * i;
    uint64_t a, b;
    memcpy(&a, k, 8);
    memcpy(&b, k + 8, 8);
    uint64_t h = (a ^ (b * 0x9E3779B97F4A7C15ull)) * 0xBF58476D1CE4E5B9ull;
    for (uint64_t p = (h >> 17) & mask;; p = (p + 1) & mask) {
      const uint32_t v = slot[p];
      if (!v) {
        first.push_back(i);
        slot[p] = (uint32_t)first.size();
        return v + (uint32_t)first.size() - 1;
      }
      if (!memcmp(base + 32 * first[v - 1], k, 32)) return v - 1;
    }
  }
};

// Persistent verifying-key cache (pv_keycache_add): host-side index of the
// cached 32-byte keys; key j's comb tables sit in slot j of every device's
// `kc` table.  Open addressing over all 32 bytes with a per-process random
// seed (keys come from the ledger, so their first bytes are attacker-chosen).
struct KeyCache {
  std::vector<uint8_t> keys;      // 32 bytes per cached key, slot order
  std::vector<uint32_t> slot;     // 0 = empty, else 1 + slot
  uint64_t mask = 0;
  uint64_t seed = 0;
  uint64_t count() const { return keys.size() / 32; }
  uint64_t hash(const uint8_t* k) const {
    uint64_t h = seed;
    for (int i = 0; i < 4; ++i) {
      uint64_t w;
      memcpy(&w, k + 8 * i, 8);
      h = (h ^ w) * 0x9E3779B97F4A7C15ull;
      h ^= h >> 29;
    }
    return h;
  }
  // slot of key k, or UINT32_MAX
  uint32_t find(const uint8_t* k) const {
    if (slot.empty()) return UINT32_MAX;
    for (uint64_t p = hash(k) & mask;; p = (p + 1) & mask) {
      const uint32_t v = slot[p];
      if (!v) return UINT32_MAX;
      if (!memcmp(keys.data() + 32 * (uint64_t)(v - 1), k, 32)) return v - 1;
    }
  }
  void rehash(uint64_t cap) {
    slot.assign(cap, 0);
    mask = cap - 1;
    for (uint64_t j = 0; j < count(); ++j)
      for (uint64_t p = hash(keys.data() + 32 * j) & mask;; p = (p + 1) & mask)
        if (!slot[p]) {
          slot[p] = (uint32_t)(j + 1);
          break;
        }
  }
  // append keys (already known to be absent and distinct) as new slots
  void commit(const std::vector<uint8_t>& add) {
    if (!seed) seed = ((uint64_t)std::random_device{}() << 32 | std::random_device{}()) | 1;
    keys.insert(keys.end(), add.begin(), add.end());
    uint64_t cap = slot.size() ? slot.size() : 64;
    while (cap < 2 * count()) cap <<= 1;
    rehash(cap);
  }
  void clear() {
    keys.clear();
    slot.clear();
    mask = 0;
  }
};
KeyCache g_kc;

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
int ws_begin(Workspace& w, hipStream_t s) {
  if (w.done_on && w.done_on != s) HIP_OK(hipStreamWaitEvent(s, w.done, 0));
  return PV_OK;
}

int ws_end(Workspace& w, hipStream_t s) {
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

std::mutex g_mu;
std::vector<Device> g_devs;
void release_trees();   // resident Merkle trees (pv_merkle_tree_*), below
void release_stores();  // resident trie node stores (pv_state_store_*), below

Device* find_dev(int id) {
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

// the process's schedule tuning (include/plenum_verify.h, pv_set_tuning):
// defaults only, never the environment
pv_tuning default_tuning() {
  pv_tuning t{};
  t.struct_size = sizeof(pv_tuning);
  t.curve_mode = PV_CURVE_HALF;
  t.lat_max = PV_LAT_MAX;
  t.lat_keyed_max = PV_LAT_KEYED_MAX;
  t.small_zc_max = PV_SMALL_ZC_MAX;
  t.lat_kernel = PV_LAT_QUAD;
  t.host_fused = 1;
  t.host_staging = PV_STAGING_PINNED;
  t.host_chunks = PV_HOST_CHUNKS;
  t.host_first_pct = 50;
  t.host_copy_threads = PV_HOST_COPY_THREADS;
  t.host_ramp = PV_HOST_RAMP;
  t.host_pin_max_mb = (uint32_t)(PV_HOST_PIN_MAX >> 20);
  t.bls_quad_max = PV_BLS_QUAD_MAX_DEFAULT;
  t.bls_oct_max = PV_BLS_OCT_MAX_DEFAULT;
  return t;
}
pv_tuning g_tune = default_tuning();
int g_dup = 0;   // pv_test_init_dup: engine devices sharing HIP device 0 (test only)

int check_tuning(const pv_tuning& t) {
  if (t.struct_size != sizeof(pv_tuning))
    return fail(PV_EINVAL, "struct_size %u != sizeof(pv_tuning) %zu", t.struct_size, sizeof(pv_tuning));
  if (t.curve_mode > PV_CURVE_GROUPED) return fail(PV_EINVAL, "unknown curve mode %u", t.curve_mode);
  if (t.lat_max > (1ull << 20) || t.lat_keyed_max > (1ull << 20) || t.small_zc_max > (1ull << 20))
    return fail(PV_EINVAL, "lat_max / lat_keyed_max / small_zc_max must be <= 2^20");
  if (t.lat_kernel > PV_LAT_PAIR) return fail(PV_EINVAL, "unknown latency kernel %u", t.lat_kernel);
  if (t.host_fused > 1) return fail(PV_EINVAL, "host_fused must be 0 or 1");
  if (t.host_staging > PV_STAGING_PAGEABLE) return fail(PV_EINVAL, "unknown staging mode %u", t.host_staging);
  if (t.host_chunks < 1 || t.host_chunks > 256) return fail(PV_EINVAL, "host_chunks must be in 1..256");
  if (t.host_first_pct < 10 || t.host_first_pct > 100) return fail(PV_EINVAL, "host_first_pct must be in 10..100");
  if (t.host_copy_threads < 1 || t.host_copy_threads > 64) return fail(PV_EINVAL, "host_copy_threads must be in 1..64");
  if (t.host_ramp != 0 && (t.host_ramp < 1024 || t.host_ramp > (1ull << 20)))
    return fail(PV_EINVAL, "host_ramp must be 0 or in 1024..2^20");
  if (t.host_pin_max_mb < 16 || t.host_pin_max_mb > 4096) return fail(PV_EINVAL, "host_pin_max_mb must be in 16..4096");
  if (t.host_trace > 1) return fail(PV_EINVAL, "host_trace must be 0 or 1");
  if (t.bls_quad_max > (1u << 20) || t.bls_oct_max > (1u << 20))
    return fail(PV_EINVAL, "bls_quad_max / bls_oct_max must be <= 2^20");
  if (t.reserved != 0) return fail(PV_EINVAL, "reserved must be 0");
  return PV_OK;
}

void apply_tuning(Device& d, const pv_tuning& t) {
  const CurveMode m = t.curve_mode == PV_CURVE_HALF ? CurveMode::Half
                      : t.curve_mode == PV_CURVE_FULL ? CurveMode::Full : CurveMode::Grouped;
  if (m != d.mode)
    for (auto& w : d.ws) w.half_ran = false;
  d.mode = m;
  d.lat_max = t.lat_max;
  d.lat_keyed_max = t.lat_keyed_max;
  d.zc_max = t.small_zc_max;
  d.lat_quad = t.lat_kernel == PV_LAT_QUAD;
  d.chunk_fused = t.host_fused != 0;
  d.host_chunks = (int)t.host_chunks;
  d.first_pct = (int)t.host_first_pct;
  d.copy_threads = (int)t.host_copy_threads;
  d.ramp = t.host_ramp;
  d.pin_max = size_t(t.host_pin_max_mb) << 20;
  const bool pinned = t.host_staging == PV_STAGING_PINNED;
  if (d.pinned && !pinned && d.copy) {   // pageable staging holds no page-locked memory
    (void)hipSetDevice(d.ord);
    (void)hipStreamSynchronize(d.copy);
    d.pin[0].release();
    d.pin[1].release();
    d.vout.release();
  }
  d.pinned = pinned;
}

int init_device(Device& d) {
  HIP_OK(hipSetDevice(d.ord));
  HIP_OK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  d.ws[0].stream = d.stream;
  HIP_OK(hipStreamCreateWithFlags(&d.ws[1].stream, hipStreamNonBlocking));
  HIP_OK(hipStreamCreateWithFlags(&d.copy, hipStreamNonBlocking));
  HIP_OK(hipEventCreateWithFlags(&d.copied, hipEventDisableTiming));
  for (auto& e : d.staged) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_OK(hipEventCreateWithFlags(&d.keys_ready, hipEventDisableTiming));
  HIP_OK(hipEventCreateWithFlags(&d.joined, hipEventDisableTiming));
  for (auto& w : d.ws) HIP_OK(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
  for (int i = 0; i < 2; ++i) {
    HIP_OK(hipStreamCreateWithFlags(&d.kside[i], hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&d.kfork[i], hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&d.kjoin[i], hipEventDisableTiming));
  }
  d.zc_in.flags = d.zc_out.flags = d.zc_flag.flags = hipHostMallocCoherent | hipHostMallocMapped;
  apply_tuning(d, g_tune);
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, d.ord));
  d.cu_count = prop.multiProcessorCount;
  HIP_OK(d.btab.ensure(pv::BTAB_CHUNKS * pv::BTAB_ENTRIES * pv::BTAB_WORDS));
  HIP_OK(pv::launch_btable_init(d.btab.p, d.stream));
  HIP_OK(d.bw.ensure(pv::BWTAB_WORDS));
  HIP_OK(pv::launch_bw_init(d.bw.p, d.stream));
  // persistent curve grid: resident blocks per CU from the occupancy query
  // (kept <= 4 blocks of 256 threads per CU, see cdna_hip_programming.md §1)
  int per_cu = 0;
  HIP_OK(pv::curve_occupancy(&per_cu));
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 4) per_cu = 4;
  d.curve_blocks = d.cu_count * per_cu;
  int halfper = 0;
  HIP_OK(pv::curve_half_occupancy(&halfper));
  if (halfper < 1) halfper = 1;
  if (halfper > 4) halfper = 4;
  d.curve_half_blocks = d.cu_count * halfper;
  {
    const size_t a = (size_t)d.curve_blocks * pv::ATAB_WORDS, b = (size_t)d.curve_half_blocks * pv::HALF_SCRATCH_WORDS;
    d.scratch_words = (a > b ? a : b) * pv::CURVE_BLOCK;
    HIP_OK(d.ws[0].scratch.ensure(d.scratch_words));
  }
  HIP_OK(d.ws[0].qc.ensure(2));
  int kper = 0;
  HIP_OK(pv::curve_occupancy(&kper, true));
  if (kper < 1) kper = 1;
  if (kper > per_cu) kper = per_cu;
  d.curve_blocks_keyed = d.cu_count * kper;
  int sper = 0;
  HIP_OK(pv::sha256_occupancy(&sper));
  d.sha256_blocks = d.cu_count * (sper < 1 ? 1 : sper);
  int kper3 = 0;
  HIP_OK(pv::sha3_occupancy(&kper3));
  d.sha3_blocks = d.cu_count * (kper3 < 1 ? 1 : kper3);
  int hper = 0;
  HIP_OK(pv::hash_occupancy(&hper));
  if (hper < 1) hper = 1;
  d.hash_blocks = d.cu_count * hper;
  HIP_OK(d.counter.ensure(1));
  HIP_OK(d.ws[0].counter.ensure(1));
  for (auto& e : d.ev) HIP_OK(hipEventCreate(&e));
  HIP_OK(hipStreamSynchronize(d.stream));
  return PV_OK;
}

void release_device(Device& d) {
  if (d.id < 0) return;
  (void)hipSetDevice(d.ord);
  for (auto& w : d.ws)
    if (w.stream) (void)hipStreamSynchronize(w.stream);
  for (int i = 0; i < 2; ++i) {
    if (d.kside[i]) (void)hipStreamSynchronize(d.kside[i]), (void)hipStreamDestroy(d.kside[i]);
    if (d.kfork[i]) (void)hipEventDestroy(d.kfork[i]);
    if (d.kjoin[i]) (void)hipEventDestroy(d.kjoin[i]);
    d.kside[i] = nullptr;
    d.kfork[i] = d.kjoin[i] = nullptr;
  }
  d.btab.release(); d.bw.release(); d.counter.release();
  for (auto& w : d.ws) w.release();
  if (d.ws[1].stream) (void)hipStreamDestroy(d.ws[1].stream);
  for (auto& w : d.ws) w.stream = nullptr;
  d.pk.release(); d.sig.release(); d.blob.release(); d.verdict.release(); d.tamper.release(); d.stage.release();
  d.off.release(); d.batch_off.release();
  d.sender.release(); d.votes.release(); d.reached.release(); d.scan.release(); d.tflag.release(); d.tbits.release();
  d.ktab.release(); d.kidx.release(); d.kscr.release(); d.kscr2.release(); d.mk0.release(); d.mk1.release();
  d.kc.release(); d.kcpk.release();
  d.kc_count = 0;
  for (auto& e : d.ev)
    if (e) (void)hipEventDestroy(e), e = nullptr;
  for (auto& r : d.live_pool)
    for (auto& e : r.e)
      if (e) (void)hipEventDestroy(e), e = nullptr;
  d.live_pool.clear();
  d.live_used = 0;
  if (d.copied) (void)hipEventDestroy(d.copied);
  d.copied = nullptr;
  if (d.copy) (void)hipStreamSynchronize(d.copy), (void)hipStreamDestroy(d.copy);
  for (auto& e : d.staged)
    if (e) (void)hipEventDestroy(e), e = nullptr;
  if (d.keys_ready) (void)hipEventDestroy(d.keys_ready);
  d.keys_ready = nullptr;
  if (d.joined) (void)hipEventDestroy(d.joined);
  d.joined = nullptr;
  d.dl.release(); d.dlc.release();
  d.pin[0].release();
  d.pin[1].release();
  d.zc_in.release();
  d.zc_out.release();
  d.zc_flag.release();
  d.zc_done.release();
  d.zc_done_armed = false;
  d.vout.release();
  if (d.pool) d.pool->shutdown();
  d.copy = nullptr;
  if (d.stream) (void)hipStreamDestroy(d.stream);
  d.stream = nullptr;
  d.id = -1;
}

// fold the recorded live-timing events into the sums (waits for them)
int resolve_live(Device& d) {
  for (size_t k = 0; k < d.live_used; ++k) {
    hipEvent_t* e = d.live_pool[k].e;
    HIP_OK(hipEventSynchronize(e[2]));
    float a = 0, b = 0, c = 0;
    HIP_OK(hipEventElapsedTime(&a, e[0], e[1]));
    HIP_OK(hipEventElapsedTime(&b, e[1], e[2]));
    HIP_OK(hipEventElapsedTime(&c, e[0], e[3]));
    d.live_hash += a;
    d.live_sha += c;
    d.live_curve += b;
  }
  d.live_used = 0;
  return PV_OK;
}

// The two stages of a verify for device-resident inputs, on stream s with
// workspace w.  prep: pre-checks + SHA-512 (+ the lattice stage of the
// half-size path); curve: the curve kernel writing verdicts + bitmap.
// `bm` = the caller's bitmap or null (then w.bitmap).
uint64_t* stage_bitmap(Workspace& w, uint64_t* bitmap, uint64_t n, int& rc) {
  rc = PV_OK;
  if (bitmap) return bitmap;
  const hipError_t e = w.bitmap.ensure((n + 63) / 64);
  if (e != hipSuccess)
    rc = fail(e == hipErrorOutOfMemory ? PV_ENOMEM : PV_EIO, "bitmap allocation failed: %s", hipGetErrorString(e));
  return w.bitmap.p;
}

// small generic batches: the whole verify is one k_verify_quad launch
bool lat_fused(const Device& d, const uint32_t* ktab, uint64_t n) {
  return !ktab && d.mode != CurveMode::Grouped && n <= d.lat_max && d.lat_quad;
}
// small keyed batches: one k_verify_quad_keyed launch
bool lat_keyed(const Device& d, const uint32_t* ktab, uint64_t n, bool wide) {
  return ktab && !wide && n <= d.lat_keyed_max && d.lat_quad;
}

int enqueue_prep(Device& d, Workspace& w, const uint8_t* pk, const uint8_t* sig, const uint8_t* blob,
                 const uint64_t* off, uint64_t n, uint64_t* bm, hipStream_t s, const uint32_t* ktab,
                 const uint32_t* kidx, bool wide, hipEvent_t sha_ev = nullptr) {
  if (lat_keyed(d, ktab, n, wide)) {   // k_verify_quad_keyed runs the whole verify
    if (sha_ev) HIP_OK(hipEventRecord(sha_ev, s));
    return PV_OK;
  }
  if (lat_fused(d, ktab, n)) {
    // k_verify_quad runs the whole verify; only the deferred counter is reset
    HIP_OK(w.qc.ensure(2));
    HIP_OK(hipMemsetAsync(w.qc.p, 0, sizeof(unsigned long long), s));
    if (sha_ev) HIP_OK(hipEventRecord(sha_ev, s));
    return PV_OK;
  }
  HIP_OK(w.h.ensure(n * 16));
  HIP_OK(w.pre.ensure(n));
  HIP_OK(w.counter.ensure(1));
  HIP_OK(w.qc.ensure(2));
  HIP_OK(w.scratch.ensure(d.scratch_words));
  const bool half = !ktab && d.mode != CurveMode::Grouped;
  if (half) {
    if (n > 0xffffffffull) return fail(PV_EINVAL, "at most 2^32-1 signatures per device call");
    HIP_OK(w.hrec.ensure(n * pv::HSREC_WORDS));
    HIP_OK(w.dlist.ensure(n));
  }
  // the half-size path runs the pre-checks in k_lattice (k_hash hashes every
  // signature); keyed and grouped batches in k_precheck before the hash
  HIP_OK(pv::launch_hash(pk, sig, blob, off, n, w.counter.p, w.h.p, half ? nullptr : w.pre.p, d.hash_blocks, s, kidx));
  // live timing: the SHA-512 stage alone (its roofline in bench.py), before the lattice
  if (sha_ev) HIP_OK(hipEventRecord(sha_ev, s));
  if (half)
    HIP_OK(pv::launch_lattice(pk, sig, w.h.p, w.pre.p, n, w.hrec.p, w.dlist.p, w.qc.p, w.qc.p + 1, bm,
                              d.mode == CurveMode::Full, s));
  return PV_OK;
}

int enqueue_curve(Device& d, Workspace& w, const uint8_t* pk, const uint8_t* sig, const uint8_t* blob,
                  const uint64_t* off, uint64_t n, uint8_t* verdict, uint64_t* bm, hipStream_t s, const uint32_t* ktab,
                  const uint32_t* kidx, bool wide) {
  const bool half = !ktab && d.mode != CurveMode::Grouped;
  if (lat_keyed(d, ktab, n, wide)) {
    // small keyed batch: one launch, the comb split over the signature's two
    // lane quads (the hashed key bytes are pk[kidx[i]])
    HIP_OK(pv::launch_verify_quad_keyed(pk, true, sig, blob, off, n, nullptr, ktab, kidx, d.bw.p, verdict, bm, s));
  } else if (lat_fused(d, ktab, n)) {
    // small batch: one launch, 8 lanes per signature (each point on a lane
    // quad) plus one hashing lane per signature in a second wave
    HIP_OK(pv::launch_verify_quad(pk, sig, blob, off, n, d.bw.p, verdict, bm, w.qc.p, d.mode == CurveMode::Full, s));
    w.half_ran = true;
    d.last_ws = (int)(&w - d.ws);
  } else if (half && n <= d.lat_max) {
    // (PV_LAT_PAIR) lane pairs per signature, one table of scratch per lane
    HIP_OK(w.scratch.ensure(std::max<size_t>(d.scratch_words, (size_t)((2 * n + 63) / 64 * 64) * pv::ATAB_LAT_WORDS)));
    HIP_OK(pv::launch_curve_lat(pk, sig, w.h.p, w.hrec.p, d.btab.p, d.bw.p, w.scratch.p,
                                w.scratch.cap / pv::ATAB_LAT_WORDS, verdict, bm, n, s));
    w.half_ran = true;
    d.last_ws = (int)(&w - d.ws);
  } else if (half) {
    HIP_OK(pv::launch_curve_half(pk, sig, w.h.p, w.hrec.p, d.btab.p, d.bw.p, w.scratch.p,
                                 w.scratch.cap / pv::HALF_SCRATCH_WORDS, verdict, bm, n, w.dlist.p, w.qc.p, w.qc.p + 1,
                                 d.curve_half_blocks, s));
    w.half_ran = true;
    d.last_ws = (int)(&w - d.ws);
  } else {
    HIP_OK(pv::launch_curve(pk, sig, w.h.p, w.pre.p, d.btab.p, w.scratch.p, w.scratch.cap / pv::ATAB_WORDS, verdict,
                            bm, n, ktab ? d.curve_blocks_keyed : d.curve_blocks, s, ktab, kidx, d.bw.p, w.qc.p + 1,
                            wide));
  }
  return PV_OK;
}

// enqueue hash + curve for device-resident inputs on stream s with workspace w
int enqueue_verify(Device& d, Workspace& w, const uint8_t* pk, const uint8_t* sig, const uint8_t* blob,
                   const uint64_t* off, uint64_t n, uint8_t* verdict, uint64_t* bitmap, hipStream_t s, bool timed,
                   float* ms_hash, float* ms_curve, const uint32_t* ktab = nullptr, const uint32_t* kidx = nullptr,
                   bool wide = false, hipEvent_t curve_after = nullptr) {
  if (n == 0) return PV_OK;
  const bool live = !timed && d.live_timing;
  hipEvent_t* lev = nullptr;
  if (live) {
    if (d.live_used == d.live_pool.size() && d.live_used >= 256) {
      const int rc = resolve_live(d);
      if (rc) return rc;
    }
    if (d.live_used == d.live_pool.size()) {
      d.live_pool.emplace_back();
      for (auto& e : d.live_pool.back().e) HIP_OK(hipEventCreate(&e));
    }
    lev = d.live_pool[d.live_used++].e;
    ++d.live_launches;
  }
  WsUse use(w, s);
  if (use.rc) return use.rc;
  int rc = PV_OK;
  uint64_t* bm = stage_bitmap(w, bitmap, n, rc);
  if (rc) return rc;
  if (timed) HIP_OK(hipEventRecord(d.ev[0], s));
  if (lev) HIP_OK(hipEventRecord(lev[0], s));
  rc = enqueue_prep(d, w, pk, sig, blob, off, n, bm, s, ktab, kidx, wide, lev ? lev[3] : nullptr);
  if (rc) return rc;
  // the "hash" interval also holds the scalar stage of the half-size path
  if (timed) HIP_OK(hipEventRecord(d.ev[1], s));
  if (lev) HIP_OK(hipEventRecord(lev[1], s));
  // keys prepared on a side stream (pv_verify_keys_device_async): the curve
  // kernel reads their tables
  if (curve_after) HIP_OK(hipStreamWaitEvent(s, curve_after, 0));
  rc = enqueue_curve(d, w, pk, sig, blob, off, n, verdict, bm, s, ktab, kidx, wide);
  if (rc) return rc;
  rc = use.end();
  if (rc) return rc;
  if (lev) HIP_OK(hipEventRecord(lev[2], s));
  if (timed) {
    HIP_OK(hipEventRecord(d.ev[2], s));
    HIP_OK(hipEventSynchronize(d.ev[2]));
    float a = 0, b = 0;
    HIP_OK(hipEventElapsedTime(&a, d.ev[0], d.ev[1]));
    HIP_OK(hipEventElapsedTime(&b, d.ev[1], d.ev[2]));
    if (ms_hash) *ms_hash += a;
    if (ms_curve) *ms_curve += b;
  }
  return PV_OK;
}

struct HostBatch {
  const uint8_t* pk;
  const uint8_t* sig;
  const uint8_t* blob;
  const uint64_t* off;
  uint8_t* verdict;
  uint32_t flags;
};

// One device's shard [s, e) of a host-buffer batch (pv_verify_batch), on the
// calling thread: key dedup and buffers, then a pipeline of chunks.  Chunk c's
// inputs are gathered by host threads into page-locked slot c & 1 (its
// offsets rebased to the shard and checked while they are copied), DMA'd on
// the copy stream, and verified on workspace c & 1's stream (see the loop).
// Verdicts come back through a page-locked buffer.  Returns after every verdict of the
// shard is in hb.verdict (or on error, after the device has drained).
// A shard of a Looper-pass size (m <= lat_max: the one-launch latency kernel).
// The inputs are gathered into page-locked slot 0 in the layout off | pk | sig
// | blob | 16 zero bytes, DMA'd with ONE copy into the device image `stage`,
// verified by one k_verify_quad launch and the verdicts copied back, all on
// workspace 0's stream (no copy stream, no cross-stream events).  Keys are
// never deduplicated here: the latency kernel beats preparing them (same
// verdicts).  Returns 1 when the shard does not fit the path (caller falls
// back to the pipeline).
// [p, p + n) lies inside one page-locked host allocation (hipHostMalloc'd or
// registered by the caller, e.g. torch pin_memory()), so the copy engine can
// read it directly and the gather into the staging ring can be skipped
bool host_locked(const void* p, size_t n) {
  if (n == 0) return true;
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (a.type != hipMemoryTypeHost) return false;
  void* start = nullptr;
  size_t size = 0;
  hipDeviceptr_t dp = const_cast<void*>(p);
  if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, dp) != hipSuccess ||
      hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, dp) != hipSuccess || !start) {
    (void)hipGetLastError();
    return false;
  }
  return static_cast<const char*>(p) >= static_cast<const char*>(start) &&
         static_cast<const char*>(p) + n <= static_cast<const char*>(start) + size;
}

uint64_t small_bytes(const HostBatch& hb, uint64_t s, uint64_t e) {
  const uint64_t m = e - s;
  // + the key-cache tail: 8-byte alignment, list count, kidx and the two lists
  return (m + 1) * 8 + m * 96 + (hb.off[e] - hb.off[s]) + 16 + 16 + 8 * m;
}

// all-cached zero-copy calls up to this size complete by the keyed kernel's own
// word: 64 signatures = the 16 blocks of 4 that profiles/r05_ab_completion_word.jsonl
// measured faster than a k_signal launch (125 blocks measured slower)
constexpr uint64_t ZC_SELF_MAX = 64;
// spin budget of the completion word before the stream synchronize takes over
// (pv_test_set_spin_ns shortens it so a test reaches the fallback)
std::atomic<int64_t> g_zc_spin_ns{20'000'000};
// spins until *w == v (acquire) or `ns` nanoseconds have passed
bool spin_wait_word(const uint32_t* w, uint32_t v, int64_t ns) {
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 0;; ++i) {
    if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == v) return true;
    if ((i & 255u) == 255u &&
        std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() > ns)
      return false;
  }
}

int run_small(Device& d, const HostBatch& hb, uint64_t s, uint64_t e) {
  const uint64_t m = e - s;
  HIP_OK(hipSetDevice(d.ord));
  Workspace& w = d.ws[0];
  struct Drain {
    Device& d;
    bool done = false;   // the call's work is known complete (zero-copy completion word)
    ~Drain() {
      if (done) return;
      (void)hipSetDevice(d.ord);
      (void)hipStreamSynchronize(d.ws[0].stream);
    }
  } drain{d};
  const uint64_t b0 = hb.off[s], bytes = hb.off[e] - b0;
  const size_t o_pk = (m + 1) * 8, o_sig = o_pk + m * 32, o_blob = o_sig + m * 64, total = small_bytes(hb, s, e);
  // zero-copy: the kernels read the image from and write the verdicts to
  // fine-grained host memory (no copy launches); else one H2D into `stage`
  // and one D2H of the verdicts
  const bool zc = m <= d.zc_max;
  PinBuf& pin = zc ? d.zc_in : d.pin[0];
  PinBuf& vout = zc ? d.zc_out : d.vout;
  if (pin.ensure(total) != hipSuccess || vout.ensure(m) != hipSuccess) {
    (void)hipGetLastError();
    return 1;
  }
  uint8_t* base = pin.p;
  const uint8_t* g = nullptr;
  uint8_t* vdst = nullptr;
  if (zc) {
    g = pin.dev;
    vdst = vout.dev;
  } else {
    HIP_OK(d.stage.ensure(total));
    HIP_OK(d.verdict.ensure(m));
    g = d.stage.p;
    vdst = d.verdict.p;
  }
  std::atomic<bool> bad{false};
  const CopyJob jobs[4] = {{base, reinterpret_cast<const uint8_t*>(hb.off + s), (m + 1) * 8, b0, true},
                           {base + o_pk, hb.pk + 32 * s, m * 32},
                           {base + o_sig, hb.sig + 64 * s, m * 64},
                           {base + o_blob, hb.blob ? hb.blob + b0 : nullptr, bytes}};
  d.pool->run(jobs, 4, d.copy_threads, &bad);
  if (bad.load())
    return fail(PV_EINVAL, "msg_off not monotone in [%llu, %llu]", (unsigned long long)s, (unsigned long long)e);
  memset(base + o_blob + bytes, 0, 16);   // the hash reads aligned words past the last message
  // keys in the persistent key cache (pv_keycache_add): those signatures run
  // the keyed latency kernel over a list, the others k_verify_quad_list; the
  // image gets a tail of the uncached count, kidx[m] and the two lists (cached
  // indices from the front, uncached from the back)
  const size_t o_ext = (o_blob + bytes + 16 + 7) & ~size_t(7);
  uint64_t nk = 0, ng = 0;
  if (g_kc.count() && d.kc_count == g_kc.count() && d.lat_keyed_max && d.lat_quad) {
    uint32_t* kidx = reinterpret_cast<uint32_t*>(base + o_ext + 8);
    uint32_t* kl = kidx + m;
    for (uint64_t i = 0; i < m; ++i) {
      const uint32_t sl = g_kc.find(hb.pk + 32 * (s + i));
      kidx[i] = sl == UINT32_MAX ? 0u : sl;
      if (sl != UINT32_MAX) kl[nk++] = (uint32_t)i;
      else kl[m - 1 - ng++] = (uint32_t)i;
    }
    *reinterpret_cast<uint64_t*>(base + o_ext) = ng;
  }
  // zero-copy calls complete by a word in fine-grained host memory that the host
  // polls (~5 us below a stream synchronize, tools/ubench/sync_lat.hip): an
  // all-cached call's keyed kernel writes it from its last block, other calls
  // end with a k_signal launch
  const bool poll = zc;
  uint32_t seq = 0;
  bool signalled = false;
  if (poll) {
    const bool fresh = d.zc_flag.p == nullptr;
    HIP_OK(d.zc_flag.ensure(64));
    // hipHostMalloc leaves the contents unspecified (recycled pinned pages after a
    // shutdown / init cycle): a stale word equal to the first seq would complete
    // the call before the kernel ran
    if (fresh) {
      __atomic_store_n(reinterpret_cast<uint32_t*>(d.zc_flag.p), 0u, __ATOMIC_RELEASE);
      d.zc_seq = 0;
    }
    if (++d.zc_seq == 0) d.zc_seq = 1;
    seq = d.zc_seq;
  }
  if (nk) {
    const size_t total_ext = o_ext + 8 + 8 * m;
    if (!zc) HIP_OK(hipMemcpyAsync(d.stage.p, base, total_ext, hipMemcpyHostToDevice, w.stream));
    WsUse use(w, w.stream);
    if (use.rc) return use.rc;
    const uint64_t* goff = reinterpret_cast<const uint64_t*>(g);
    const uint32_t* kidx = reinterpret_cast<const uint32_t*>(g + o_ext + 8);
    // up to 16 blocks: measured 2-3 us faster than a k_signal launch; at 125
    // blocks 3-4 us slower (every comb wave's system-scope fence and the
    // counter), profiles/r05_ab_completion_word.jsonl
    const bool self = poll && ng == 0 && nk <= ZC_SELF_MAX;
    if (self && !d.zc_done_armed) {
      HIP_OK(d.zc_done.ensure(1));
      HIP_OK(hipMemsetAsync(d.zc_done.p, 0, sizeof(uint32_t), w.stream));
      d.zc_done_armed = true;
    }
    HIP_OK(pv::launch_verify_quad_keyed(g + o_pk, false, g + o_sig, g + o_blob, goff, nk, kidx + m, d.kc.p, kidx,
                                        d.bw.p, vdst, nullptr, w.stream, self ? d.zc_done.p : nullptr,
                                        self ? reinterpret_cast<uint32_t*>(d.zc_flag.dev) : nullptr, seq));
    signalled = self;
    if (ng)
      HIP_OK(pv::launch_verify_quad_list(g + o_pk, g + o_sig, g + o_blob, goff, kidx + 2 * m - ng,
                                         reinterpret_cast<const unsigned long long*>(g + o_ext), ng, (int)((ng + 7) / 8),
                                         d.bw.p, vdst, d.mode == CurveMode::Full, w.stream));
    if (const int rc = use.end()) return rc;
  } else {
    if (!zc) HIP_OK(hipMemcpyAsync(d.stage.p, base, total, hipMemcpyHostToDevice, w.stream));
    const int rc = enqueue_verify(d, w, g + o_pk, g + o_sig, g + o_blob, reinterpret_cast<const uint64_t*>(g), m,
                                  vdst, nullptr, w.stream, false, nullptr, nullptr);
    if (rc) return rc;
  }
  if (poll) {
    // past the spin budget (a fault, a long queue) the synchronize reports /
    // waits as before
    if (!signalled) HIP_OK(pv::launch_signal(reinterpret_cast<uint32_t*>(d.zc_flag.dev), seq, w.stream));
    drain.done = spin_wait_word(reinterpret_cast<const uint32_t*>(d.zc_flag.p), seq,
                                 g_zc_spin_ns.load(std::memory_order_relaxed));
    if (!drain.done) HIP_OK(hipStreamSynchronize(w.stream));
  } else {
    if (!zc) HIP_OK(hipMemcpyAsync(vout.p, d.verdict.p, m, hipMemcpyDeviceToHost, w.stream));
    HIP_OK(hipStreamSynchronize(w.stream));
  }
  memcpy(hb.verdict + s, vout.p, m);
  return PV_OK;
}

int run_shard(Device& d, const HostBatch& hb, uint64_t s, uint64_t e) {
  // before any size arithmetic: a shard whose end offset lies below its start
  // would wrap bytes + 16 (the per-chunk checks come later)
  if (hb.off[e] < hb.off[s])
    return fail(PV_EINVAL, "msg_off not monotone in [%llu, %llu]", (unsigned long long)s, (unsigned long long)e);
  const uint64_t m = e - s;
  if (m == 0) return PV_OK;
  if (m <= d.lat_max && d.lat_quad && d.mode != CurveMode::Grouped && d.pinned &&
      small_bytes(hb, s, e) <= d.pin_max) {
    const int rc = run_small(d, hb, s, e);
    if (rc != 1) return rc;
  }
  HIP_OK(hipSetDevice(d.ord));
  // on every exit (errors included) wait for the work that reads host memory
  struct Drain {
    Device& d;
    ~Drain() {
      (void)hipSetDevice(d.ord);
      (void)hipStreamSynchronize(d.copy);
      for (auto& w : d.ws) (void)hipStreamSynchronize(w.stream);
    }
  } drain{d};
  // async batches may still hold either workspace on a caller's stream
  for (auto& w : d.ws) {
    const int rc = ws_begin(w, w.stream);
    if (rc) return rc;
  }
  const uint8_t* pk = hb.pk;
  const uint64_t b0 = hb.off[s], bytes = hb.off[e] - b0;
  // PV_FLAG_DEDUP_KEYS: prepare each distinct key once (cached multiples of
  // -A) when at least half of the shard's signatures repeat a key
  std::vector<uint8_t> upk;
  std::vector<uint32_t> idx;
  uint64_t nk = m;
  if (hb.flags & PV_FLAG_DEDUP_KEYS) {
    // a sample first: s keys (one at a pseudo-random position in each of s
    // equal strides, so positions never repeat) from a pool of <= m/2
    // distinct keys in even use repeat ~s^2/m times; a sample with under a
    // quarter of that means mostly distinct keys, and the full pass is
    // skipped (the choice only affects speed, never verdicts)
    KeyIndex ki;
    bool dedup = true;
    if (m >= PV_DEDUP_SAMPLE_MIN) {
      uint64_t smp = 8;
      while (smp * smp < 64 * m) smp <<= 1;  // s >= 8 sqrt(m): ~64 expected repeats at the threshold
      const uint64_t stride = m / smp;
      ki.reset(pk + 32 * s, m);
      for (uint64_t j = 0; j < smp; ++j) {
        uint64_t x = (j + 1) * 0x9E3779B97F4A7C15ull;
        x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
        x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
        ki.insert(j * stride + (x ^ (x >> 31)) % stride);
      }
      dedup = 4 * (smp - ki.first.size()) * m >= smp * smp;
    }
    if (dedup) {
      ki.reset(pk + 32 * s, m);
      idx.resize(m);
      for (uint64_t k = 0; k < m && 2 * ki.first.size() <= m; ++k) idx[k] = ki.insert(k);
      nk = ki.first.size();
      if (2 * nk > m) {
        nk = m;
        idx.clear();
      } else {
        upk.resize(nk * 32);
        for (uint64_t j = 0; j < nk; ++j) memcpy(upk.data() + 32 * j, pk + 32 * (s + ki.first[j]), 32);
      }
    }
  }
  const bool keyed = !idx.empty();
  HIP_OK(d.pk.ensure((keyed ? nk : m) * 32));
  HIP_OK(d.sig.ensure(m * 64));
  HIP_OK(d.blob.ensure(bytes + 16));
  HIP_OK(d.off.ensure(m + 1));
  HIP_OK(d.verdict.ensure(m));
  // chunk bounds: short leading chunks so the kernels start early -- the
  // ramp r, 2r, ... below a regular chunk (default), or with host_ramp 0
  // one first chunk of first_pct % of a regular one (>= PV_HOST_CHUNK_MIN) --
  // then the rest in equal chunks.  With pinned
  // staging the chunk count doubles until a chunk's inputs fit one
  // pin_max slot; a shard whose PV_HOST_CHUNK_MIN-signature chunks still do not
  // fit (or whose page-locked allocation fails) uses pageable staging.
  auto chunk_bytes = [&](uint64_t c0, uint64_t c1) -> size_t {
    return (c1 - c0 + 1) * 8 + (keyed ? 0 : (c1 - c0) * 32) + (c1 - c0) * 64 + (hb.off[s + c1] - hb.off[s + c0]);
  };
  std::vector<uint64_t> bounds;
  size_t cap = 0;
  for (uint64_t hc = d.host_chunks;; hc *= 2) {
    const uint64_t reg = std::max<uint64_t>(PV_HOST_CHUNK_MIN, (m + hc - 1) / hc);
    const uint64_t first = std::min(m, std::max<uint64_t>(PV_HOST_CHUNK_MIN, reg * (uint64_t)d.first_pct / 100));
    bounds.assign(1, 0);
    if (hc > 1 && d.ramp) {
      // tuning.host_ramp = r: leading chunks of r, 2r, 4r, ... signatures (< a
      // regular chunk), so the first kernels start after a short DMA
      for (uint64_t r = d.ramp; r < reg && bounds.back() + r < m; r *= 2) bounds.push_back(bounds.back() + r);
    } else if (hc > 1 && first < m) {
      bounds.push_back(first);
    }
    const uint64_t rest = m - bounds.back();
    const uint64_t k = std::max<uint64_t>(1, std::min<uint64_t>((rest + reg - 1) / reg, rest / PV_HOST_CHUNK_MIN));
    const uint64_t c0 = bounds.back();
    for (uint64_t j = 1; j <= k; ++j) bounds.push_back(c0 + rest * j / k);
    cap = 0;
    for (size_t j = 1; j < bounds.size(); ++j) cap = std::max(cap, chunk_bytes(bounds[j - 1], bounds[j]));
    if (!d.pinned || cap <= d.pin_max || reg == PV_HOST_CHUNK_MIN || hc >= 4096) break;
  }
  const size_t nch = bounds.size() - 1;
  // chunk sizes come from the offsets at the chunk bounds: check those before
  // anything is sized from them (each chunk's offsets are checked as they are copied)
  for (size_t j = 1; j < bounds.size(); ++j)
    if (hb.off[s + bounds[j]] < hb.off[s + bounds[j - 1]])
      return fail(PV_EINVAL, "msg_off not monotone in [%llu, %llu]", (unsigned long long)(s + bounds[j - 1]),
                  (unsigned long long)(s + bounds[j]));
  bool pinned = d.pinned && cap <= d.pin_max;
  if (pinned && (d.pin[0].ensure(cap) != hipSuccess || d.pin[1].ensure(cap) != hipSuccess ||
                 d.vout.ensure(m) != hipSuccess)) {
    (void)hipGetLastError();
    d.pin[0].release();
    d.pin[1].release();
    d.vout.release();
    pinned = false;
  }
  std::vector<uint64_t> offs;  // pageable staging: the shard's rebased offsets (read by in-flight copies)
  if (!pinned) offs.resize(m + 1);
  // caller buffers already page-locked: DMA pk / sig / blob straight from them,
  // only the offsets (rebased, checked) go through the staging ring
  const bool direct = pinned && !keyed && host_locked(pk + 32 * s, m * 32) && host_locked(hb.sig + 64 * s, m * 64) &&
                      host_locked(hb.blob ? hb.blob + b0 : nullptr, bytes);
  HIP_OK(hipMemsetAsync(d.blob.p + bytes, 0, 16, d.copy));
  // generic batches: one fused launch per chunk, deferred records listed for
  // one lane-quad pass at the end (its count is zeroed on the copy stream,
  // which every chunk's kernels wait for)
  // (PV_CURVE_MODE=full: every record deferred, i.e. verified by the list pass)
  const bool fused = !keyed && d.chunk_fused && d.mode != CurveMode::Grouped;
  if (fused) {
    if (m > 0xffffffffull) return fail(PV_EINVAL, "at most 2^32-1 signatures per device call");
    HIP_OK(d.dl.ensure(m));
    HIP_OK(d.dlc.ensure(1));
    HIP_OK(hipMemsetAsync(d.dlc.p, 0, sizeof(unsigned long long), d.copy));
    for (auto& w : d.ws) w.half_ran = false;   // pv_curve_stats describes device-resident calls
  }
  if (keyed) {
    HIP_OK(d.ktab.ensure(nk * pv::KEYTAB_WORDS));
    HIP_OK(d.kidx.ensure(m));
    HIP_OK(d.kscr.ensure((nk + 63) / 64 * 64 * pv::KEYTAB_SCRATCH));   // lane-interleaved per 64 keys
    HIP_OK(hipMemcpyAsync(d.pk.p, upk.data(), nk * 32, hipMemcpyHostToDevice, d.copy));
    HIP_OK(hipMemcpyAsync(d.kidx.p, idx.data(), m * 4, hipMemcpyHostToDevice, d.copy));
    HIP_OK(hipEventRecord(d.copied, d.copy));
    HIP_OK(hipStreamWaitEvent(d.ws[0].stream, d.copied, 0));
    HIP_OK(pv::launch_keys(d.pk.p, nk, d.ktab.p, d.kscr.p, d.ws[0].stream));
    HIP_OK(hipEventRecord(d.keys_ready, d.ws[0].stream));
    HIP_OK(hipStreamWaitEvent(d.ws[1].stream, d.keys_ready, 0));
  }
  // tuning.host_trace: per-chunk host timings on stderr (pipeline diagnostics)
  const bool trace = g_tune.host_trace != 0;
  const auto tstart = std::chrono::steady_clock::now();
  auto us = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tstart).count(); };
  if (trace) fprintf(stderr, "[pv host] dev %d shard %llu sigs: setup %.1f us, %zu chunks, pinned %d, direct %d\n", d.id,
                     (unsigned long long)m, us(), nch, (int)pinned, (int)direct);
  // chunk c is verified on workspace c & 1 and its stream, so chunk c + 1's
  // kernels start while chunk c's curve grid drains.  (A separate prep stream
  // for every chunk's hash + lattice with three workspaces measured no better:
  // squeezed into the slots the curve grids leave, the prep kernels of a chunk
  // take ~1.1 ms either way -- profiles/r02_e2e_timeline_prepstream_notadopted.txt.)
  for (size_t c = 0; c < nch; ++c) {
    const uint64_t c0 = bounds[c], c1 = bounds[c + 1], mc = c1 - c0;
    Workspace& w = d.ws[c & 1];
    const double t_begin = trace ? us() : 0;
    double t_slot = 0, t_gather = 0;
    const uint64_t cb0 = hb.off[s + c0] - b0, cbytes = hb.off[s + c1] - hb.off[s + c0];
    const uint8_t* src_pk = pk + 32 * (s + c0);
    const uint8_t* src_sig = hb.sig + 64 * (s + c0);
    const uint8_t* src_blob = hb.blob ? hb.blob + b0 + cb0 : nullptr;
    const uint8_t* src_off;
    std::atomic<bool> bad{false};
    if (pinned) {
      // gather the chunk into slot c & 1 once its previous H2D (chunk c - 2) is done
      const int slot = (int)(c & 1);
      if (c >= 2) HIP_OK(hipEventSynchronize(d.staged[slot]));
      if (trace) t_slot = us();
      uint8_t* base = d.pin[slot].p;
      uint8_t *p_off = base, *p_pk = p_off + (mc + 1) * 8, *p_sig = p_pk + (keyed ? 0 : mc * 32),
              *p_blob = p_sig + mc * 64;
      const CopyJob jobs[4] = {{p_off, reinterpret_cast<const uint8_t*>(hb.off + s + c0), (mc + 1) * 8, b0, true},
                               {p_pk, src_pk, keyed ? 0 : mc * 32},
                               {p_sig, src_sig, mc * 64},
                               {p_blob, src_blob, cbytes}};
      d.pool->run(jobs, direct ? 1 : 4, d.copy_threads, &bad);
      if (trace) t_gather = us();
      src_off = p_off;
      if (!direct) {
        src_pk = p_pk;
        src_sig = p_sig;
        src_blob = p_blob;
      }
    } else {
      const CopyJob job{reinterpret_cast<uint8_t*>(offs.data() + c0), reinterpret_cast<const uint8_t*>(hb.off + s + c0),
                        (mc + 1) * 8, b0, true};
      gather_range(&job, 1, 0, job.n, &bad);
      src_off = reinterpret_cast<const uint8_t*>(offs.data() + c0);
    }
    if (bad.load()) return fail(PV_EINVAL, "msg_off not monotone in [%llu, %llu]", (unsigned long long)(s + c0),
                                (unsigned long long)(s + c1));
    if (!keyed) HIP_OK(hipMemcpyAsync(d.pk.p + 32 * c0, src_pk, mc * 32, hipMemcpyHostToDevice, d.copy));
    HIP_OK(hipMemcpyAsync(d.sig.p + 64 * c0, src_sig, mc * 64, hipMemcpyHostToDevice, d.copy));
    if (cbytes) HIP_OK(hipMemcpyAsync(d.blob.p + cb0, src_blob, cbytes, hipMemcpyHostToDevice, d.copy));
    HIP_OK(hipMemcpyAsync(d.off.p + c0, src_off, (mc + 1) * 8, hipMemcpyHostToDevice, d.copy));
    if (pinned) HIP_OK(hipEventRecord(d.staged[c & 1], d.copy));
    HIP_OK(hipEventRecord(d.copied, d.copy));
    HIP_OK(hipStreamWaitEvent(w.stream, d.copied, 0));
    // blob base + shard-relative offsets: the hash kernel reads blob + off[i]
    if (fused) {
      HIP_OK(w.hrec.ensure(mc * pv::HSREC_WORDS));
      HIP_OK(w.qc.ensure(2));
      HIP_OK(w.scratch.ensure(d.scratch_words));
      HIP_OK(pv::launch_chunk_half(d.pk.p + 32 * c0, d.sig.p + 64 * c0, d.blob.p, d.off.p + c0, mc, w.hrec.p, d.bw.p,
                                   w.scratch.p, w.scratch.cap / pv::HALF_SCRATCH_WORDS, d.verdict.p + c0, d.dl.p,
                                   d.dlc.p, c0, w.qc.p + 1, d.curve_half_blocks, d.mode == CurveMode::Full, w.stream));
      if (const int rc = ws_end(w, w.stream)) return rc;
      if (trace)
        fprintf(stderr, "[pv host] chunk %zu (%llu sigs): begin %.1f slot-free %.1f gathered %.1f enqueued %.1f us\n", c,
                (unsigned long long)mc, t_begin, t_slot, t_gather, us());
      continue;
    }
    int rc = enqueue_verify(d, w, keyed ? d.pk.p : d.pk.p + 32 * c0, d.sig.p + 64 * c0, d.blob.p, d.off.p + c0, mc,
                            d.verdict.p + c0, nullptr, w.stream, false, nullptr, nullptr, keyed ? d.ktab.p : nullptr,
                            keyed ? d.kidx.p + c0 : nullptr);
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(pinned ? d.vout.p + c0 : hb.verdict + s + c0, d.verdict.p + c0, mc, hipMemcpyDeviceToHost,
                          w.stream));
    if (trace)
      fprintf(stderr, "[pv host] chunk %zu (%llu sigs): begin %.1f slot-free %.1f gathered %.1f enqueued %.1f us\n", c,
              (unsigned long long)mc, t_begin, t_slot, t_gather, us());
  }
  if (fused) {
    // the deferred records of every chunk (ws[1]'s chunks joined into ws[0]),
    // then all verdicts in one copy
    Workspace& w0 = d.ws[0];
    HIP_OK(hipEventRecord(d.joined, d.ws[1].stream));
    HIP_OK(hipStreamWaitEvent(w0.stream, d.joined, 0));
    HIP_OK(pv::launch_verify_quad_list(d.pk.p, d.sig.p, d.blob.p, d.off.p, d.dl.p, d.dlc.p, m, d.cu_count * 8, d.bw.p,
                                       d.verdict.p, d.mode == CurveMode::Full, w0.stream));
    HIP_OK(hipMemcpyAsync(pinned ? d.vout.p : hb.verdict + s, d.verdict.p, m, hipMemcpyDeviceToHost, w0.stream));
  }
  HIP_OK(hipStreamSynchronize(d.copy));
  for (auto& w : d.ws) HIP_OK(hipStreamSynchronize(w.stream));
  if (pinned) memcpy(hb.verdict + s, d.vout.p, m);
  if (trace) fprintf(stderr, "[pv host] drained %.1f us\n", us());
  return PV_OK;
}

// Key preparation on stream ks into ktab, through slot's key scratch (kscr /
// kscr2, ordered like workspace `slot`: the host pipeline prepares keys in
// kscr on ws[0]'s stream).  Wide format (radix-256 comb): KEYTAB_WIDE_LANES
// (128) lanes and 160 KB of scratch per key, verified through k_curve<true, 1>.
int keys_launch(Device& d, const uint8_t* pk, uint64_t k, uint32_t* ktab, bool wide, hipStream_t ks, int slot) {
  DevBuf<uint32_t>& scr = slot ? d.kscr2 : d.kscr;
  if (wide) {
    HIP_OK(scr.ensure(k * pv::KEYTAB_WIDE_LANES * (uint64_t)pv::KEYTAB_WIDE_SCRATCH));
    HIP_OK(pv::launch_keys_wide(pk, k, ktab, scr.p, ks));
  } else {
    HIP_OK(scr.ensure((k + 63) / 64 * 64 * pv::KEYTAB_SCRATCH));
    HIP_OK(pv::launch_keys(pk, k, ktab, scr.p, ks));
  }
  return PV_OK;
}

// ... as one use of the slot's workspace on s
int keys_prepare(Device& d, const uint8_t* pk, uint64_t k, uint32_t* ktab, bool wide, hipStream_t s, int slot) {
  WsUse use(d.ws[slot], s);
  if (use.rc) return use.rc;
  if (const int rc = keys_launch(d, pk, k, ktab, wide, s, slot)) return rc;
  return use.end();
}

// prepare keys[0 .. count) (32 bytes each) into key-cache slots [first,
// first + count) of device d, growing its table (existing slots are kept);
// synchronous.  d.kc_count is left to the caller.
int kc_prepare(Device& d, const uint8_t* keys, uint64_t first, uint64_t count) {
  if (count == 0) return PV_OK;
  HIP_OK(hipSetDevice(d.ord));
  const uint64_t need = (first + count) * (uint64_t)pv::KEYTAB_WORDS;
  if (need > d.kc.cap) {
    size_t cap = d.kc.cap ? d.kc.cap : 64 * (size_t)pv::KEYTAB_WORDS;
    while (cap < need) cap *= 2;
    DevBuf<uint32_t> nb;
    HIP_OK(nb.ensure(cap));
    if (first) {
      const hipError_t e = hipMemcpy(nb.p, d.kc.p, first * pv::KEYTAB_WORDS * sizeof(uint32_t), hipMemcpyDeviceToDevice);
      if (e != hipSuccess) {
        nb.release();
        HIP_OK(e);
      }
    }
    d.kc.release();
    d.kc = nb;
  }
  WsUse use(d.ws[0], d.stream);
  if (use.rc) return use.rc;
  HIP_OK(d.kcpk.ensure(32 * count));
  HIP_OK(hipMemcpyAsync(d.kcpk.p, keys, 32 * count, hipMemcpyHostToDevice, d.stream));
  if (const int rc = keys_launch(d, d.kcpk.p, count, d.kc.p + first * pv::KEYTAB_WORDS, false, d.stream, 0)) return rc;
  if (const int rc = use.end()) return rc;
  HIP_OK(hipStreamSynchronize(d.stream));
  return PV_OK;
}

std::vector<Device*> select_devs(uint32_t mask) {
  std::vector<Device*> v;
  for (auto& d : g_devs)
    if (mask == 0 || (mask >> d.id) & 1u) v.push_back(&d);
  return v;
}

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

int offsets_ok(const uint64_t* off, uint64_t n, const char* what) {
  for (uint64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return fail(PV_EINVAL, "%s not monotone at %llu", what, (unsigned long long)i);
  return PV_OK;
}

// bytes of src, then the 16 zero bytes the hash kernels read past the last message
int upload_padded(uint8_t* dst, const uint8_t* src, uint64_t bytes, hipStream_t s) {
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

// The pv_verify_*_device(_async) forms.  keyed: ktab / key_idx are arguments
// of the form; async: the caller names the workspace slot, passes a bitmap and
// synchronises itself.
int verify_device(bool keyed, bool wide, bool async, const uint32_t* ktab, const uint32_t* key_idx, const uint8_t* pk,
                  const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off, uint64_t n, uint8_t* verdict,
                  uint64_t* bitmap, int device, void* stream, int slot) {
  Entry en(device, slot);
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if ((keyed && (!ktab || !key_idx)) || !pk || !sig || !msg_blob || !msg_off || !verdict || (async && !bitmap))
    return fail(PV_EINVAL, "null device buffer");
  if (const int rc = en.begin(stream)) return rc;
  const int rc = enqueue_verify(*en.d, en.d->ws[slot], pk, sig, msg_blob, msg_off, n, verdict, bitmap, en.s, false,
                                nullptr, nullptr, ktab, key_idx, wide);
  return async ? rc : en.finish(rc);
}

// pv_time_verify_device / _keyed_device (ktab = key_idx = NULL: generic)
int time_verify(const uint32_t* ktab, const uint32_t* key_idx, const uint8_t* pk, const uint8_t* sig,
                const uint8_t* msg_blob, const uint64_t* msg_off, uint64_t n, uint8_t* verdict, uint64_t* bitmap,
                int device, void* stream, int iters, float* ms_hash, float* ms_curve) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (iters <= 0) return fail(PV_EINVAL, "iters must be > 0");
  if (const int rc = en.begin(stream)) return rc;
  float a = 0, b = 0;
  for (int it = 0; it < iters; ++it)
    if (const int rc = enqueue_verify(*en.d, en.d->ws[0], pk, sig, msg_blob, msg_off, n, verdict, bitmap, en.s, true,
                                      &a, &b, ktab, key_idx))
      return rc;
  if (ms_hash) *ms_hash = a / iters;
  if (ms_curve) *ms_curve = b / iters;
  return PV_OK;
}

// pv_keys_prepare(_wide)_device(_async)
int keys_prepare_device(bool wide, bool async, const uint8_t* pk, uint64_t k, uint32_t* ktab, int device, void* stream,
                        int slot) {
  Entry en(device, slot);
  if (const int rc = en.check()) return rc;
  if (k == 0) return PV_OK;
  if (!pk || !ktab) return fail(PV_EINVAL, "null device buffer");
  if (const int rc = en.begin(stream)) return rc;
  const int rc = keys_prepare(*en.d, pk, k, ktab, wide, en.s, slot);
  return async ? rc : en.finish(rc);
}

}  // namespace

extern "C" {

// engine devices 0..dup-1 all on HIP device 0 (pv_test_init_dup), else one per HIP device
static int init_devices(uint32_t device_mask, int dup) {
  DeviceGuard dg;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) return fail(PV_ENODEV, "no HIP device available (%s)", hipGetErrorString(e));
  const int n_ids = dup ? dup : count;
  for (int id = 0; id < n_ids && id < 32; ++id) {
    if (device_mask && !((device_mask >> id) & 1u)) continue;
    if (find_dev(id)) continue;
    g_devs.emplace_back();
    g_devs.back().id = id;
    g_devs.back().ord = dup ? 0 : id;
    int rc = init_device(g_devs.back());
    if (rc == PV_OK && g_kc.count()) {   // a device added after keys were cached gets them too
      rc = kc_prepare(g_devs.back(), g_kc.keys.data(), 0, g_kc.count());
      if (rc == PV_OK) g_devs.back().kc_count = g_kc.count();
    }
    if (rc != PV_OK) {
      release_device(g_devs.back());
      g_devs.pop_back();
      return rc;
    }
  }
  if (g_devs.empty()) return fail(PV_ENODEV, "device_mask 0x%x selects no visible device", device_mask);
  return PV_OK;
}

int pv_init(uint32_t device_mask) {
  std::lock_guard<std::mutex> lk(g_mu);
  return init_devices(device_mask, g_dup);
}

int pv_test_init_dup(uint32_t k) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (k < 2 || k > 8) return fail(PV_EINVAL, "pv_test_init_dup: k must be in 2..8 (got %u)", k);
  if (!g_devs.empty()) return fail(PV_EINVAL, "pv_test_init_dup: devices already initialised (call pv_shutdown first)");
  g_dup = (int)k;
  const int rc = init_devices(0, g_dup);
  if (rc != PV_OK) g_dup = 0;
  return rc;
}

int pv_test_set_spin_ns(int64_t ns) {
  if (ns < 0) return fail(PV_EINVAL, "pv_test_set_spin_ns: ns must be >= 0 (got %lld)", (long long)ns);
  g_zc_spin_ns.store(ns, std::memory_order_relaxed);
  return PV_OK;
}

void pv_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceGuard dg;
  release_trees();
  release_stores();
  for (auto& d : g_devs) release_device(d);
  g_devs.clear();
  g_kc.clear();
  g_dup = 0;
}

int pv_keycache_add(const uint8_t* pk, uint64_t k) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (k == 0) return PV_OK;
  if (!pk) return fail(PV_EINVAL, "null buffer");
  if (g_kc.count() + k > 0xfffffffeull) return fail(PV_EINVAL, "key cache limited to 2^32 - 2 keys");
  // keys not cached yet, first occurrence only
  std::vector<uint8_t> add;
  {
    KeyIndex seen;
    seen.reset(pk, k);
    for (uint64_t i = 0; i < k; ++i) {
      const size_t before = seen.first.size();
      (void)seen.insert(i);
      if (seen.first.size() != before && g_kc.find(pk + 32 * i) == UINT32_MAX)
        add.insert(add.end(), pk + 32 * i, pk + 32 * i + 32);
    }
  }
  if (add.empty()) return PV_OK;
  const uint64_t first = g_kc.count(), cnt = add.size() / 32;
  for (auto& d : g_devs) {
    const int rc = kc_prepare(d, add.data(), first, cnt);
    if (rc) return rc;   // committed nowhere: every device keeps its previous slots
  }
  g_kc.commit(add);
  for (auto& d : g_devs) d.kc_count = g_kc.count();
  return PV_OK;
}

int pv_keycache_clear(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceGuard dg;
  g_kc.clear();
  for (auto& d : g_devs) {
    (void)hipSetDevice(d.ord);
    (void)hipStreamSynchronize(d.stream);
    d.kc.release();
    d.kc_count = 0;
  }
  return PV_OK;
}

int pv_keycache_size(uint64_t* count) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!count) return fail(PV_EINVAL, "null buffer");
  *count = g_kc.count();
  return PV_OK;
}

const char* pv_last_error(void) { return g_err.c_str(); }

int pv_device_count(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceGuard dg;
  return (int)g_devs.size();
}

int pv_verify_batch(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off,
                    uint64_t n, uint8_t* verdict, uint32_t device_mask, uint32_t flags) {
  if (flags & ~PV_FLAG_DEDUP_KEYS) return fail(PV_EINVAL, "unknown flags 0x%x", flags);
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!pk || !sig || !msg_off || !verdict || (!msg_blob && msg_off[n] != msg_off[0]))
    return fail(PV_EINVAL, "null buffer");
  if (msg_off[n] < msg_off[0]) return fail(PV_EINVAL, "msg_off not monotone");
  std::vector<Device*> devs = select_devs(device_mask);
  if (devs.empty()) return fail(PV_ENODEV, "device_mask 0x%x selects no initialised device", device_mask);
  const HostBatch hb{pk, sig, msg_blob, msg_off, verdict, flags};
  const uint64_t G = devs.size();
  if (G == 1) return run_shard(*devs[0], hb, 0, n);
  // O(G) pre-check of the shard boundaries (each shard also checks its own
  // range first, and every chunk its offsets while they are copied)
  for (uint64_t g = 0; g < G; ++g)
    if (msg_off[n * (g + 1) / G] < msg_off[n * g / G])
      return fail(PV_EINVAL, "msg_off not monotone in shard %llu [%llu, %llu]", (unsigned long long)g,
                  (unsigned long long)(n * g / G), (unsigned long long)(n * (g + 1) / G));
  // one worker thread per device: each gathers, stages and launches its own
  // shard, so no device waits on another's host gathers (errors come back as
  // codes + messages; no exception crosses the ABI)
  std::vector<int> rc(G, PV_OK);
  std::vector<std::string> err(G);
  std::vector<std::thread> ts;
  auto work = [&](uint64_t g) {
    rc[g] = run_shard(*devs[g], hb, n * g / G, n * (g + 1) / G);
    if (rc[g]) err[g] = g_err;
  };
  std::vector<uint64_t> inline_g;
  try {
    ts.reserve(G);
  } catch (...) {
  }
  for (uint64_t g = 1; g < G; ++g) {
    try {
      ts.emplace_back(work, g);
    } catch (...) {
      inline_g.push_back(g);
    }
  }
  work(0);
  for (uint64_t g : inline_g) work(g);
  for (auto& t : ts) t.join();
  for (uint64_t g = 0; g < G; ++g)
    if (rc[g]) return fail(rc[g], "device %d: %s", devs[g]->id, err[g].c_str());
  return PV_OK;
}

int pv_verify_batch_device(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off,
                           uint64_t n, uint8_t* verdict, uint64_t* bitmap, int device, void* stream) {
  return verify_device(false, false, false, nullptr, nullptr, pk, sig, msg_blob, msg_off, n, verdict, bitmap, device,
                       stream, 0);
}

int pv_verify_batch_device_async(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg_blob,
                                 const uint64_t* msg_off, uint64_t n, uint8_t* verdict, uint64_t* bitmap, int device,
                                 void* stream, int slot) {
  return verify_device(false, false, true, nullptr, nullptr, pk, sig, msg_blob, msg_off, n, verdict, bitmap, device,
                       stream, slot);
}

int pv_verify_keyed_device(const uint32_t* ktab, const uint32_t* key_idx, const uint8_t* pk, const uint8_t* sig,
                           const uint8_t* msg_blob, const uint64_t* msg_off, uint64_t n, uint8_t* verdict,
                           uint64_t* bitmap, int device, void* stream) {
  return verify_device(true, false, false, ktab, key_idx, pk, sig, msg_blob, msg_off, n, verdict, bitmap, device,
                       stream, 0);
}

int pv_verify_keyed_device_async(const uint32_t* ktab, const uint32_t* key_idx, const uint8_t* pk, const uint8_t* sig,
                                 const uint8_t* msg_blob, const uint64_t* msg_off, uint64_t n, uint8_t* verdict,
                                 uint64_t* bitmap, int device, void* stream, int slot) {
  return verify_device(true, false, true, ktab, key_idx, pk, sig, msg_blob, msg_off, n, verdict, bitmap, device,
                       stream, slot);
}

int pv_verify_keyed_wide_device(const uint32_t* ktab, const uint32_t* key_idx, const uint8_t* pk, const uint8_t* sig,
                                const uint8_t* msg_blob, const uint64_t* msg_off, uint64_t n, uint8_t* verdict,
                                uint64_t* bitmap, int device, void* stream) {
  return verify_device(true, true, false, ktab, key_idx, pk, sig, msg_blob, msg_off, n, verdict, bitmap, device,
                       stream, 0);
}

int pv_verify_keyed_wide_device_async(const uint32_t* ktab, const uint32_t* key_idx, const uint8_t* pk,
                                      const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off, uint64_t n,
                                      uint8_t* verdict, uint64_t* bitmap, int device, void* stream, int slot) {
  return verify_device(true, true, true, ktab, key_idx, pk, sig, msg_blob, msg_off, n, verdict, bitmap, device, stream,
                       slot);
}

int pv_keys_prepare_device(const uint8_t* pk, uint64_t k, uint32_t* ktab, int device, void* stream) {
  return keys_prepare_device(false, false, pk, k, ktab, device, stream, 0);
}

int pv_keys_prepare_device_async(const uint8_t* pk, uint64_t k, uint32_t* ktab, int device, void* stream, int slot) {
  return keys_prepare_device(false, true, pk, k, ktab, device, stream, slot);
}

int pv_keys_prepare_wide_device(const uint8_t* pk, uint64_t k, uint32_t* ktab, int device, void* stream) {
  return keys_prepare_device(true, false, pk, k, ktab, device, stream, 0);
}

int pv_keys_prepare_wide_device_async(const uint8_t* pk, uint64_t k, uint32_t* ktab, int device, void* stream,
                                      int slot) {
  return keys_prepare_device(true, true, pk, k, ktab, device, stream, slot);
}

// key preparation beside the hash stage: the keys are built on the slot's side
// stream while k_hash runs on `s`; the keyed curve waits for both
int pv_verify_keys_device_async(const uint8_t* pk, uint64_t k, uint32_t* ktab, const uint32_t* key_idx,
                                const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off, uint64_t n,
                                uint8_t* verdict, uint64_t* bitmap, uint32_t wide, int device, void* stream, int slot) {
  Entry en(device, slot);
  if (const int rc = en.check()) return rc;
  if (wide > 1) return fail(PV_EINVAL, "wide must be 0 or 1");
  if (k == 0 && n == 0) return PV_OK;
  if (n > 0 && k == 0) return fail(PV_EINVAL, "signatures without keys");
  if (!pk || !ktab || (n > 0 && (!key_idx || !sig || !msg_blob || !msg_off || !verdict || !bitmap)))
    return fail(PV_EINVAL, "null device buffer");
  if (const int rc = en.begin(stream)) return rc;
  Device* d = en.d;
  hipStream_t s = en.s;
  Workspace& w = d->ws[slot];
  // the slot's key table and key scratch were last used by its previous batch:
  // fork after that (the use orders s), join before the curve
  WsUse use(w, s);
  if (use.rc) return use.rc;
  // beside the hash stage only when the key grid is small (less than one wave
  // per SIMD: C3's 25 wide node keys, a latency-bound 50-wave grid): a key
  // grid that fills the GPU (C4's 2^20 keys) competes with k_hash for the
  // same issue slots and ran 1.3 % slower beside it
  // (profiles/r06_ab_keys_beside.jsonl), so it stays in line on `s`
  const uint64_t lanes = wide ? k * (uint64_t)pv::KEYTAB_WIDE_LANES : k;
  const bool side = lanes <= 64ull * 4 * (uint64_t)d->cu_count;
  hipStream_t ks = side ? d->kside[slot] : s;
  if (side) {
    HIP_OK(hipEventRecord(d->kfork[slot], s));
    // from here an early return joins the side stream back before the
    // workspace counts as released (its work writes the key scratch and ktab)
    use.fork(ks, d->kjoin[slot]);
    HIP_OK(hipStreamWaitEvent(ks, d->kfork[slot], 0));
  }
  if (const int rc = keys_launch(*d, pk, k, ktab, wide != 0, ks, slot)) return rc;
  if (side) HIP_OK(hipEventRecord(d->kjoin[slot], ks));
  if (n == 0) {
    if (side) HIP_OK(hipStreamWaitEvent(s, d->kjoin[slot], 0));
    return use.end();
  }
  const int rc = enqueue_verify(*d, w, pk, sig, msg_blob, msg_off, n, verdict, bitmap, s, false, nullptr, nullptr, ktab,
                                key_idx, wide != 0, side ? d->kjoin[slot] : nullptr);
  if (rc == PV_OK) use.open = false;   // enqueue_verify joined and recorded the workspace's last use
  return rc;
}

int pv_time_verify_keyed_device(const uint32_t* ktab, const uint32_t* key_idx, const uint8_t* pk, const uint8_t* sig,
                                const uint8_t* msg_blob, const uint64_t* msg_off, uint64_t n, uint8_t* verdict,
                                uint64_t* bitmap, int device, void* stream, int iters, float* ms_hash,
                                float* ms_curve) {
  return time_verify(ktab, key_idx, pk, sig, msg_blob, msg_off, n, verdict, bitmap, device, stream, iters, ms_hash,
                     ms_curve);
}

int pv_time_verify_device(const uint8_t* pk, const uint8_t* sig, const uint8_t* msg_blob, const uint64_t* msg_off,
                          uint64_t n, uint8_t* verdict, uint64_t* bitmap, int device, void* stream, int iters,
                          float* ms_hash, float* ms_curve) {
  return time_verify(nullptr, nullptr, pk, sig, msg_blob, msg_off, n, verdict, bitmap, device, stream, iters, ms_hash,
                     ms_curve);
}

// (these two look the device up before the guard exists: their own lines)
int pv_kernel_timing(int device, int enable, float* hash_ms, float* curve_ms, uint64_t* launches) {
  std::lock_guard<std::mutex> lk(g_mu);
  Device* d = find_dev(device);
  if (!d) return fail(PV_ENOTINIT, "device %d not initialised (call pv_init)", device);
  DeviceGuard dg;
  HIP_OK(hipSetDevice(d->ord));
  {
    const int rc = resolve_live(*d);
    if (rc) return rc;
  }
  if (enable) {
    d->live_hash = d->live_curve = d->live_sha = 0;
    d->live_launches = 0;
  }
  if (hash_ms) *hash_ms = d->live_hash;
  if (curve_ms) *curve_ms = d->live_curve;
  if (launches) *launches = d->live_launches;
  d->live_timing = enable != 0;
  return PV_OK;
}

int pv_kernel_timing_sha(int device, float* sha_ms) {
  std::lock_guard<std::mutex> lk(g_mu);
  Device* d = find_dev(device);
  if (!d) return fail(PV_ENOTINIT, "device %d not initialised (call pv_init)", device);
  DeviceGuard dg;
  HIP_OK(hipSetDevice(d->ord));
  const int rc = resolve_live(*d);
  if (rc) return rc;
  if (sha_ms) *sha_ms = d->live_sha;
  return PV_OK;
}

int pv_get_tuning(pv_tuning* t) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!t) return fail(PV_EINVAL, "null pointer");
  if (t->struct_size != sizeof(pv_tuning))
    return fail(PV_EINVAL, "struct_size %u != sizeof(pv_tuning) %zu", t->struct_size, sizeof(pv_tuning));
  *t = g_tune;
  return PV_OK;
}

int pv_set_tuning(const pv_tuning* t) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!t) return fail(PV_EINVAL, "null pointer");
  if (int rc = check_tuning(*t)) return rc;
  g_tune = *t;
  pvbls::set_quad_max(g_tune.bls_quad_max);
  pvbls::set_oct_max(g_tune.bls_oct_max);
  DeviceGuard dg;
  for (auto& d : g_devs) apply_tuning(d, g_tune);
  return PV_OK;
}

int pv_curve_stats(int device, uint32_t* mode, uint64_t* deferred) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  Device* d = en.d;
  if (mode) *mode = d->mode == CurveMode::Half ? PV_CURVE_HALF : d->mode == CurveMode::Full ? PV_CURVE_FULL
                                                                                             : PV_CURVE_GROUPED;
  if (deferred) {
    *deferred = 0;
    Workspace& w = d->ws[d->last_ws];
    if (w.half_ran) {
      HIP_OK(hipSetDevice(d->ord));
      HIP_OK(w.done_on ? hipEventSynchronize(w.done) : hipStreamSynchronize(w.stream));
      HIP_OK(hipMemcpy(deferred, w.qc.p, sizeof(uint64_t), hipMemcpyDeviceToHost));
    }
  }
  return PV_OK;
}

int pv_tally_votes_device(const uint8_t* verdict, const uint32_t* sender, const uint64_t* batch_off,
                          uint64_t n_batches, uint32_t n_nodes, uint32_t quorum, uint32_t* votes, uint8_t* reached,
                          int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n_nodes == 0 || n_nodes > 1024) return fail(PV_EINVAL, "n_nodes must be in 1..1024");
  if (n_batches == 0) return PV_OK;
  if (!verdict || !sender || !batch_off || !votes || !reached) return fail(PV_EINVAL, "null device buffer");
  if (const int rc = en.begin(stream)) return rc;
  Device* d = en.d;
  hipStream_t s = en.s;
  HIP_OK(d->tflag.ensure(1));
  HIP_OK(hipMemsetAsync(d->tflag.p, 0, 4, s));
  HIP_OK(pv::launch_tally(verdict, sender, batch_off, n_batches, n_nodes, quorum, votes, reached, d->tflag.p, s));
  uint32_t bad = 0;
  HIP_OK(hipMemcpyAsync(&bad, d->tflag.p, 4, hipMemcpyDeviceToHost, s));
  if (const int rc = en.finish()) return rc;
  if (bad) return fail(PV_EINVAL, "a sender index is >= n_nodes (%u)", n_nodes);
  return PV_OK;
}

int pv_tally_votes_device_async(const uint8_t* verdict, const uint32_t* sender, const uint64_t* batch_off,
                                uint64_t n_batches, uint32_t n_nodes, uint32_t quorum, uint32_t* votes,
                                uint8_t* reached, uint32_t* bad, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n_nodes == 0 || n_nodes > 1024) return fail(PV_EINVAL, "n_nodes must be in 1..1024");
  if (!bad) return fail(PV_EINVAL, "null device buffer");
  if (n_batches == 0) return PV_OK;
  if (!verdict || !sender || !batch_off || !votes || !reached) return fail(PV_EINVAL, "null device buffer");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_tally(verdict, sender, batch_off, n_batches, n_nodes, quorum, votes, reached, bad, en.s));
  return PV_OK;
}

int pv_tally_votes(const uint8_t* verdict, const uint32_t* sender, const uint64_t* batch_off, uint64_t n_batches,
                   uint32_t n_nodes, uint32_t quorum, uint32_t* votes, uint8_t* reached) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n_nodes == 0 || n_nodes > 1024) return fail(PV_EINVAL, "n_nodes must be in 1..1024");
  if (n_batches == 0) return PV_OK;
  if (!verdict || !sender || !batch_off || !votes || !reached) return fail(PV_EINVAL, "null buffer");
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  // (its own rebase: the refusal has no position, unlike offsets_ok's)
  const uint64_t b0 = batch_off[0], m = batch_off[n_batches] - b0;
  std::vector<uint64_t> offs(n_batches + 1);
  for (uint64_t k = 0; k <= n_batches; ++k) {
    if (k && batch_off[k] < batch_off[k - 1]) return fail(PV_EINVAL, "batch_off not monotone");
    offs[k] = batch_off[k] - b0;
  }
  for (uint64_t k = 0; k < m; ++k)
    if (sender[b0 + k] >= n_nodes)
      return fail(PV_EINVAL, "sender[%llu] = %u is >= n_nodes (%u)", (unsigned long long)(b0 + k), sender[b0 + k],
                  n_nodes);
  HIP_OK(d.verdict.ensure(m ? m : 1));
  HIP_OK(d.sender.ensure(m ? m : 1));
  HIP_OK(d.batch_off.ensure(n_batches + 1));
  HIP_OK(d.votes.ensure(n_batches));
  HIP_OK(d.reached.ensure(n_batches));
  HIP_OK(d.tflag.ensure(1));
  if (m) {
    HIP_OK(hipMemcpyAsync(d.verdict.p, verdict + b0, m, hipMemcpyHostToDevice, d.stream));
    HIP_OK(hipMemcpyAsync(d.sender.p, sender + b0, m * 4, hipMemcpyHostToDevice, d.stream));
  }
  HIP_OK(hipMemcpyAsync(d.batch_off.p, offs.data(), (n_batches + 1) * 8, hipMemcpyHostToDevice, d.stream));
  HIP_OK(pv::launch_tally(d.verdict.p, d.sender.p, d.batch_off.p, n_batches, n_nodes, quorum, d.votes.p, d.reached.p,
                          d.tflag.p, d.stream));
  HIP_OK(hipMemcpyAsync(votes, d.votes.p, n_batches * 4, hipMemcpyDeviceToHost, d.stream));
  HIP_OK(hipMemcpyAsync(reached, d.reached.p, n_batches, hipMemcpyDeviceToHost, d.stream));
  return en.finish();
}

int pv_tally_device(const uint32_t* verdict_bits, const uint32_t* dup_mask, uint64_t n_batches, uint32_t n_nodes,
                    uint32_t quorum, uint8_t* reached, uint32_t* votes, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n_nodes == 0) return fail(PV_EINVAL, "n_nodes must be >= 1");
  if (n_batches == 0) return PV_OK;
  if (!verdict_bits || !reached) return fail(PV_EINVAL, "null device buffer");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_tally_bits(verdict_bits, dup_mask, n_batches, n_nodes, quorum, votes, reached, en.s));
  return en.finish();
}

int pv_tally(const uint32_t* verdict_bits, const uint32_t* dup_mask, uint64_t n_batches, uint32_t n_nodes,
             uint32_t quorum, uint8_t* reached) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n_nodes == 0) return fail(PV_EINVAL, "n_nodes must be >= 1");
  if (n_batches == 0) return PV_OK;
  if (!verdict_bits || !reached) return fail(PV_EINVAL, "null buffer");
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  const uint64_t words = n_batches * ((n_nodes + 31) / 32);
  HIP_OK(d.tbits.ensure(2 * words));
  HIP_OK(d.reached.ensure(n_batches));
  HIP_OK(hipMemcpyAsync(d.tbits.p, verdict_bits, words * 4, hipMemcpyHostToDevice, d.stream));
  if (dup_mask) HIP_OK(hipMemcpyAsync(d.tbits.p + words, dup_mask, words * 4, hipMemcpyHostToDevice, d.stream));
  HIP_OK(pv::launch_tally_bits(d.tbits.p, dup_mask ? d.tbits.p + words : nullptr, n_batches, n_nodes, quorum, nullptr,
                               d.reached.p, d.stream));
  HIP_OK(hipMemcpyAsync(reached, d.reached.p, n_batches, hipMemcpyDeviceToHost, d.stream));
  return en.finish();
}

int pv_sign_batch_device(const uint8_t* seeds, const uint8_t* msg_blob, const uint64_t* msg_off, uint64_t n,
                         uint8_t* pk_out, uint8_t* sig_out, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_sign(seeds, msg_blob, msg_off, n, en.d->btab.p, pk_out, sig_out, en.s));
  return en.finish();
}

int pv_sign_batch(const uint8_t* seeds, const uint8_t* msg_blob, const uint64_t* msg_off, uint64_t n,
                  uint8_t* pk_out, uint8_t* sig_out) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!seeds || !msg_off || !pk_out || !sig_out) return fail(PV_EINVAL, "null buffer");
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  Ragged msgs(msg_off, n);   // (this form does not refuse decreasing offsets)
  HIP_OK(d.tamper.ensure(n * 32));  // seeds staging
  HIP_OK(d.pk.ensure(n * 32));
  HIP_OK(d.sig.ensure(n * 64));
  HIP_OK(hipMemcpyAsync(d.tamper.p, seeds, n * 32, hipMemcpyHostToDevice, d.stream));
  if (const int rc = msgs.stage(msg_blob, d, d.stream)) return rc;
  HIP_OK(pv::launch_sign(d.tamper.p, d.blob.p, d.off.p, n, d.btab.p, d.pk.p, d.sig.p, d.stream));
  HIP_OK(hipMemcpyAsync(pk_out, d.pk.p, n * 32, hipMemcpyDeviceToHost, d.stream));
  HIP_OK(hipMemcpyAsync(sig_out, d.sig.p, n * 64, hipMemcpyDeviceToHost, d.stream));
  return en.finish();
}

}  // extern "C"

namespace {
// leaf digests (n x 8 words) -> root (8 words) on stream s, all device memory
// root of the empty tree: hash_empty(), SHA-256 of the empty string (ledger/tree_hasher.py:17-19)
const uint32_t EMPTY_ROOT[8] = {0x42c4b0e3u, 0x141cfc98u, 0xc8f4fb9au, 0x24b96f99u,
                                0xe441ae27u, 0x4c939b64u, 0x1b9995a4u, 0x55b85278u};
int enqueue_merkle(Device& d, const uint8_t* blob, const uint64_t* off, uint64_t n, uint32_t* leaves, uint32_t* root,
                   hipStream_t s) {
  if (n == 0) {
    HIP_OK(hipMemcpyAsync(root, EMPTY_ROOT, 32, hipMemcpyHostToDevice, s));
    return PV_OK;
  }
  HIP_OK(pv::launch_sha256(blob, off, n, 1, 0x00, d.counter.p, leaves, d.sha256_blocks, s));
  const uint32_t* in = leaves;
  uint64_t m = n;
  int which = 0;
  while (m > 1) {
    if (m <= (uint64_t)pv::MERKLE_TAIL) {   // the last levels: one launch
      HIP_OK(pv::launch_merkle_tail(in, m, root, s));
      break;
    }
    uint32_t* out = (m + 1) / 2 == 1 ? root : (which ? d.mk1.p : d.mk0.p);
    HIP_OK(pv::launch_merkle_level(in, m, out, s));
    in = out;
    m = (m + 1) / 2;
    which ^= 1;
  }
  if (n == 1) HIP_OK(hipMemcpyAsync(root, leaves, 32, hipMemcpyDeviceToDevice, s));
  return PV_OK;
}
}  // namespace

extern "C" {

int pv_sha256_batch_device(const uint8_t* blob, const uint64_t* off, uint64_t n, int32_t prefix, uint8_t* digests,
                           int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!blob || !off || !digests) return fail(PV_EINVAL, "null device buffer");
  if (prefix > 255) return fail(PV_EINVAL, "prefix must be -1 (none) or a byte value");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_sha256(blob, off, n, prefix < 0 ? 0 : 1, prefix < 0 ? 0 : (uint32_t)prefix, en.d->counter.p,
                           reinterpret_cast<uint32_t*>(digests), en.d->sha256_blocks, en.s));
  return en.finish();
}

int pv_merkle_root_device(const uint8_t* blob, const uint64_t* off, uint64_t n, uint8_t* leaf_hashes, uint8_t* root,
                          int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (!root || (n && (!blob || !off))) return fail(PV_EINVAL, "null device buffer");
  if (const int rc = en.begin(stream)) return rc;
  Device* d = en.d;
  uint32_t* leaves = reinterpret_cast<uint32_t*>(leaf_hashes);
  if (!leaves && n) {
    HIP_OK(d->mk1.ensure((n + 1) / 2 * 8 + n * 8));
    leaves = d->mk1.p + (n + 1) / 2 * 8;
  }
  HIP_OK(d->mk0.ensure((n + 1) / 2 * 8 + 8));
  if (leaf_hashes) HIP_OK(d->mk1.ensure((n + 1) / 2 * 8 + 8));
  return en.finish(enqueue_merkle(*d, blob, off, n, leaves, reinterpret_cast<uint32_t*>(root), en.s));
}

int pv_merkle_root(const uint8_t* blob, const uint64_t* off, uint64_t n, uint8_t* root, uint8_t* leaf_hashes) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (!root || (n && (!off || (!blob && off[n] != off[0])))) return fail(PV_EINVAL, "null buffer");
  Ragged leaf(off, n);
  if (const int rc = leaf.check("off")) return rc;
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  HIP_OK(d.mk0.ensure((n + 1) / 2 * 8 + 8));
  HIP_OK(d.mk1.ensure((n + 1) / 2 * 8 + n * 8 + 8));
  uint32_t* leaves = d.mk1.p + (n + 1) / 2 * 8;
  uint32_t* droot = d.mk0.p + (n + 1) / 2 * 8;
  if (const int rc = leaf.stage(blob, d, d.stream)) return rc;
  if (const int rc = enqueue_merkle(d, d.blob.p, d.off.p, n, leaves, droot, d.stream)) return rc;
  HIP_OK(hipMemcpyAsync(root, droot, 32, hipMemcpyDeviceToHost, d.stream));
  if (leaf_hashes && n) HIP_OK(hipMemcpyAsync(leaf_hashes, leaves, n * 32, hipMemcpyDeviceToHost, d.stream));
  return en.finish();
}

int pv_sha256_batch(const uint8_t* blob, const uint64_t* off, uint64_t n, int32_t prefix, uint8_t* digests) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!off || !digests || (!blob && off[n] != off[0])) return fail(PV_EINVAL, "null buffer");
  if (prefix > 255) return fail(PV_EINVAL, "prefix must be -1 (none) or a byte value");
  Ragged msgs(off, n);
  if (const int rc = msgs.check("off")) return rc;
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  HIP_OK(d.mk0.ensure(n * 8));
  if (const int rc = msgs.stage(blob, d, d.stream)) return rc;
  HIP_OK(pv::launch_sha256(d.blob.p, d.off.p, n, prefix < 0 ? 0 : 1, prefix < 0 ? 0 : (uint32_t)prefix, d.counter.p,
                           d.mk0.p, d.sha256_blocks, d.stream));
  HIP_OK(hipMemcpyAsync(digests, d.mk0.p, n * 32, hipMemcpyDeviceToHost, d.stream));
  return en.finish();
}

}  // extern "C"

// ------------------------------------------ Merkle audit paths / consistency
namespace {

int merkle_blocks(const Device& d) { return d.cu_count * 32; }

// A resident tree: one device buffer per level (level 0 = leaf hashes, an odd
// last node moves up), capacities geometric, plus the device table of level
// pointers the generation kernels read.
constexpr uint32_t MT_LEVELS = 65;
struct MerkleTree {
  bool live = false;
  int dev = -1;           // Device::id
  uint64_t n = 0;         // leaves
  uint64_t committed = 0; // leaves [committed, n) are staged (pv_merkle_tree_stage*)
  uint32_t depth = 0;     // levels above the leaves
  uint64_t hint = 1;
  std::vector<uint32_t*> lv;
  std::vector<uint64_t> cap;   // nodes
  const uint32_t** table = nullptr;   // device: MT_LEVELS level pointers
  std::vector<const uint32_t*> host_table;
  bool dirty = true;
};
std::vector<MerkleTree> g_trees;   // handle = index + 1

void tree_release(MerkleTree& t) {
  if (!t.live) return;
  if (Device* d = find_dev(t.dev)) {
    (void)hipSetDevice(d->ord);
    (void)hipStreamSynchronize(d->stream);
  }
  for (uint32_t* p : t.lv)
    if (p) (void)hipFree(p);
  if (t.table) (void)hipFree(t.table);
  t = MerkleTree();
}

void release_trees() {
  for (auto& t : g_trees) tree_release(t);
  g_trees.clear();
}

MerkleTree* find_tree(int32_t handle) {
  if (handle < 1 || (size_t)handle > g_trees.size() || !g_trees[handle - 1].live) return nullptr;
  return &g_trees[handle - 1];
}

uint64_t level_count(uint64_t n, uint32_t l) { return n == 0 ? 0 : ((n - 1) >> l) + 1; }

// level l holds at least `need` nodes afterwards; on overflow the capacity
// doubles and the nodes in use are copied device-to-device on s
int tree_grow(MerkleTree& t, uint32_t l, uint64_t need, hipStream_t s) {
  if (l >= MT_LEVELS) return fail(PV_EINVAL, "Merkle tree deeper than %u levels", MT_LEVELS - 1);
  if (l >= t.lv.size()) {
    t.lv.resize(l + 1, nullptr);
    t.cap.resize(l + 1, 0);
  }
  if (need <= t.cap[l]) return PV_OK;
  uint64_t nc = t.cap[l];
  if (nc == 0) {
    nc = l < 64 ? ((t.hint - 1) >> l) + 1 : 1;
  }
  while (nc < need) nc *= 2;
  uint32_t* np = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&np), nc * 32));
  uint64_t used = l <= t.depth ? level_count(t.n, l) : 0;
  if (used > t.cap[l]) used = t.cap[l];
  if (t.lv[l]) {
    hipError_t e = hipSuccess;
    if (used) e = hipMemcpyAsync(np, t.lv[l], used * 32, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      (void)hipFree(np);
      HIP_OK(e);
    }
    (void)hipFree(t.lv[l]);
  }
  t.lv[l] = np;
  t.cap[l] = nc;
  t.dirty = true;
  return PV_OK;
}

// leaves n .. n + k - 1 are in level 0: rebuild the parents they change.  At
// level l + 1 the first changed parent is n_old >> (l + 1) (the old promoted
// right-edge node is recomputed); levels are added as the tree deepens.
int tree_rebuild(MerkleTree& t, uint64_t n_new, hipStream_t s) {
  const uint64_t n_old = t.n;
  uint64_t m = n_new;
  uint32_t l = 0;
  while (m > 1) {
    const uint64_t outs = (m + 1) / 2;
    int rc = tree_grow(t, l + 1, outs, s);
    if (rc) return rc;
    HIP_OK(pv::launch_merkle_level_keep(t.lv[l], l + 1 < 64 ? n_old >> (l + 1) : 0, m, t.lv[l + 1], s));
    m = outs;
    ++l;
  }
  t.depth = l;
  t.n = n_new;
  if (t.dirty) {
    if (!t.table) HIP_OK(hipMalloc(reinterpret_cast<void**>(&t.table), MT_LEVELS * sizeof(uint32_t*)));
    t.host_table.assign(MT_LEVELS, nullptr);
    for (size_t i = 0; i < t.lv.size(); ++i) t.host_table[i] = t.lv[i];
    HIP_OK(hipMemcpyAsync(t.table, t.host_table.data(), MT_LEVELS * sizeof(uint32_t*), hipMemcpyHostToDevice, s));
    t.dirty = false;
  }
  return PV_OK;
}

// extend* appends and commits: refused while leaves are staged
int tree_unstaged(const MerkleTree& t) {
  if (t.committed == t.n) return PV_OK;
  return fail(PV_EINVAL, "the tree holds %llu staged leaves: commit or discard them before extend",
              (unsigned long long)(t.n - t.committed));
}

// the tree has n_new leaves and the leaves from f0 on are new (stage: f0 = the old size) or lost
// their right neighbours (discard: f0 = n_new - 1): one k_merkle_edge launch rebuilds their ancestors
int tree_edge(MerkleTree& t, uint64_t f0, uint64_t n_new, hipStream_t s) {
  uint32_t depth = 0;
  for (uint64_t m = n_new; m > 1; m = (m + 1) / 2) {
    ++depth;
    if (const int rc = tree_grow(t, depth, (m + 1) / 2, s)) return rc;
  }
  if (n_new > 1) HIP_OK(pv::launch_merkle_edge(t.lv.data(), depth + 1, f0, n_new, s));
  t.depth = depth;
  t.n = n_new;
  if (t.dirty) {   // a level moved: the table the read kernels use, as tree_rebuild uploads it
    t.host_table.assign(MT_LEVELS, nullptr);
    for (size_t i = 0; i < t.lv.size(); ++i) t.host_table[i] = t.lv[i];
    HIP_OK(hipMemcpyAsync(t.table, t.host_table.data(), MT_LEVELS * sizeof(uint32_t*), hipMemcpyHostToDevice, s));
    t.dirty = false;
  }
  return PV_OK;
}

// root (HOST, may be null) <- MTH(0, n) once the work queued on s is done
int tree_root(const MerkleTree& t, uint8_t* root, hipStream_t s) {
  if (!root) return PV_OK;
  if (t.n == 0) {
    memcpy(root, EMPTY_ROOT, 32);
    return PV_OK;
  }
  HIP_OK(hipMemcpyAsync(root, t.lv[t.depth], 32, hipMemcpyDeviceToHost, s));
  return PV_OK;
}

// k staged leaf hashes are in level 0 behind the n the tree has: their ancestors.  Up to
// MERKLE_EDGE_MAX leaves in one launch, more by the per-level rebuild of extend.
int tree_stage(MerkleTree& t, uint64_t k, uint8_t* root_out, hipStream_t s) {
  const int rc = k <= pv::MERKLE_EDGE_MAX ? tree_edge(t, t.n, t.n + k, s) : tree_rebuild(t, t.n + k, s);
  if (rc) return rc;
  return tree_root(t, root_out, s);
}

// resolve a handle to its tree and point the (host-form) entry scope at the
// tree's device; en.begin() then makes it current
int tree_enter(Entry& en, int32_t handle, MerkleTree** t) {
  if (const int rc = en.check()) return rc;
  *t = find_tree(handle);
  if (!*t) return fail(PV_EINVAL, "no Merkle tree with handle %d", (int)handle);
  en.d = find_dev((*t)->dev);
  if (!en.d) return fail(PV_EINVAL, "the device of Merkle tree %d is gone", (int)handle);
  return PV_OK;
}

// all device memory; leaf = leaf hashes, or NULL: hash blob / off into d.mk0 first
int enqueue_verify_incl(Device& d, const uint32_t* leaf, const uint8_t* blob, const uint64_t* off,
                        const uint64_t* index, const uint64_t* tree_size, const uint32_t* nodes,
                        const uint64_t* proof_off, const uint32_t* roots, const uint32_t* root_idx, uint64_t n,
                        uint8_t* status, uint32_t* computed, uint64_t* stop_index, hipStream_t s) {
  if (!leaf) {   // leaf mode: the existing leaf hasher, then the walk
    HIP_OK(d.mk0.ensure(n * 8));
    HIP_OK(pv::launch_sha256(blob, off, n, 1, 0x00, d.counter.p, d.mk0.p, d.sha256_blocks, s));
    leaf = d.mk0.p;
  }
  HIP_OK(pv::launch_merkle_verify_incl(leaf, index, tree_size, nodes, proof_off, roots, root_idx, n, status, computed,
                                       stop_index, merkle_blocks(d), s));
  return PV_OK;
}

}  // namespace

extern "C" {

int pv_merkle_verify_inclusion_device(const uint8_t* leaf_hashes, const uint8_t* leaf_blob, const uint64_t* leaf_off,
                                      const uint64_t* index, const uint64_t* tree_size, const uint8_t* nodes,
                                      const uint64_t* proof_off, const uint8_t* roots, const uint32_t* root_idx,
                                      uint64_t n_roots, uint64_t n, uint8_t* status, uint8_t* computed,
                                      uint64_t* stop_index, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if ((!leaf_hashes && (!leaf_blob || !leaf_off)) || !index || !tree_size || !nodes || !proof_off || !roots ||
      !status || !computed || !stop_index)
    return fail(PV_EINVAL, "null device buffer");
  if (root_idx && n_roots == 0) return fail(PV_EINVAL, "root_idx without roots");
  if (misaligned16(leaf_hashes) || misaligned16(nodes) || misaligned16(roots) || misaligned16(computed))
    return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  return en.finish(enqueue_verify_incl(*en.d, w32(leaf_hashes), leaf_blob, leaf_off, index, tree_size, w32(nodes),
                                       proof_off, w32(roots), root_idx, n, status, w32(computed), stop_index, en.s));
}

int pv_merkle_verify_inclusion(const uint8_t* leaf_hashes, const uint8_t* leaf_blob, const uint64_t* leaf_off,
                               const uint64_t* index, const uint64_t* tree_size, const uint8_t* nodes,
                               const uint64_t* proof_off, const uint8_t* roots, const uint32_t* root_idx,
                               uint64_t n_roots, uint64_t n, uint8_t* status, uint8_t* computed,
                               uint64_t* stop_index) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if ((!leaf_hashes && !leaf_off) || !index || !tree_size || !proof_off || !roots || !status || !computed ||
      !stop_index)
    return fail(PV_EINVAL, "null buffer");
  Ragged proofs(proof_off, n);   // in nodes
  if (const int rc = proofs.check("proof_off")) return rc;
  if (proofs.len && !nodes) return fail(PV_EINVAL, "null buffer");
  Ragged leaf(leaf_hashes ? nullptr : leaf_off, leaf_hashes ? 0 : n);   // leaf mode only
  if (const int rc = leaf.check("leaf_off")) return rc;
  if (leaf.len && !leaf_blob) return fail(PV_EINVAL, "null buffer");
  if (root_idx)
    for (uint64_t i = 0; i < n; ++i)
      if (root_idx[i] >= n_roots)
        return fail(PV_EINVAL, "root_idx[%llu] = %u is not below n_roots %llu", (unsigned long long)i, root_idx[i],
                    (unsigned long long)n_roots);
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dleaf, dblob, dnodes, droots, dstatus, dcomp;
  TmpBuf<uint64_t> dloff, dindex, dsize, dpoff, dstop;
  TmpBuf<uint32_t> dridx;
  StreamDrain tail{s};
  if (leaf_hashes) {
    HIP_OK(dleaf.put(leaf_hashes, n * 32, s));
  } else if (const int rc = leaf.stage(leaf_blob, dblob, dloff, s)) {
    return rc;
  }
  HIP_OK(dindex.put(index, n, s));
  HIP_OK(dsize.put(tree_size, n, s));
  HIP_OK(dnodes.put(proofs.len ? nodes + proofs.b0 * 32 : nullptr, proofs.len * 32, s));
  HIP_OK(dpoff.put(proofs.rebased(), n + 1, s));
  HIP_OK(droots.put(roots, (root_idx ? n_roots : n) * 32, s));
  if (root_idx) HIP_OK(dridx.put(root_idx, n, s));
  HIP_OK(dstatus.alloc(n));
  HIP_OK(dcomp.alloc(n * 32));
  HIP_OK(dstop.alloc(n));
  if (const int rc = enqueue_verify_incl(*en.d, leaf_hashes ? w32(dleaf.p) : nullptr, dblob.p, dloff.p, dindex.p,
                                         dsize.p, w32(dnodes.p), dpoff.p, w32(droots.p), dridx.p, n, dstatus.p,
                                         w32(dcomp.p), dstop.p, s))
    return rc;
  HIP_OK(hipMemcpyAsync(status, dstatus.p, n, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(computed, dcomp.p, n * 32, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(stop_index, dstop.p, n * 8, hipMemcpyDeviceToHost, s));
  return tail.finish();
}

int pv_merkle_verify_consistency_device(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_roots,
                                        const uint8_t* new_roots, const uint32_t* old_root_idx,
                                        const uint32_t* new_root_idx, uint64_t n_roots, const uint8_t* nodes,
                                        const uint64_t* proof_off, uint64_t n, uint8_t* status, uint8_t* old_computed,
                                        uint8_t* new_computed, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!old_size || !new_size || !old_roots || !new_roots || !nodes || !proof_off || !status || !old_computed ||
      !new_computed)
    return fail(PV_EINVAL, "null device buffer");
  if ((old_root_idx == nullptr) != (new_root_idx == nullptr))
    return fail(PV_EINVAL, "old_root_idx and new_root_idx go together");
  if (old_root_idx && n_roots == 0) return fail(PV_EINVAL, "root indices without roots");
  if (misaligned16(old_roots) || misaligned16(new_roots) || misaligned16(nodes) || misaligned16(old_computed) ||
      misaligned16(new_computed))
    return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_merkle_verify_cons(old_size, new_size, w32(old_roots), w32(new_roots), old_root_idx, new_root_idx,
                                       w32(nodes), proof_off, n, status, w32(old_computed), w32(new_computed),
                                       merkle_blocks(*en.d), en.s));
  return en.finish();
}

int pv_merkle_verify_consistency(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_roots,
                                 const uint8_t* new_roots, const uint32_t* old_root_idx, const uint32_t* new_root_idx,
                                 uint64_t n_roots, const uint8_t* nodes, const uint64_t* proof_off, uint64_t n,
                                 uint8_t* status, uint8_t* old_computed, uint8_t* new_computed) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!old_size || !new_size || !old_roots || !new_roots || !proof_off || !status || !old_computed || !new_computed)
    return fail(PV_EINVAL, "null buffer");
  if ((old_root_idx == nullptr) != (new_root_idx == nullptr))
    return fail(PV_EINVAL, "old_root_idx and new_root_idx go together");
  Ragged proofs(proof_off, n);   // in nodes
  if (const int rc = proofs.check("proof_off")) return rc;
  if (proofs.len && !nodes) return fail(PV_EINVAL, "null buffer");
  if (old_root_idx)
    for (uint64_t i = 0; i < n; ++i)
      if (old_root_idx[i] >= n_roots || new_root_idx[i] >= n_roots)
        return fail(PV_EINVAL, "a root index of pair %llu is not below n_roots %llu", (unsigned long long)i,
                    (unsigned long long)n_roots);
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  const uint64_t nr = old_root_idx ? n_roots : n;
  TmpBuf<uint8_t> dnodes, dro, drn, dstatus, dco, dcn;
  TmpBuf<uint64_t> dold, dnew, dpoff;
  TmpBuf<uint32_t> dio, din;
  StreamDrain tail{s};
  HIP_OK(dold.put(old_size, n, s));
  HIP_OK(dnew.put(new_size, n, s));
  HIP_OK(dro.put(old_roots, nr * 32, s));
  HIP_OK(drn.put(new_roots, nr * 32, s));
  if (old_root_idx) {
    HIP_OK(dio.put(old_root_idx, n, s));
    HIP_OK(din.put(new_root_idx, n, s));
  }
  HIP_OK(dnodes.put(proofs.len ? nodes + proofs.b0 * 32 : nullptr, proofs.len * 32, s));
  HIP_OK(dpoff.put(proofs.rebased(), n + 1, s));
  HIP_OK(dstatus.alloc(n));
  HIP_OK(dco.alloc(n * 32));
  HIP_OK(dcn.alloc(n * 32));
  HIP_OK(pv::launch_merkle_verify_cons(dold.p, dnew.p, w32(dro.p), w32(drn.p), dio.p, din.p, w32(dnodes.p), dpoff.p, n,
                                       dstatus.p, w32(dco.p), w32(dcn.p), merkle_blocks(*en.d), s));
  HIP_OK(hipMemcpyAsync(status, dstatus.p, n, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(old_computed, dco.p, n * 32, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(new_computed, dcn.p, n * 32, hipMemcpyDeviceToHost, s));
  return tail.finish();
}

int pv_merkle_tree_create(uint64_t capacity_hint, int device, int32_t* handle) {
  Entry en(device);
  if (!handle) return fail(PV_EINVAL, "null pointer");
  if (const int rc = en.check()) return rc;
  Device* d = en.d;
  if (capacity_hint > (1ull << 40)) return fail(PV_EINVAL, "capacity_hint above 2^40 leaves");
  size_t slot = 0;
  while (slot < g_trees.size() && g_trees[slot].live) ++slot;
  if (slot == g_trees.size()) {
    if (g_trees.size() >= 0x7fffffffull) return fail(PV_ENOMEM, "too many Merkle trees");
    g_trees.emplace_back();
  }
  MerkleTree& t = g_trees[slot];
  t = MerkleTree();
  t.live = true;
  t.dev = d->id;
  t.hint = capacity_hint ? capacity_hint : 1;
  if (const int rc = en.begin()) return rc;
  int rc = tree_grow(t, 0, t.hint, d->stream);
  if (rc == PV_OK) rc = tree_rebuild(t, 0, d->stream);   // uploads the level table
  if (rc == PV_OK) {
    hipError_t e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) rc = fail(PV_EIO, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
  }
  if (rc) {
    tree_release(t);
    return rc;
  }
  *handle = (int32_t)(slot + 1);
  return PV_OK;
}

int pv_merkle_tree_free(int32_t handle) {
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceGuard dg;
  MerkleTree* t = find_tree(handle);
  if (!t) return fail(PV_EINVAL, "no Merkle tree with handle %d", (int)handle);
  tree_release(*t);
  return PV_OK;
}

// append k leaf hashes from host or device memory and rebuild the parents they change
static int tree_extend_hashes(int32_t handle, const uint8_t* leaf_hashes, uint64_t k, hipMemcpyKind kind,
                              void* stream) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (k == 0) return PV_OK;
  if (!leaf_hashes) return fail(PV_EINVAL, "null buffer");
  if (k > (1ull << 40) || t->n + k > (1ull << 40)) return fail(PV_EINVAL, "tree limited to 2^40 leaves");
  if (const int rc = tree_unstaged(*t)) return rc;
  if (const int rc = en.begin(stream)) return rc;
  if (const int rc = tree_grow(*t, 0, t->n + k, en.s)) return rc;
  HIP_OK(hipMemcpyAsync(t->lv[0] + 8 * t->n, leaf_hashes, k * 32, kind, en.s));
  if (const int rc = tree_rebuild(*t, t->n + k, en.s)) return rc;
  t->committed = t->n;
  return en.finish();
}

int pv_merkle_tree_extend_hashes_device(int32_t handle, const uint8_t* leaf_hashes, uint64_t k, void* stream) {
  return tree_extend_hashes(handle, leaf_hashes, k, hipMemcpyDeviceToDevice, stream);
}

int pv_merkle_tree_extend_hashes(int32_t handle, const uint8_t* leaf_hashes, uint64_t k) {
  return tree_extend_hashes(handle, leaf_hashes, k, hipMemcpyHostToDevice, nullptr);
}

int pv_merkle_tree_extend(int32_t handle, const uint8_t* blob, const uint64_t* off, uint64_t k) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (k == 0) return PV_OK;
  if (!off || (!blob && off[k] != off[0])) return fail(PV_EINVAL, "null buffer");
  if (k > (1ull << 40) || t->n + k > (1ull << 40)) return fail(PV_EINVAL, "tree limited to 2^40 leaves");
  Ragged leaf(off, k);
  if (const int rc = leaf.check("off")) return rc;
  if (const int rc = tree_unstaged(*t)) return rc;
  if (const int rc = en.begin()) return rc;
  Device* d = en.d;
  hipStream_t s = en.s;
  if (const int rc = leaf.stage(blob, *d, s)) return rc;
  if (const int rc = tree_grow(*t, 0, t->n + k, s)) return rc;
  HIP_OK(pv::launch_sha256(d->blob.p, d->off.p, k, 1, 0x00, d->counter.p, t->lv[0] + 8 * t->n, d->sha256_blocks, s));
  if (const int rc = tree_rebuild(*t, t->n + k, s)) return rc;
  t->committed = t->n;
  return en.finish();
}

int pv_merkle_tree_info(int32_t handle, uint64_t* n, uint32_t* depth, uint8_t* root) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (n) *n = t->n;
  if (depth) *depth = t->depth;
  if (root && t->n == 0) memcpy(root, EMPTY_ROOT, 32);
  if (!root || t->n == 0) return PV_OK;
  if (const int rc = en.begin()) return rc;
  HIP_OK(hipMemcpyAsync(root, t->lv[t->depth], 32, hipMemcpyDeviceToHost, en.s));
  return en.finish();
}

// k requests over a resident tree: audit paths (a = index, b = tree_size, roots_out given) or
// consistency proofs (a = first, b = second).  host: the arrays are host memory and every
// request is checked before any launch; else they are device memory and the kernel marks a
// refused request in its length.
static int tree_requests(int32_t handle, const uint64_t* a, const uint64_t* b, uint64_t k, uint8_t* nodes_out,
                         uint32_t* len_out, uint8_t* roots_out, bool paths, bool host, void* stream) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (k == 0) return PV_OK;
  if (!a || !b || !nodes_out || !len_out || (paths && !roots_out)) return fail(PV_EINVAL, "null buffer");
  if (host) {
    for (uint64_t i = 0; i < k; ++i)   // refused before any launch, never clamped
      if (paths ? (b[i] == 0 || b[i] > t->n || a[i] >= b[i]) : (a[i] > b[i] || b[i] > t->n))
        return fail(PV_EINVAL, "request %llu: (%llu, %llu) outside a tree of %llu leaves", (unsigned long long)i,
                    (unsigned long long)a[i], (unsigned long long)b[i], (unsigned long long)t->n);
  } else if (misaligned16(nodes_out) || misaligned16(roots_out)) {
    return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  }
  if (const int rc = en.begin(stream)) return rc;
  hipStream_t s = en.s;
  const uint64_t node_bytes = k * ((uint64_t)t->depth + 1) * 32;
  TmpBuf<uint64_t> da, db;
  TmpBuf<uint8_t> dnodes, droots;
  TmpBuf<uint32_t> dlen;
  StreamDrain tail{s};
  const uint64_t *pa = a, *pb = b;
  uint8_t *pn = nodes_out, *pr = roots_out;
  uint32_t* pl = len_out;
  if (host) {
    HIP_OK(da.put(a, k, s));
    HIP_OK(db.put(b, k, s));
    HIP_OK(dnodes.alloc(node_bytes));
    HIP_OK(droots.alloc(k * 32));
    HIP_OK(dlen.alloc(k));
    pa = da.p, pb = db.p, pn = dnodes.p, pr = droots.p, pl = dlen.p;
  }
  if (paths)
    HIP_OK(pv::launch_merkle_paths(t->table, t->n, t->depth, pa, pb, k, w32(pn), pl, w32(pr), merkle_blocks(*en.d), s));
  else
    HIP_OK(pv::launch_merkle_cons_proofs(t->table, t->n, t->depth, pa, pb, k, w32(pn), pl, merkle_blocks(*en.d), s));
  if (host) {
    HIP_OK(hipMemcpyAsync(nodes_out, pn, node_bytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(len_out, pl, k * 4, hipMemcpyDeviceToHost, s));
    if (paths) HIP_OK(hipMemcpyAsync(roots_out, pr, k * 32, hipMemcpyDeviceToHost, s));
  }
  return tail.finish();
}

int pv_merkle_audit_paths_device(int32_t handle, const uint64_t* index, const uint64_t* tree_size, uint64_t k,
                                 uint8_t* nodes_out, uint32_t* len_out, uint8_t* roots_out, void* stream) {
  return tree_requests(handle, index, tree_size, k, nodes_out, len_out, roots_out, true, false, stream);
}

int pv_merkle_audit_paths(int32_t handle, const uint64_t* index, const uint64_t* tree_size, uint64_t k,
                          uint8_t* nodes_out, uint32_t* len_out, uint8_t* roots_out) {
  return tree_requests(handle, index, tree_size, k, nodes_out, len_out, roots_out, true, true, nullptr);
}

int pv_merkle_consistency_proofs_device(int32_t handle, const uint64_t* first, const uint64_t* second, uint64_t k,
                                        uint8_t* nodes_out, uint32_t* len_out, void* stream) {
  return tree_requests(handle, first, second, k, nodes_out, len_out, nullptr, false, false, stream);
}

int pv_merkle_consistency_proofs(int32_t handle, const uint64_t* first, const uint64_t* second, uint64_t k,
                                 uint8_t* nodes_out, uint32_t* len_out) {
  return tree_requests(handle, first, second, k, nodes_out, len_out, nullptr, false, true, nullptr);
}

// ------------------------------------------------ the ledger write cycle
// stage k leaf hashes from host or device memory
static int tree_stage_hashes(int32_t handle, const uint8_t* leaf_hashes, uint64_t k, uint8_t* root_out,
                             hipMemcpyKind kind, void* stream) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (k == 0) return PV_OK;   // as extend: nothing staged, nothing written
  if (!leaf_hashes) return fail(PV_EINVAL, "null buffer");
  if (k > (1ull << 40) || t->n + k > (1ull << 40)) return fail(PV_EINVAL, "tree limited to 2^40 leaves");
  if (const int rc = en.begin(stream)) return rc;
  if (const int rc = tree_grow(*t, 0, t->n + k, en.s)) return rc;
  HIP_OK(hipMemcpyAsync(t->lv[0] + 8 * t->n, leaf_hashes, k * 32, kind, en.s));
  return en.finish(tree_stage(*t, k, root_out, en.s));
}

int pv_merkle_tree_stage_hashes(int32_t handle, const uint8_t* leaf_hashes, uint64_t k, uint8_t* root_out) {
  return tree_stage_hashes(handle, leaf_hashes, k, root_out, hipMemcpyHostToDevice, nullptr);
}

int pv_merkle_tree_stage_hashes_device(int32_t handle, const uint8_t* leaf_hashes, uint64_t k, uint8_t* root_out,
                                       void* stream) {
  return tree_stage_hashes(handle, leaf_hashes, k, root_out, hipMemcpyDeviceToDevice, stream);
}

int pv_merkle_tree_stage(int32_t handle, const uint8_t* blob, const uint64_t* off, uint64_t k, uint8_t* root_out) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (k == 0) return PV_OK;   // as extend: nothing staged, nothing written
  if (!off || (!blob && off[k] != off[0])) return fail(PV_EINVAL, "null buffer");
  if (k > (1ull << 40) || t->n + k > (1ull << 40)) return fail(PV_EINVAL, "tree limited to 2^40 leaves");
  Ragged leaf(off, k);
  if (const int rc = leaf.check("off")) return rc;
  if (const int rc = en.begin()) return rc;
  Device* d = en.d;
  hipStream_t s = en.s;
  if (const int rc = leaf.stage(blob, *d, s)) return rc;
  if (const int rc = tree_grow(*t, 0, t->n + k, s)) return rc;
  HIP_OK(pv::launch_sha256(d->blob.p, d->off.p, k, 1, 0x00, d->counter.p, t->lv[0] + 8 * t->n, d->sha256_blocks, s));
  return en.finish(tree_stage(*t, k, root_out, s));
}

int pv_merkle_tree_commit(int32_t handle, uint64_t count) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (count > t->n - t->committed)
    return fail(PV_EINVAL, "commit of %llu leaves, %llu staged", (unsigned long long)count,
                (unsigned long long)(t->n - t->committed));
  t->committed += count;
  return PV_OK;
}

int pv_merkle_tree_discard(int32_t handle, uint64_t count, uint8_t* root_out) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (count > t->n - t->committed)
    return fail(PV_EINVAL, "expected to revert %llu txns while there are only %llu", (unsigned long long)count,
                (unsigned long long)(t->n - t->committed));
  if (const int rc = en.begin()) return rc;
  if (count) {
    const uint64_t n_new = t->n - count;
    if (const int rc = tree_edge(*t, n_new ? n_new - 1 : 0, n_new, en.s)) return rc;
  }
  return en.finish(tree_root(*t, root_out, en.s));
}

int pv_merkle_tree_sizes(int32_t handle, uint64_t* committed, uint64_t* total) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (committed) *committed = t->committed;
  if (total) *total = t->n;
  return PV_OK;
}

int pv_merkle_tree_frontier(int32_t handle, uint64_t tree_size, uint8_t* hashes_out, uint32_t* count_out) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (tree_size > t->n)
    return fail(PV_EINVAL, "frontier of %llu leaves outside a tree of %llu", (unsigned long long)tree_size,
                (unsigned long long)t->n);
  const uint32_t cnt = (uint32_t)__builtin_popcountll(tree_size);
  if (count_out) *count_out = cnt;
  if (cnt == 0 || !hashes_out) return PV_OK;
  if (const int rc = en.begin()) return rc;
  TmpBuf<uint8_t> dout;
  StreamDrain tail{en.s};
  HIP_OK(dout.alloc(64 * 32));
  HIP_OK(pv::launch_merkle_frontier(t->table, tree_size, w32(dout.p), en.s));
  HIP_OK(hipMemcpyAsync(hashes_out, dout.p, (size_t)cnt * 32, hipMemcpyDeviceToHost, en.s));
  return tail.finish();
}

// nodes the reference's hash store receives while leaves first + 1 .. last are appended
static uint64_t hs_nodes(uint64_t first, uint64_t last) {
  return (last - (uint64_t)__builtin_popcountll(last)) - (first - (uint64_t)__builtin_popcountll(first));
}

static int tree_hs_range(const MerkleTree& t, uint64_t first, uint64_t last) {
  if (first > last || last > t.n)
    return fail(PV_EINVAL, "leaves (%llu, %llu] outside a tree of %llu", (unsigned long long)first,
                (unsigned long long)last, (unsigned long long)t.n);
  return PV_OK;
}

static int tree_hash_store(int32_t handle, uint64_t first, uint64_t last, uint8_t* leaf_out, uint8_t* node_out,
                           uint64_t node_cap, uint64_t* n_nodes, bool host, void* stream) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (const int rc = tree_hs_range(*t, first, last)) return rc;
  const uint64_t need = hs_nodes(first, last);
  if (n_nodes) *n_nodes = need;
  if (node_out && node_cap < need)
    return fail(PV_EINVAL, "node_cap %llu below the %llu nodes of the range", (unsigned long long)node_cap,
                (unsigned long long)need);
  if (first == last || (!leaf_out && !(node_out && need))) return PV_OK;
  if (!host && (misaligned16(leaf_out) || misaligned16(node_out)))
    return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dleaf, dnode;
  StreamDrain tail{s};
  uint8_t *pl = leaf_out, *pn = need ? node_out : nullptr;
  if (host) {
    if (pl) {
      HIP_OK(dleaf.alloc((last - first) * 32));
      pl = dleaf.p;
    }
    if (pn) {
      HIP_OK(dnode.alloc(need * 32));
      pn = dnode.p;
    }
  }
  HIP_OK(pv::launch_merkle_hs_gather(t->table, first, last, w32(pl), w32(pn), merkle_blocks(*en.d), s));
  if (host) {
    if (pl) HIP_OK(hipMemcpyAsync(leaf_out, pl, (last - first) * 32, hipMemcpyDeviceToHost, s));
    if (pn) HIP_OK(hipMemcpyAsync(node_out, pn, need * 32, hipMemcpyDeviceToHost, s));
  }
  return tail.finish();
}

int pv_merkle_tree_hash_store(int32_t handle, uint64_t first, uint64_t last, uint8_t* leaf_out, uint8_t* node_out,
                              uint64_t node_cap, uint64_t* n_nodes) {
  return tree_hash_store(handle, first, last, leaf_out, node_out, node_cap, n_nodes, true, nullptr);
}

int pv_merkle_tree_hash_store_device(int32_t handle, uint64_t first, uint64_t last, uint8_t* leaf_out,
                                     uint8_t* node_out, uint64_t node_cap, uint64_t* n_nodes, void* stream) {
  return tree_hash_store(handle, first, last, leaf_out, node_out, node_cap, n_nodes, false, stream);
}

int pv_merkle_tree_check_nodes(int32_t handle, uint64_t first, uint64_t last, const uint8_t* node_hashes,
                               uint64_t* n_bad, uint64_t* first_bad) {
  Entry en;
  MerkleTree* t;
  if (const int rc = tree_enter(en, handle, &t)) return rc;
  if (const int rc = tree_hs_range(*t, first, last)) return rc;
  if (!n_bad || !first_bad) return fail(PV_EINVAL, "null pointer");
  const uint64_t need = hs_nodes(first, last);
  *n_bad = 0;
  *first_bad = UINT64_MAX;
  if (need == 0) return PV_OK;
  if (!node_hashes) return fail(PV_EINVAL, "null buffer");
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dnodes;
  TmpBuf<unsigned long long> dres;
  StreamDrain tail{s};
  unsigned long long res[2] = {0, ~0ull};
  HIP_OK(dnodes.put(node_hashes, need * 32, s));
  HIP_OK(dres.put(res, 2, s));
  HIP_OK(pv::launch_merkle_hs_check(t->table, first, last, w32(dnodes.p), dres.p, merkle_blocks(*en.d), s));
  HIP_OK(hipMemcpyAsync(res, dres.p, sizeof(res), hipMemcpyDeviceToHost, s));
  if (const int rc = tail.finish()) return rc;
  *n_bad = res[0];
  *first_bad = res[1];
  return PV_OK;
}

// ------------------------------------------------ SHA3-256 / state proofs
int pv_sha3_256_batch_device(const uint8_t* blob, const uint64_t* off, uint64_t n, uint8_t* digests, int device,
                             void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!blob || !off || !digests) return fail(PV_EINVAL, "null device buffer");
  if (misaligned16(digests)) return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(blob) & 3u) return fail(PV_EINVAL, "blob must be 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_sha3_256(blob, off, off + 1, n, en.d->counter.p, w32(digests), en.d->sha3_blocks, en.s));
  return en.finish();
}

int pv_sha3_256_batch(const uint8_t* blob, const uint64_t* off, uint64_t n, uint8_t* digests) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (n == 0) return PV_OK;
  if (!off || !digests || (!blob && off[n] != off[0])) return fail(PV_EINVAL, "null buffer");
  Ragged msgs(off, n);
  if (const int rc = msgs.check("off")) return rc;
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  HIP_OK(d.mk0.ensure(n * 8));
  if (const int rc = msgs.stage(blob, d, d.stream)) return rc;
  HIP_OK(pv::launch_sha3_256(d.blob.p, d.off.p, d.off.p + 1, n, d.counter.p, d.mk0.p, d.sha3_blocks, d.stream));
  HIP_OK(hipMemcpyAsync(digests, d.mk0.p, n * 32, hipMemcpyDeviceToHost, d.stream));
  return en.finish();
}

int pv_rlp_split_list(const uint8_t* rlp, uint64_t len, uint64_t* item_beg, uint64_t* item_end, uint64_t cap,
                      uint64_t* count) {
  if (!count || (len && !rlp) || (cap && (!item_beg || !item_end))) return fail(PV_EINVAL, "null buffer");
  if (!pv::rlp_split_list(rlp, len, item_beg, item_end, cap, count))
    return fail(PV_EINVAL, "not one RLP list of at most %llu items ending at its end", (unsigned long long)cap);
  return PV_OK;
}

int pv_state_proof_verify_device(const uint8_t* node_blob, const uint64_t* node_beg, const uint64_t* node_end,
                                 const uint64_t* proof_first, const uint8_t* roots, const uint32_t* proof_idx,
                                 const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob,
                                 const uint64_t* val_off, uint64_t N, uint64_t P, uint64_t Q, uint8_t* status,
                                 uint8_t* node_digests, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (Q == 0) return PV_OK;
  if (!proof_first || !roots || !proof_idx || !key_off || !val_off || !status ||
      (N && (!node_blob || !node_beg || !node_end || !node_digests)))
    return fail(PV_EINVAL, "null device buffer");
  if (P == 0) return fail(PV_EINVAL, "queries without proofs");
  if (misaligned16(node_digests) || (reinterpret_cast<uintptr_t>(roots) & 3u) ||
      (reinterpret_cast<uintptr_t>(node_blob) & 3u))
    return fail(PV_EINVAL, "node_digests must be 16-byte aligned, roots and node_blob 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  Device* d = en.d;
  hipStream_t s = en.s;
  HIP_OK(pv::launch_sha3_256(node_blob, node_beg, node_end, N, d->counter.p, w32(node_digests), d->sha3_blocks, s));
  HIP_OK(pv::launch_trie_verify(node_blob, node_beg, node_end, w32(node_digests), proof_first, w32(roots), P,
                                proof_idx, key_blob, key_off, val_blob, val_off, Q, status, merkle_blocks(*d), s));
  return en.finish();
}

int pv_state_proof_verify(const uint8_t* node_blob, uint64_t node_blob_len, const uint64_t* node_beg,
                          const uint64_t* node_end, const uint64_t* proof_first, const uint8_t* roots,
                          const uint32_t* proof_idx, const uint8_t* key_blob, const uint64_t* key_off,
                          const uint8_t* val_blob, const uint64_t* val_off, uint64_t N, uint64_t P, uint64_t Q,
                          uint8_t* status) {
  Entry en;
  if (const int rc = en.check()) return rc;
  if (Q == 0) return PV_OK;
  if (!proof_first || !roots || !proof_idx || !key_off || !val_off || !status ||
      (N && (!node_beg || !node_end)) || (node_blob_len && !node_blob))
    return fail(PV_EINVAL, "null buffer");
  if (P == 0) return fail(PV_EINVAL, "queries without proofs");
  Ragged keys(key_off, Q), vals(val_off, Q);
  if (const int rc = keys.check("key_off")) return rc;
  if (const int rc = vals.check("val_off")) return rc;
  if ((keys.len && !key_blob) || (vals.len && !val_blob)) return fail(PV_EINVAL, "null buffer");
  for (uint64_t j = 0; j < N; ++j)
    if (node_beg[j] > node_end[j] || node_end[j] > node_blob_len)
      return fail(PV_EINVAL, "node %llu lies outside the blob", (unsigned long long)j);
  if (const int rc = offsets_ok(proof_first, P, "proof_first")) return rc;
  if (proof_first[P] != N)
    return fail(PV_EINVAL, "proof_first ends at %llu, not at N = %llu", (unsigned long long)proof_first[P],
                (unsigned long long)N);
  for (uint64_t i = 0; i < Q; ++i)
    if (proof_idx[i] >= P)
      return fail(PV_EINVAL, "proof_idx[%llu] = %u is not below P = %llu", (unsigned long long)i, proof_idx[i],
                  (unsigned long long)P);
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dblob, droots, dkeys, dvals, dstatus, ddig;
  TmpBuf<uint64_t> dbeg, dend, dfirst, dkoff, dvoff;
  TmpBuf<uint32_t> dpidx;
  StreamDrain tail{s};
  HIP_OK(dblob.alloc(node_blob_len + 16));
  if (const int rc = upload_padded(dblob.p, node_blob, node_blob_len, s)) return rc;
  HIP_OK(dbeg.put(node_beg, N, s));
  HIP_OK(dend.put(node_end, N, s));
  HIP_OK(dfirst.put(proof_first, P + 1, s));
  HIP_OK(droots.put(roots, P * 32, s));
  HIP_OK(dpidx.put(proof_idx, Q, s));
  HIP_OK(dkeys.put(keys.len ? key_blob + keys.b0 : nullptr, keys.len, s));
  HIP_OK(dkoff.put(keys.rebased(), Q + 1, s));
  HIP_OK(dvals.put(vals.len ? val_blob + vals.b0 : nullptr, vals.len, s));
  HIP_OK(dvoff.put(vals.rebased(), Q + 1, s));
  HIP_OK(dstatus.alloc(Q));
  HIP_OK(ddig.alloc(N * 32));
  HIP_OK(pv::launch_sha3_256(dblob.p, dbeg.p, dend.p, N, d.counter.p, w32(ddig.p), d.sha3_blocks, s));
  HIP_OK(pv::launch_trie_verify(dblob.p, dbeg.p, dend.p, w32(ddig.p), dfirst.p, w32(droots.p), P, dpidx.p, dkeys.p,
                                dkoff.p, dvals.p, dvoff.p, Q, dstatus.p, merkle_blocks(d), s));
  HIP_OK(hipMemcpyAsync(status, dstatus.p, Q, hipMemcpyDeviceToHost, s));
  return tail.finish();
}

int pv_synth_layout_device(uint32_t cfg, uint32_t mode, uint64_t first, uint64_t n, uint32_t mlen_min,
                           uint32_t mlen_max, uint32_t n_nodes, uint64_t* off, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (!off) return fail(PV_EINVAL, "null device buffer");
  if (mode > PV_SYNTH_COMMIT) return fail(PV_EINVAL, "unknown synth mode %u", mode);
  if (mode == PV_SYNTH_RANGE && mlen_max < mlen_min) return fail(PV_EINVAL, "mlen_max < mlen_min");
  if (mode == PV_SYNTH_COMMIT && (n_nodes == 0 || n_nodes > 1024))
    return fail(PV_EINVAL, "n_nodes must be in 1..1024");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(en.d->scan.ensure(pv::scan_sums_words(n + 1)));
  HIP_OK(pv::launch_synth_layout(cfg, mode, first, n, mlen_min, mlen_max, n_nodes, off, en.d->scan.p, en.s));
  return en.finish();
}

int pv_synth_fill_device(uint32_t cfg, uint32_t mode, uint64_t first, uint64_t n, uint32_t key_mod,
                         uint32_t n_nodes, const uint64_t* off, uint8_t* blob, uint8_t* seeds, uint8_t* pk,
                         uint8_t* sig, uint8_t* tamper, uint32_t* sender, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (!off || !blob || !seeds || !pk || !sig || !tamper) return fail(PV_EINVAL, "null device buffer");
  if (mode > PV_SYNTH_COMMIT) return fail(PV_EINVAL, "unknown synth mode %u", mode);
  if (mode == PV_SYNTH_COMMIT && (n_nodes == 0 || n_nodes > 1024))
    return fail(PV_EINVAL, "n_nodes must be in 1..1024");
  if (const int rc = en.begin(stream)) return rc;
  hipStream_t s = en.s;
  uint64_t total = 0;
  HIP_OK(hipMemcpyAsync(&total, off + n, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  HIP_OK(pv::launch_synth(cfg, mode, first, n, key_mod, n_nodes, seeds, tamper, sender, s));
  HIP_OK(pv::launch_synth_fill(cfg, mode, first, n, n_nodes, off, blob, s));
  HIP_OK(hipMemsetAsync(blob + total, 0, 16, s));
  HIP_OK(pv::launch_sign(seeds, blob, off, n, en.d->btab.p, pk, sig, s));
  HIP_OK(pv::launch_tamper(first, n, tamper, off, blob, sig, s));
  return en.finish();
}

int pv_synth_device(uint32_t cfg, uint64_t first, uint64_t n, uint32_t key_mod, uint32_t mlen, uint64_t* off,
                    uint8_t* blob, uint8_t* seeds, uint8_t* pk, uint8_t* sig, uint8_t* tamper, int device,
                    void* stream) {
  int rc = pv_synth_layout_device(cfg, PV_SYNTH_FIXED, first, n, mlen, mlen, 0, off, device, stream);
  if (rc) return rc;
  return pv_synth_fill_device(cfg, PV_SYNTH_FIXED, first, n, key_mod, 0, off, blob, seeds, pk, sig, tamper, nullptr,
                              device, stream);
}

}  // extern "C"

// --------------------------------- resident trie node store / proof generation
namespace {

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
std::vector<StateStore> g_stores;   // store id = index + 1

void store_release(StateStore& st) {
  if (!st.live) return;
  if (Device* d = find_dev(st.dev)) {
    (void)hipSetDevice(d->ord);
    (void)hipStreamSynchronize(d->stream);
  }
  void* bufs[] = {st.blob, st.beg, st.end, st.dig, st.dup, st.table, st.unique};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  st = StateStore();
}

StateStore* find_store(int32_t id) {
  if (id < 1 || (size_t)id > g_stores.size() || !g_stores[id - 1].live) return nullptr;
  return &g_stores[id - 1];
}

// resolve a store id and point the entry scope at the store's device
int store_enter(Entry& en, int32_t id, StateStore** st) {
  if (const int rc = en.check()) return rc;
  *st = find_store(id);
  if (!*st) return fail(PV_EINVAL, "no state store with id %d", (int)id);
  en.d = find_dev((*st)->dev);
  if (!en.d) return fail(PV_EINVAL, "the device of state store %d is gone", (int)id);
  return PV_OK;
}

// *p holds at least `need` elements afterwards (+ `pad` elements never counted
// in the capacity); the `used` elements in use move device-to-device on s
template <typename T>
int store_grow(T** p, uint64_t* cap, uint64_t need, uint64_t used, uint64_t pad, hipStream_t s) {
  if (*p && need <= *cap) return PV_OK;
  uint64_t nc = *cap ? *cap : 1;
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

int store_reserve(StateStore& st, uint64_t nodes, uint64_t bytes, hipStream_t s) {
  if (const int rc = store_grow(&st.blob, &st.cap_bytes, bytes, st.n_bytes, 16, s)) return rc;
  if (nodes <= st.cap_nodes && st.beg) return PV_OK;
  // the four per-node arrays grow in step: same start, same doubling
  uint64_t c0 = st.cap_nodes, c1 = st.cap_nodes, c2 = st.cap_nodes, cd = st.cap_nodes * 8;
  if (const int rc = store_grow(&st.beg, &c0, nodes, st.n_nodes, 0, s)) return rc;
  if (const int rc = store_grow(&st.end, &c1, nodes, st.n_nodes, 0, s)) return rc;
  if (const int rc = store_grow(&st.dup, &c2, nodes, st.n_nodes, 0, s)) return rc;
  if (const int rc = store_grow(&st.dig, &cd, c0 * 8, st.n_nodes * 8, 0, s)) return rc;
  st.cap_nodes = c0;
  return PV_OK;
}

// a table of `slots` slots holding every node that has one; launched before an
// insert that would push the nodes above slots / 2
int store_rehash(StateStore& st, uint32_t slots, const Device& d, hipStream_t s) {
  uint32_t* nt = nullptr;
  HIP_OK(hipMalloc(reinterpret_cast<void**>(&nt), (size_t)slots * 4));
  hipError_t e = hipMemsetAsync(nt, 0, (size_t)slots * 4, s);
  if (e == hipSuccess)
    e = pv::launch_trie_store_rehash(nt, slots, st.dig, st.dup, (uint32_t)st.n_nodes, merkle_blocks(d), s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipFree(nt);
    HIP_OK(e);
  }
  if (st.table) (void)hipFree(st.table);
  st.table = nt;
  st.slots = slots;
  return PV_OK;
}

// pv_state_store_add[_device]: host = the arrays are host memory and checked here
int store_add(int32_t id, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new, uint8_t* digests,
              uint64_t* n_added, bool host, void* stream) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, id, &st)) return rc;
  if (n_added) *n_added = 0;
  if (n_new == 0) return PV_OK;
  if (!node_blob || !node_off) return fail(PV_EINVAL, host ? "null buffer" : "null device buffer");
  if (n_new > pv::TS_MAX_NODES || st->n_nodes + n_new > pv::TS_MAX_NODES)
    return fail(PV_EINVAL, "state store limited to 2^32 - 2 nodes");
  if (host)
    for (uint64_t i = 0; i < n_new; ++i)
      if (node_off[i + 1] <= node_off[i])
        return fail(PV_EINVAL, "node_off not strictly increasing at %llu (an empty node)", (unsigned long long)i);
  if (const int rc = en.begin(stream)) return rc;
  Device& d = *en.d;
  hipStream_t s = en.s;
  uint64_t ends[2] = {0, 0};   // node_off[0], node_off[n_new]
  if (host) {
    ends[0] = node_off[0];
    ends[1] = node_off[n_new];
  } else {   // the two ends size the copy; the offsets between them are read by the kernel only
    HIP_OK(hipMemcpyAsync(&ends[0], node_off, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(&ends[1], node_off + n_new, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (ends[1] < ends[0]) return fail(PV_EINVAL, "node_off ends below its start");
  }
  const uint64_t total = ends[1] - ends[0];
  if (total > (1ull << 40)) return fail(PV_EINVAL, "more than 2^40 bytes of nodes in one call");
  const uint64_t nodes = st->n_nodes + n_new;
  if (const int rc = store_reserve(*st, nodes, st->n_bytes + total, s)) return rc;
  TmpBuf<uint64_t> doff;
  StreamDrain tail{s};
  const uint64_t* poff = node_off;
  if (host) {
    HIP_OK(doff.put(node_off, n_new + 1, s));
    poff = doff.p;
  }
  if (total)
    HIP_OK(hipMemcpyAsync(st->blob + st->n_bytes, node_blob + ends[0], total,
                          host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemsetAsync(st->blob + st->n_bytes + total, 0, 16, s));
  HIP_OK(hipMemsetAsync(st->dup + st->n_nodes, 0, n_new, s));
  HIP_OK(pv::launch_trie_store_layout(poff, n_new, st->n_bytes, total, st->beg, st->end, st->n_nodes,
                                      merkle_blocks(d), s));
  HIP_OK(pv::launch_sha3_256(st->blob, st->beg + st->n_nodes, st->end + st->n_nodes, n_new, d.counter.p,
                             st->dig + 8 * st->n_nodes, d.sha3_blocks, s));
  if (nodes > st->slots / 2) {
    uint64_t ns = st->slots;
    while (nodes > ns / 2) ns *= 2;   // nodes < 2^32, so ns <= 2^33
    if (ns > (1ull << 31)) return fail(PV_ENOMEM, "state store table above 2^31 slots");
    if (const int rc = store_rehash(*st, (uint32_t)ns, d, s)) return rc;
  }
  HIP_OK(pv::launch_trie_store_insert(st->table, st->slots, st->dig, st->dup, (uint32_t)st->n_nodes, (uint32_t)n_new,
                                      st->unique, merkle_blocks(d), s));
  unsigned int uniq = 0;
  HIP_OK(hipMemcpyAsync(&uniq, st->unique, 4, hipMemcpyDeviceToHost, s));
  if (digests)
    HIP_OK(hipMemcpyAsync(digests, st->dig + 8 * st->n_nodes, n_new * 32,
                          host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
  if (const int rc = tail.finish()) return rc;
  if (n_added) *n_added = uniq - st->n_unique;
  st->n_unique = uniq;
  st->n_nodes = nodes;
  st->n_bytes += total;
  return PV_OK;
}

}  // namespace

extern "C" {

int pv_state_store_create(uint64_t node_hint, uint64_t byte_hint, int device, int32_t* store_out) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (!store_out) return fail(PV_EINVAL, "null pointer");
  if (node_hint > pv::TS_MAX_NODES) return fail(PV_EINVAL, "node_hint above 2^32 - 2 nodes");
  if (byte_hint > (1ull << 40)) return fail(PV_EINVAL, "byte_hint above 2^40 bytes");
  size_t idx = 0;
  while (idx < g_stores.size() && g_stores[idx].live) ++idx;
  if (idx == g_stores.size()) {
    if (g_stores.size() >= 0x7fffffffull) return fail(PV_ENOMEM, "too many state stores");
    g_stores.emplace_back();
  }
  StateStore& st = g_stores[idx];
  st = StateStore();
  st.live = true;
  st.dev = en.d->id;
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  uint64_t slots = pv::TS_MIN_SLOTS;
  while (node_hint > slots / 2) slots *= 2;
  int rc = slots > (1ull << 31) ? fail(PV_ENOMEM, "state store table above 2^31 slots") : PV_OK;
  if (rc == PV_OK) rc = store_reserve(st, node_hint ? node_hint : 1, byte_hint ? byte_hint : 1, s);
  if (rc == PV_OK) rc = store_rehash(st, (uint32_t)slots, *en.d, s);   // an empty table
  if (rc == PV_OK) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&st.unique), 4);
    if (e == hipSuccess) e = hipMemsetAsync(st.unique, 0, 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(st.blob, 0, 16, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(PV_EIO, "state store allocation failed: %s", hipGetErrorString(e));
  }
  if (rc) {
    store_release(st);
    return rc;
  }
  *store_out = (int32_t)(idx + 1);
  return PV_OK;
}

int pv_state_store_free(int32_t store) {
  std::lock_guard<std::mutex> lk(g_mu);
  DeviceGuard dg;
  StateStore* st = find_store(store);
  if (!st) return fail(PV_EINVAL, "no state store with id %d", (int)store);
  store_release(*st);
  return PV_OK;
}

int pv_state_store_add(int32_t store, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new,
                       uint8_t* digests, uint64_t* n_added) {
  return store_add(store, node_blob, node_off, n_new, digests, n_added, true, nullptr);
}

int pv_state_store_add_device(int32_t store, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new,
                              uint8_t* digests, void* stream) {
  return store_add(store, node_blob, node_off, n_new, digests, nullptr, false, stream);
}

int pv_state_store_info(int32_t store, uint64_t* n_nodes, uint64_t* n_unique, uint64_t* n_bytes, uint64_t* n_slots) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_nodes) *n_nodes = st->n_nodes;
  if (n_unique) *n_unique = st->n_unique;
  if (n_bytes) *n_bytes = st->n_bytes;
  if (n_slots) *n_slots = st->slots;
  return PV_OK;
}

int pv_state_store_walk_device(int32_t store, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots,
                               const uint8_t* key_blob, const uint64_t* key_off, uint64_t n_queries,
                               uint32_t max_nodes, uint8_t* status, uint32_t* node_count, uint32_t* node_ids,
                               uint64_t* proof_len, uint64_t* val_rel, uint64_t* val_len, void* stream) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_queries == 0) return PV_OK;
  if (!roots || !key_blob || !key_off || !status || !node_count || !node_ids || !proof_len || !val_rel || !val_len)
    return fail(PV_EINVAL, "null device buffer");
  if (max_nodes == 0) return fail(PV_EINVAL, "max_nodes must be >= 1");
  if (n_roots == 0) return fail(PV_EINVAL, "queries without roots");
  if (n_queries > (1ull << 40) / max_nodes) return fail(PV_EINVAL, "n_queries x max_nodes above 2^40 node ids");
  if (reinterpret_cast<uintptr_t>(roots) & 3u) return fail(PV_EINVAL, "roots must be 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_trie_prove(st->blob, st->beg, st->end, st->dig, st->table, st->slots, (uint32_t)st->n_nodes,
                               w32(roots), root_idx, n_roots, key_blob, key_off, n_queries, max_nodes, status,
                               node_count, node_ids, proof_len, val_rel, val_len, merkle_blocks(*en.d), en.s));
  return en.finish();
}

int pv_state_store_pack_device(int32_t store, const uint32_t* node_ids, const uint32_t* node_count,
                               uint32_t max_nodes, const uint64_t* proof_off, uint64_t n_queries,
                               uint8_t* proof_blob, void* stream) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_queries == 0) return PV_OK;
  if (!node_ids || !node_count || !proof_off || !proof_blob) return fail(PV_EINVAL, "null device buffer");
  if (max_nodes == 0) return fail(PV_EINVAL, "max_nodes must be >= 1");
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(pv::launch_trie_proof_pack(st->blob, st->beg, st->end, (uint32_t)st->n_nodes, node_ids, node_count,
                                    max_nodes, proof_off, n_queries, proof_blob, merkle_blocks(*en.d), en.s));
  return en.finish();
}

int pv_state_store_prove(int32_t store, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots,
                         const uint8_t* key_blob, const uint64_t* key_off, uint64_t n_queries, uint32_t max_nodes,
                         uint8_t* status, uint32_t* node_count, uint64_t* proof_off, uint64_t* val_rel,
                         uint64_t* val_len, uint8_t* proof_blob, uint64_t proof_cap) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_queries == 0) return PV_OK;
  if (!roots || !key_off || !status || !node_count || !proof_off || !val_rel || !val_len)
    return fail(PV_EINVAL, "null buffer");
  if (max_nodes == 0) return fail(PV_EINVAL, "max_nodes must be >= 1");
  if (n_roots == 0) return fail(PV_EINVAL, "queries without roots");
  if (n_queries > (1ull << 40) / max_nodes) return fail(PV_EINVAL, "n_queries x max_nodes above 2^40 node ids");
  if (!root_idx && n_roots < n_queries)
    return fail(PV_EINVAL, "%llu roots for %llu queries without root_idx", (unsigned long long)n_roots,
                (unsigned long long)n_queries);
  Ragged keys(key_off, n_queries);
  if (const int rc = keys.check("key_off")) return rc;
  if (keys.len && !key_blob) return fail(PV_EINVAL, "null buffer");
  if (root_idx)
    for (uint64_t i = 0; i < n_queries; ++i)
      if (root_idx[i] >= n_roots)
        return fail(PV_EINVAL, "root_idx[%llu] = %u is not below n_roots %llu", (unsigned long long)i, root_idx[i],
                    (unsigned long long)n_roots);
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> droots, dkeys, dstatus, dproof;
  TmpBuf<uint32_t> dridx, dcount, dids;
  TmpBuf<uint64_t> dkoff, dlen, dvrel, dvlen, dpoff;
  StreamDrain tail{s};
  HIP_OK(droots.put(roots, n_roots * 32, s));
  if (root_idx) HIP_OK(dridx.put(root_idx, n_queries, s));
  HIP_OK(dkeys.alloc(keys.len + 4));
  if (keys.len) HIP_OK(hipMemcpyAsync(dkeys.p, key_blob + keys.b0, keys.len, hipMemcpyHostToDevice, s));
  HIP_OK(dkoff.put(keys.rebased(), n_queries + 1, s));
  HIP_OK(dstatus.alloc(n_queries));
  HIP_OK(dcount.alloc(n_queries));
  HIP_OK(dids.alloc(n_queries * max_nodes));
  HIP_OK(dlen.alloc(n_queries));
  HIP_OK(dvrel.alloc(n_queries));
  HIP_OK(dvlen.alloc(n_queries));
  HIP_OK(pv::launch_trie_prove(st->blob, st->beg, st->end, st->dig, st->table, st->slots, (uint32_t)st->n_nodes,
                               w32(droots.p), root_idx ? dridx.p : nullptr, n_roots, dkeys.p, dkoff.p, n_queries,
                               max_nodes, dstatus.p, dcount.p, dids.p, dlen.p, dvrel.p, dvlen.p, merkle_blocks(d), s));
  HIP_OK(hipMemcpyAsync(status, dstatus.p, n_queries, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(node_count, dcount.p, n_queries * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(proof_off + 1, dlen.p, n_queries * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(val_rel, dvrel.p, n_queries * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(val_len, dvlen.p, n_queries * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  proof_off[0] = 0;   // the lengths, scanned in place
  for (uint64_t i = 0; i < n_queries; ++i) proof_off[i + 1] += proof_off[i];
  const uint64_t total = proof_off[n_queries];
  if (!proof_blob) return tail.finish();   // the sizing call
  if (proof_cap < total)
    return fail(PV_EINVAL, "proof_cap %llu is below the %llu bytes of the proofs", (unsigned long long)proof_cap,
                (unsigned long long)total);
  if (total == 0) return tail.finish();
  HIP_OK(dpoff.put(proof_off, n_queries + 1, s));
  HIP_OK(dproof.alloc(total));
  HIP_OK(pv::launch_trie_proof_pack(st->blob, st->beg, st->end, (uint32_t)st->n_nodes, dids.p, dcount.p, max_nodes,
                                    dpoff.p, n_queries, dproof.p, merkle_blocks(d), s));
  HIP_OK(hipMemcpyAsync(proof_blob, dproof.p, total, hipMemcpyDeviceToHost, s));
  return tail.finish();
}

}  // extern "C"

namespace {

// the buffers a prune builds beside the store's own: freed unless the swap took them
struct FreshStore {
  uint8_t* blob = nullptr;
  uint64_t *beg = nullptr, *end = nullptr;
  uint32_t *dig = nullptr, *table = nullptr;
  uint8_t* dup = nullptr;
  unsigned int* unique = nullptr;
  bool taken = false;
  ~FreshStore() {
    if (taken) return;
    void* bufs[] = {blob, beg, end, dig, table, dup, unique};
    for (void* p : bufs)
      if (p) (void)hipFree(p);
  }
};

template <typename T>
hipError_t fresh_alloc(T** p, uint64_t n) {
  return hipMalloc(reinterpret_cast<void**>(p), (size_t)n * sizeof(T));
}

// HIP events at the phase boundaries of a timed prune (pv_time_state_store_prune)
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

// pv_state_store_prune; phase_ms (NULL, or 3 floats: mark, scans + copy, rehash of an applied prune)
int prune_impl(int32_t store, const uint8_t* keep_roots, uint64_t n_roots, int apply, uint8_t* root_status,
               uint64_t* n_kept, uint64_t* bytes_kept, uint64_t* n_missing, uint8_t* kept_digests,
               uint64_t digest_cap, float* phase_ms) {
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (n_roots == 0) return fail(PV_EINVAL, "no root to keep (free the store instead)");
  if (!keep_roots) return fail(PV_EINVAL, "null buffer");
  if (n_roots > (1ull << 31)) return fail(PV_EINVAL, "more than 2^31 roots to keep");
  if (const int rc = en.begin()) return rc;
  Device& d = *en.d;
  hipStream_t s = en.s;
  const int mb = merkle_blocks(d);
  const uint64_t n = st->n_nodes, words = (n + 31) / 32;
  TmpBuf<uint8_t> droots, dstatus;
  TmpBuf<uint32_t> bits, queue, ddig;
  TmpBuf<unsigned long long> counts;
  TmpBuf<uint64_t> keep, len;
  FreshStore f;
  PhaseEvents ph;
  StreamDrain tail{s};
  if (phase_ms) HIP_OK(ph.create());
  HIP_OK(ph.mark(0, s));
  // mark: the roots, then one launch per level until a level appends nothing
  HIP_OK(droots.put(keep_roots, n_roots * 32, s));
  HIP_OK(dstatus.alloc(n_roots));
  HIP_OK(bits.alloc(words));
  if (words) HIP_OK(hipMemsetAsync(bits.p, 0, words * 4, s));
  HIP_OK(queue.alloc(st->n_unique));   // an id is enqueued by the lane that flipped its bit: at most once
  HIP_OK(counts.alloc(pv::TP_COUNTS));
  HIP_OK(hipMemsetAsync(counts.p, 0, pv::TP_COUNTS * 8, s));
  const pv::TpCtx c{st->blob, st->beg,  st->end, st->dig,  st->table, st->slots,
                    (uint32_t)n, bits.p, queue.p, counts.p};
  HIP_OK(pv::launch_trie_prune_seed(c, w32(droots.p), n_roots, dstatus.p, mb, s));
  unsigned long long hc[pv::TP_COUNTS] = {0, 0, 0};
  for (uint64_t head = 0;;) {
    HIP_OK(hipMemcpyAsync(hc, counts.p, sizeof hc, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (hc[pv::TP_TAIL] > st->n_unique) return fail(PV_EIO, "state prune: the mark queue overran the store");
    if (hc[pv::TP_TAIL] == head) break;   // each level marks at least one new node, or ends the loop
    HIP_OK(pv::launch_trie_prune_level(c, head, hc[pv::TP_TAIL], mb, s));
    head = hc[pv::TP_TAIL];
  }
  const uint64_t kept = hc[pv::TP_TAIL];
  HIP_OK(ph.mark(1, s));
  std::vector<uint8_t> hstat(n_roots);
  HIP_OK(hipMemcpyAsync(hstat.data(), dstatus.p, n_roots, hipMemcpyDeviceToHost, s));
  // new ids and new byte offsets: two exclusive scans over the keep flags and the kept lengths
  HIP_OK(keep.alloc(n + 1));
  HIP_OK(len.alloc(n + 1));
  HIP_OK(pv::launch_trie_prune_flags(bits.p, st->beg, st->end, n, keep.p, len.p, mb, s));
  HIP_OK(d.scan.ensure(pv::scan_sums_words(n + 1)));
  HIP_OK(pv::launch_exclusive_scan(keep.p, n + 1, d.scan.p, s));
  HIP_OK(pv::launch_exclusive_scan(len.p, n + 1, d.scan.p, s));
  uint64_t bytes = 0;
  HIP_OK(hipMemcpyAsync(&bytes, len.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (root_status) memcpy(root_status, hstat.data(), n_roots);
  if (hc[pv::TP_OVERFLOW])
    return fail(PV_EINVAL, "state prune: inline nodes nest more than %d deep under a stored node", pv::TP_MAX_INLINE);
  if (n_kept) *n_kept = kept;
  if (bytes_kept) *bytes_kept = bytes;
  if (n_missing) *n_missing = hc[pv::TP_MISSING];
  if (apply)
    for (uint64_t i = 0; i < n_roots; ++i)
      if (hstat[i] != PV_SP_OK)
        return fail(PV_EINVAL, "state prune: keep root %llu is not in the store", (unsigned long long)i);
  if (kept_digests && digest_cap < kept)
    return fail(PV_EINVAL, "digest capacity too small: %llu entries for %llu kept nodes",
                (unsigned long long)digest_cap, (unsigned long long)kept);
  if (!apply) {   // the reporting call: the store stays as it is
    if (kept_digests && kept) {
      HIP_OK(ddig.alloc(kept * 8));
      HIP_OK(pv::launch_trie_prune_copy(st->blob, st->beg, st->end, st->dig, bits.p, keep.p, len.p, n, nullptr,
                                        nullptr, nullptr, ddig.p, mb, s));
      HIP_OK(hipMemcpyAsync(kept_digests, ddig.p, kept * 32, hipMemcpyDeviceToHost, s));
    }
    return tail.finish();
  }
  // compact into fresh buffers beside the old ones; the swap is the last step
  const uint64_t cap_nodes = pv::tp_pow2(kept, 1), cap_bytes = pv::tp_pow2(bytes, 1);
  const uint64_t slots = pv::tp_pow2(2 * kept, pv::TS_MIN_SLOTS);   // kept <= n_unique <= 2^30
  HIP_OK(fresh_alloc(&f.blob, cap_bytes + 16));
  HIP_OK(fresh_alloc(&f.beg, cap_nodes));
  HIP_OK(fresh_alloc(&f.end, cap_nodes));
  HIP_OK(fresh_alloc(&f.dig, cap_nodes * 8));
  HIP_OK(fresh_alloc(&f.dup, cap_nodes));
  HIP_OK(fresh_alloc(&f.table, slots));
  HIP_OK(fresh_alloc(&f.unique, 1));
  HIP_OK(pv::launch_trie_prune_copy(st->blob, st->beg, st->end, st->dig, bits.p, keep.p, len.p, n, f.blob, f.beg,
                                    f.end, f.dig, mb, s));
  HIP_OK(hipMemsetAsync(f.blob + bytes, 0, 16, s));
  HIP_OK(ph.mark(2, s));
  HIP_OK(hipMemsetAsync(f.dup, 0, cap_nodes, s));
  HIP_OK(hipMemsetAsync(f.table, 0, slots * 4, s));
  HIP_OK(pv::launch_trie_store_rehash(f.table, (uint32_t)slots, f.dig, f.dup, (uint32_t)kept, mb, s));
  HIP_OK(ph.mark(3, s));
  if (kept_digests && kept) HIP_OK(hipMemcpyAsync(kept_digests, f.dig, kept * 32, hipMemcpyDeviceToHost, s));
  const unsigned int uniq = (unsigned int)kept;
  HIP_OK(hipMemcpyAsync(f.unique, &uniq, 4, hipMemcpyHostToDevice, s));
  if (const int rc = tail.finish()) return rc;
  if (phase_ms)
    for (int i = 0; i < 3; ++i) HIP_OK(hipEventElapsedTime(phase_ms + i, ph.ev[i], ph.ev[i + 1]));
  void* old[] = {st->blob, st->beg, st->end, st->dig, st->dup, st->table, st->unique};
  for (void* p : old)
    if (p) (void)hipFree(p);
  f.taken = true;
  st->blob = f.blob;
  st->beg = f.beg;
  st->end = f.end;
  st->dig = f.dig;
  st->dup = f.dup;
  st->table = f.table;
  st->unique = f.unique;
  st->cap_bytes = cap_bytes;
  st->cap_nodes = cap_nodes;
  st->slots = (uint32_t)slots;
  st->n_nodes = st->n_unique = kept;
  st->n_bytes = bytes;
  return PV_OK;
}

}  // namespace

extern "C" {

int pv_state_store_prune(int32_t store, const uint8_t* keep_roots, uint64_t n_roots, int apply, uint8_t* root_status,
                         uint64_t* n_kept, uint64_t* bytes_kept, uint64_t* n_missing, uint8_t* kept_digests,
                         uint64_t digest_cap) {
  return prune_impl(store, keep_roots, n_roots, apply, root_status, n_kept, bytes_kept, n_missing, kept_digests,
                    digest_cap, nullptr);
}

int pv_time_state_store_prune(int32_t store, const uint8_t* keep_roots, uint64_t n_roots, uint64_t* n_kept,
                              uint64_t* bytes_kept, float* ms_mark, float* ms_compact, float* ms_rehash) {
  if (!ms_mark || !ms_compact || !ms_rehash) return fail(PV_EINVAL, "null pointer");
  float ms[3] = {0, 0, 0};
  const int rc = prune_impl(store, keep_roots, n_roots, 1, nullptr, n_kept, bytes_kept, nullptr, nullptr, 0, ms);
  *ms_mark = ms[0];
  *ms_compact = ms[1];
  *ms_rehash = ms[2];
  return rc;
}

}  // extern "C"

// ------------------------------------------------------- batch trie build
namespace {

// The tail of an add for nodes whose digests are known (pv_state_build with a
// store): copy, k_trie_store_layout, the digests copied instead of a second
// k_sha3_256, then k_trie_store_insert / k_trie_store_rehash as store_add.
// blob / off (off[0] = 0, off[n_new] = total) / dig are device memory.
int store_add_hashed(StateStore& st, Device& d, hipStream_t s, const uint8_t* blob, const uint64_t* off,
                     const uint32_t* dig, uint64_t n_new, uint64_t total) {
  if (n_new == 0) return PV_OK;
  const uint64_t nodes = st.n_nodes + n_new;
  if (const int rc = store_reserve(st, nodes, st.n_bytes + total, s)) return rc;
  if (total) HIP_OK(hipMemcpyAsync(st.blob + st.n_bytes, blob, total, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemsetAsync(st.blob + st.n_bytes + total, 0, 16, s));
  HIP_OK(hipMemsetAsync(st.dup + st.n_nodes, 0, n_new, s));
  HIP_OK(pv::launch_trie_store_layout(off, n_new, st.n_bytes, total, st.beg, st.end, st.n_nodes, merkle_blocks(d), s));
  HIP_OK(hipMemcpyAsync(st.dig + 8 * st.n_nodes, dig, n_new * 32, hipMemcpyDeviceToDevice, s));
  if (nodes > st.slots / 2) {
    uint64_t ns = st.slots;
    while (nodes > ns / 2) ns *= 2;
    if (ns > (1ull << 31)) return fail(PV_ENOMEM, "state store table above 2^31 slots");
    if (const int rc = store_rehash(st, (uint32_t)ns, d, s)) return rc;
  }
  HIP_OK(pv::launch_trie_store_insert(st.table, st.slots, st.dig, st.dup, (uint32_t)st.n_nodes, (uint32_t)n_new,
                                      st.unique, merkle_blocks(d), s));
  unsigned int uniq = 0;
  HIP_OK(hipMemcpyAsync(&uniq, st.unique, 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  st.n_unique = uniq;
  st.n_nodes = nodes;
  st.n_bytes += total;
  return PV_OK;
}

// what k_trie_build_lcp refused: hs[1 .. 3] = the first index for order / value / offsets
int lcp_refusal(const uint32_t* hs) {
  if (hs[3] != 0xffffffffu)
    return fail(PV_EINVAL, "key_off or val_off decreases, or a key is above 2^20 bytes, at index %u", hs[3]);
  if (hs[2] != 0xffffffffu) return fail(PV_EINVAL, "value %u is empty or above 2^30 bytes", hs[2]);
  if (hs[1] != 0xffffffffu)
    return fail(PV_EINVAL, "keys not strictly increasing at index %u (key %u is not above key %u)", hs[1], hs[1],
                hs[1] - 1);
  return PV_OK;
}

// The build over device keys and values (sorted, distinct).  root, n_nodes and
// n_bytes are host memory; node_blob / node_off / digests are host memory with
// host_out, else device memory; st: the store that takes the nodes, or null.
int build_core(Device& d, hipStream_t s, const uint8_t* kb, const uint64_t* ko, const uint8_t* vb, const uint64_t* vo,
               uint64_t n, StateStore* st, uint8_t* root, uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob,
               uint64_t blob_cap, uint64_t* node_off, uint64_t node_cap, uint8_t* digests, bool host_out,
               const uint32_t* knib = nullptr, const uint8_t* kind = nullptr) {
  const hipMemcpyKind out_kind = host_out ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (n_nodes) *n_nodes = 0;
  if (n_bytes) *n_bytes = 0;
  if (n == 0) return PV_OK;   // the entry points return before this
  uint64_t lvoff[pv::TB_MAX_LEVELS + 1];
  pv::TbCtx c{};
  c.key_blob = kb;
  c.key_off = ko;
  c.val_blob = vb;
  c.val_off = vo;
  c.n = n;
  c.knib = knib;   // a merged item list (update_core), else null
  c.kind = kind;
  c.nlv = pv::tb_tree_layout(n, lvoff);
  const uint64_t ents = 3 * n;
  TmpBuf<uint32_t> tree, child, lvl, aux, elen, stats, odig;
  TmpBuf<uint64_t> dlvoff, off, idx, ooff;
  TmpBuf<uint8_t> inl, oblob;
  StreamDrain tail{s};
  HIP_OK(tree.alloc(lvoff[c.nlv]));
  HIP_OK(dlvoff.put(lvoff, pv::TB_MAX_LEVELS + 1, s));
  HIP_OK(child.alloc(16 * n));
  HIP_OK(lvl.alloc(ents));
  HIP_OK(aux.alloc(ents));
  HIP_OK(elen.alloc(ents));
  HIP_OK(off.alloc(ents + 1));
  HIP_OK(idx.alloc(ents + 1));
  HIP_OK(inl.alloc(32 * ents));
  uint32_t hs[5] = {0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0};   // max h, three first-bad indices, the root's entity
  HIP_OK(stats.put(hs, 5, s));
  HIP_OK(hipMemsetAsync(child.p, 0, 16 * n * 4, s));
  HIP_OK(hipMemsetAsync(off.p, 0, (ents + 1) * 8, s));
  HIP_OK(hipMemsetAsync(idx.p, 0, (ents + 1) * 8, s));
  c.tree = tree.p;
  c.lvoff = dlvoff.p;
  c.child = child.p;
  c.lvl = lvl.p;
  c.aux = aux.p;
  c.elen = elen.p;
  c.off = off.p;
  c.idx = idx.p;
  c.inl = inl.p;
  c.root_e = stats.p + 4;
  const int mb = merkle_blocks(d);
  HIP_OK(pv::launch_trie_build_lcp(c, stats.p, mb, s));
  HIP_OK(hipMemcpyAsync(hs, stats.p, 16, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (knib && (hs[1] & hs[2] & hs[3]) != 0xffffffffu)
    return fail(PV_EIO, "trie update: the merged list is not one a build takes (item %u)",
                hs[3] < hs[2] ? (hs[3] < hs[1] ? hs[3] : hs[1]) : (hs[2] < hs[1] ? hs[2] : hs[1]));
  if (const int rc = lcp_refusal(hs)) return rc;
  const uint32_t maxh = hs[0];
  for (uint32_t lv = 1; lv < c.nlv; ++lv) HIP_OK(pv::launch_trie_build_min(c, lv, lvoff[lv + 1] - lvoff[lv], mb, s));
  HIP_OK(pv::launch_trie_build_struct(c, stats.p + 4, mb, s));
  for (uint32_t lv = maxh + 1; lv-- > 0;) HIP_OK(pv::launch_trie_build_size(c, lv, mb, s));
  HIP_OK(d.scan.ensure(pv::scan_sums_words(ents + 1)));
  HIP_OK(pv::launch_exclusive_scan(off.p, ents + 1, d.scan.p, s));
  HIP_OK(pv::launch_exclusive_scan(idx.p, ents + 1, d.scan.p, s));
  uint64_t total = 0, nodes = 0, root_id = 0;
  uint32_t root_e = 0;
  HIP_OK(hipMemcpyAsync(&total, off.p + ents, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&nodes, idx.p + ents, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&root_e, stats.p + 4, 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (root_e >= ents || nodes == 0 || nodes > ents) return fail(PV_EIO, "trie build: inconsistent structure pass");
  HIP_OK(hipMemcpyAsync(&root_id, idx.p + root_e, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (n_nodes) *n_nodes = nodes;
  if (n_bytes) *n_bytes = total;
  if ((node_blob && blob_cap < total) || ((node_off || digests) && node_cap < nodes))
    return fail(PV_EINVAL, "node capacity too small: the build has %llu nodes of %llu bytes", (unsigned long long)nodes,
                (unsigned long long)total);
  if (st && (nodes > pv::TS_MAX_NODES || st->n_nodes + nodes > pv::TS_MAX_NODES))
    return fail(PV_EINVAL, "state store limited to 2^32 - 2 nodes");
  HIP_OK(oblob.alloc(total + 16));
  HIP_OK(ooff.alloc(nodes + 1));
  HIP_OK(odig.alloc(8 * nodes));
  HIP_OK(hipMemsetAsync(oblob.p + total, 0, 16, s));
  c.out_blob = oblob.p;
  c.node_off = ooff.p;
  c.dig = odig.p;
  for (uint32_t lv = maxh + 1; lv-- > 0;) HIP_OK(pv::launch_trie_build_emit(c, lv, mb, s));
  HIP_OK(hipMemcpyAsync(ooff.p + nodes, off.p + ents, 8, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(root, odig.p + 8 * root_id, 32, hipMemcpyDeviceToHost, s));
  if (node_blob && total) HIP_OK(hipMemcpyAsync(node_blob, oblob.p, total, out_kind, s));
  if (node_off) HIP_OK(hipMemcpyAsync(node_off, ooff.p, (nodes + 1) * 8, out_kind, s));
  if (digests) HIP_OK(hipMemcpyAsync(digests, odig.p, nodes * 32, out_kind, s));
  if (st)
    if (const int rc = store_add_hashed(*st, d, s, oblob.p, ooff.p, odig.p, nodes, total)) return rc;
  return tail.finish();
}

const uint8_t kBlankRoot[32] = {0xbc, 0x20, 0x71, 0xa4, 0xde, 0x84, 0x6f, 0x28, 0x57, 0x02, 0x44,
                                0x7f, 0x25, 0x89, 0xdd, 0x16, 0x36, 0x78, 0xe0, 0x97, 0x2a, 0x8a,
                                0x1b, 0x0d, 0x28, 0xb0, 0x4e, 0xd5, 0xc0, 0x94, 0x54, 0x7f};   // SHA3-256(0x80)

// The empty batch: the blank root, no nodes.  Every output that is given is
// written; nothing is launched for the build and nothing is inserted, so the
// store is not looked at.
int build_empty(Entry& en, void* stream, uint8_t* root, uint64_t* n_nodes, uint64_t* n_bytes, uint64_t* node_off,
                bool host_out) {
  if (root) memcpy(root, kBlankRoot, 32);
  if (n_nodes) *n_nodes = 0;
  if (n_bytes) *n_bytes = 0;
  if (!node_off) return PV_OK;
  if (host_out) {
    node_off[0] = 0;
    return PV_OK;
  }
  if (const int rc = en.begin(stream)) return rc;
  HIP_OK(hipMemsetAsync(node_off, 0, 8, en.s));
  return en.finish();
}

// key a before key b: bytewise, a proper prefix first
bool key_less(const uint8_t* blob, const uint64_t* off, uint64_t a, uint64_t b, bool* equal) {
  const uint64_t la = off[a + 1] - off[a], lb = off[b + 1] - off[b];
  const uint64_t m = la < lb ? la : lb;
  const int c = m ? memcmp(blob + off[a], blob + off[b], m) : 0;
  *equal = c == 0 && la == lb;
  return c < 0 || (c == 0 && la < lb);
}

// The host forms' input: the checks of the arrays, then the pairs sorted with
// the last of equal keys kept, as blobs with 16 spare bytes and offsets from 0.
int sorted_pairs(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob, const uint64_t* val_off,
                 uint64_t n, std::vector<uint64_t>& ko, std::vector<uint64_t>& vo, std::vector<uint8_t>& kb,
                 std::vector<uint8_t>& vb, bool empty_ok = false) {
  if (!key_off || !val_off || (!val_blob && !empty_ok)) return fail(PV_EINVAL, "null buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  Ragged keys(key_off, n), vals(val_off, n);
  if (const int rc = keys.check("key_off")) return rc;
  if (const int rc = vals.check("val_off")) return rc;
  if ((keys.len && !key_blob) || (vals.len && !val_blob))   // a batch of removals alone has no value byte
    return fail(PV_EINVAL, "null buffer");
  for (uint64_t i = 0; i < n; ++i) {
    if (val_off[i + 1] == val_off[i] && !empty_ok)   // pv_state_apply: a removal
      return fail(PV_EINVAL, "value %llu is empty", (unsigned long long)i);
    if (key_off[i + 1] - key_off[i] > pv::TB_MAX_KEY_BYTES || val_off[i + 1] - val_off[i] > pv::TB_MAX_VAL_BYTES)
      return fail(PV_EINVAL, "pair %llu: a key above 2^20 or a value above 2^30 bytes", (unsigned long long)i);
  }
  // sorted index; of equal keys the last occurrence stays
  std::vector<uint64_t> order(n), pick;
  for (uint64_t i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
    bool eq;
    return key_less(key_blob, key_off, a, b, &eq);
  });
  for (uint64_t k = 0; k < n; ++k) {
    bool eq = false;
    if (k + 1 < n) (void)key_less(key_blob, key_off, order[k], order[k + 1], &eq);
    if (!eq) pick.push_back(order[k]);
  }
  const uint64_t m = pick.size();
  ko.assign(m + 1, 0);
  vo.assign(m + 1, 0);
  for (uint64_t k = 0; k < m; ++k) {
    ko[k + 1] = ko[k] + (key_off[pick[k] + 1] - key_off[pick[k]]);
    vo[k + 1] = vo[k] + (val_off[pick[k] + 1] - val_off[pick[k]]);
  }
  kb.assign(ko[m] + 16, 0);
  vb.assign(vo[m] + 16, 0);
  for (uint64_t k = 0; k < m; ++k) {
    if (ko[k + 1] > ko[k]) memcpy(&kb[ko[k]], key_blob + key_off[pick[k]], ko[k + 1] - ko[k]);
    if (vo[k + 1] > vo[k]) memcpy(&vb[vo[k]], val_blob + val_off[pick[k]], vo[k + 1] - vo[k]);
  }
  return PV_OK;
}

// ------------------------------------------- the device sort (pv_trie_sort.h)
// what k_trie_sort_init refused: hs[0 .. 2] = the first input index for offsets / key length / value
int sort_refusal(const uint32_t* hs) {
  if (hs[0] != 0xffffffffu) return fail(PV_EINVAL, "key_off or val_off decreases at index %u", hs[0]);
  if (hs[1] != 0xffffffffu)
    return fail(PV_EINVAL,
                "key %u is above 1024 bytes: the device sort takes keys up to 1024 bytes, the host forms "
                "(pv_state_build, pv_state_update, pv_state_apply) sort keys of any length",
                hs[1]);
  if (hs[2] != 0xffffffffu) return fail(PV_EINVAL, "value %u is empty or above 2^30 bytes", hs[2]);
  return PV_OK;
}

// perm[0 .. *kept) = the input indices of the distinct keys in order, the last of equal keys kept
// (device memory, n entries); val_off: checked with the keys when given (the fused forms).  Nothing
// is written to perm when the first kernel refuses.  *rounds: the rounds run.  Ends synchronised.
int sort_core(Device& d, hipStream_t s, const uint8_t* kb, const uint64_t* ko, const uint64_t* vo, bool empty_ok,
              uint64_t n, uint32_t* perm, uint64_t* kept, uint32_t* rounds = nullptr) {
  const int mb = merkle_blocks(d);
  const uint64_t table_words = 256 * pv::trie_sort_blocks(n);
  TmpBuf<pv::TsRec> ra, rb;
  TmpBuf<uint64_t> x, table;
  TmpBuf<uint32_t> stats;
  StreamDrain tail{s};
  HIP_OK(ra.alloc(n));
  HIP_OK(rb.alloc(n));
  HIP_OK(x.alloc(n + 1));
  HIP_OK(table.alloc(table_words));
  uint32_t hs[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
  HIP_OK(stats.put(hs, 3, s));
  HIP_OK(d.scan.ensure(pv::scan_sums_words(table_words > n + 1 ? table_words : n + 1)));
  HIP_OK(pv::launch_trie_sort_init(kb, ko, vo, empty_ok, n, ra.p, stats.p, mb, s));
  HIP_OK(hipMemcpyAsync(hs, stats.p, 12, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (const int rc = sort_refusal(hs)) return rc;
  pv::TsRec *cur = ra.p, *other = rb.p;
  uint64_t runs = 1;
  uint32_t r = 0;
  for (;; ++r) {
    if (r >= pv::TS_MAX_ROUNDS) return fail(PV_EIO, "device sort: keys unresolved after %u rounds", r);
    if (r > 0) {   // the segment of round r is the run's rank after round r - 1
      HIP_OK(pv::launch_trie_sort_round(kb, ko, cur, x.p, n, r, other, mb, s));
      std::swap(cur, other);
    }
    const uint32_t passes = 9 + (r > 0 ? pv::ts_seg_digits(runs) : 0);
    for (uint32_t p = 0; p < passes; ++p) {
      HIP_OK(pv::launch_trie_sort_pass(cur, n, p, table.p, d.scan.p, other, s));
      std::swap(cur, other);
    }
    HIP_OK(pv::launch_trie_sort_flags(cur, n, x.p, mb, s));
    HIP_OK(pv::launch_exclusive_scan(x.p, n + 1, d.scan.p, s));
    uint64_t totals = 0;   // unresolved << 32 | runs
    HIP_OK(hipMemcpyAsync(&totals, x.p + n, 8, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    runs = totals & 0xffffffffull;
    if (runs == 0 || runs > n) return fail(PV_EIO, "device sort: inconsistent flag pass");
    if ((totals >> 32) == 0) break;
  }
  HIP_OK(pv::launch_trie_sort_finish(cur, x.p, n, perm, mb, s));
  *kept = runs;
  if (rounds) *rounds = r + 1;
  return tail.finish();
}

// The fused forms' input: device pairs in any order -> the pairs sorted with the last of equal
// keys kept, as blobs with 16 spare bytes and offsets from 0 (what sorted_pairs gives the host forms).
struct DevicePairs {
  TmpBuf<uint8_t> kb, vb;
  TmpBuf<uint64_t> ko, vo;
  uint64_t m = 0;
};

int sort_pairs_device(Device& d, hipStream_t s, const uint8_t* kb, const uint64_t* ko, const uint8_t* vb,
                      const uint64_t* vo, uint64_t n, bool empty_ok, DevicePairs& out, uint32_t* rounds = nullptr,
                      hipEvent_t sorted = nullptr) {
  const int mb = merkle_blocks(d);
  TmpBuf<uint32_t> perm;
  StreamDrain tail{s};
  HIP_OK(perm.alloc(n));
  if (const int rc = sort_core(d, s, kb, ko, vo, empty_ok, n, perm.p, &out.m, rounds)) return rc;
  if (sorted) HIP_OK(hipEventRecord(sorted, s));   // pv_time_state_sort_device: the sort ends, the gather begins
  const uint64_t m = out.m;
  HIP_OK(out.ko.alloc(m + 1));
  HIP_OK(out.vo.alloc(m + 1));
  HIP_OK(pv::launch_trie_sort_lens(perm.p, m, n, ko, vo, out.ko.p, out.vo.p, mb, s));
  HIP_OK(d.scan.ensure(pv::scan_sums_words(m + 1)));
  HIP_OK(pv::launch_exclusive_scan(out.ko.p, m + 1, d.scan.p, s));
  HIP_OK(pv::launch_exclusive_scan(out.vo.p, m + 1, d.scan.p, s));
  uint64_t kbytes = 0, vbytes = 0;
  HIP_OK(hipMemcpyAsync(&kbytes, out.ko.p + m, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&vbytes, out.vo.p + m, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  HIP_OK(out.kb.alloc(kbytes + 16));
  HIP_OK(out.vb.alloc(vbytes + 16));
  HIP_OK(hipMemsetAsync(out.kb.p + kbytes, 0, 16, s));
  HIP_OK(hipMemsetAsync(out.vb.p + vbytes, 0, 16, s));
  HIP_OK(pv::launch_trie_sort_copy(perm.p, m, n, kb, ko, vb, vo, out.ko.p, out.vo.p, out.kb.p, out.vb.p, mb, s));
  return tail.finish();
}

// The build's first kernel checks the order again.  After the device sort that refusal is a bug
// in the sort, not in the caller's input: it is reported as one, and nothing is retried.
int sort_selfcheck(int rc) {
  if (rc == PV_EINVAL && g_err.compare(0, 28, "keys not strictly increasing") == 0) {
    const std::string was = g_err;
    return fail(PV_EIO, "device sort: a bug in the sort, its output was refused by the build (%s)", was.c_str());
  }
  return rc;
}

}  // namespace

extern "C" {

// The permutation that sorts state keys: bytewise, a proper prefix first, the last of equal keys
// kept (csrc/pv_trie_sort.h); see include/plenum_verify.h.
int pv_state_sort_device(const uint8_t* key_blob, const uint64_t* key_off, uint64_t n, uint32_t* perm,
                         uint64_t* n_kept, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) {
    if (n_kept) *n_kept = 0;
    return PV_OK;
  }
  if (!n_kept) return fail(PV_EINVAL, "null pointer");
  if (!key_blob || !key_off || !perm) return fail(PV_EINVAL, "null device buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  if (reinterpret_cast<uintptr_t>(key_blob) & 3u) return fail(PV_EINVAL, "key_blob must be 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  *n_kept = 0;
  return sort_core(*en.d, en.s, key_blob, key_off, nullptr, true, n, perm, n_kept);
}

// pv_state_build_device over pairs in any order, the last of equal keys winning: the device sort,
// the gather, then the same build; see include/plenum_verify.h.
int pv_state_build_unsorted_device(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob,
                                   const uint64_t* val_off, uint64_t n, int32_t store, uint8_t* root,
                                   uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap,
                                   uint64_t* node_off, uint64_t node_cap, uint8_t* digests, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return build_empty(en, stream, root, n_nodes, n_bytes, node_off, false);
  if (!root) return fail(PV_EINVAL, "null pointer");
  if (!key_blob || !key_off || !val_blob || !val_off) return fail(PV_EINVAL, "null device buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  if ((reinterpret_cast<uintptr_t>(key_blob) & 3u) || (reinterpret_cast<uintptr_t>(val_blob) & 3u))
    return fail(PV_EINVAL, "key_blob and val_blob must be 4-byte aligned");
  if (digests && misaligned16(digests)) return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  StateStore* st = nullptr;
  if (store != -1) {
    st = find_store(store);
    if (!st) return fail(PV_EINVAL, "no state store with id %d", (int)store);
    if (st->dev != en.d->id)
      return fail(PV_EINVAL, "state store %d lives on device %d, not on device %d", (int)store, st->dev, device);
  }
  if (const int rc = en.begin(stream)) return rc;
  if (n_nodes) *n_nodes = 0;
  if (n_bytes) *n_bytes = 0;
  DevicePairs sp;
  StreamDrain tail{en.s};
  if (const int rc = sort_pairs_device(*en.d, en.s, key_blob, key_off, val_blob, val_off, n, false, sp)) return rc;
  return sort_selfcheck(build_core(*en.d, en.s, sp.kb.p, sp.ko.p, sp.vb.p, sp.vo.p, sp.m, st, root, n_nodes, n_bytes,
                                   node_blob, blob_cap, node_off, node_cap, digests, false));
}

// The sort and the gather of the fused forms alone, each timed with HIP events on the call's
// stream (tools/bench_state_sort.py); see include/plenum_verify.h.
int pv_time_state_sort_device(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob,
                              const uint64_t* val_off, uint64_t n, int device, void* stream, uint64_t* n_kept,
                              uint32_t* rounds, float* ms_sort, float* ms_gather) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (!n_kept || !rounds || !ms_sort || !ms_gather) return n == 0 ? PV_OK : fail(PV_EINVAL, "null pointer");
  *n_kept = 0;
  *rounds = 0;
  *ms_sort = *ms_gather = 0;
  if (n == 0) return PV_OK;
  if (!key_blob || !key_off || !val_blob || !val_off) return fail(PV_EINVAL, "null device buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  if ((reinterpret_cast<uintptr_t>(key_blob) & 3u) || (reinterpret_cast<uintptr_t>(val_blob) & 3u))
    return fail(PV_EINVAL, "key_blob and val_blob must be 4-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  PhaseEvents ev;
  HIP_OK(ev.create());
  DevicePairs sp;
  StreamDrain tail{en.s};
  HIP_OK(ev.mark(0, en.s));
  if (const int rc = sort_pairs_device(*en.d, en.s, key_blob, key_off, val_blob, val_off, n, true, sp, rounds, ev.ev[1]))
    return rc;
  HIP_OK(ev.mark(2, en.s));
  HIP_OK(hipEventSynchronize(ev.ev[2]));
  HIP_OK(hipEventElapsedTime(ms_sort, ev.ev[0], ev.ev[1]));
  HIP_OK(hipEventElapsedTime(ms_gather, ev.ev[1], ev.ev[2]));
  *n_kept = sp.m;
  return tail.finish();
}

// PruningState.set per pair and headHash (state/pruning_state.py:60-61, 136; Trie.update,
// state/trie/pruning_trie.py:1006-1027) as one batch; see include/plenum_verify.h.
int pv_state_build_device(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob,
                          const uint64_t* val_off, uint64_t n, int32_t store, uint8_t* root, uint64_t* n_nodes,
                          uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                          uint64_t node_cap, uint8_t* digests, int device, void* stream) {
  Entry en(device);
  if (const int rc = en.check()) return rc;
  if (n == 0) return build_empty(en, stream, root, n_nodes, n_bytes, node_off, false);
  if (!root) return fail(PV_EINVAL, "null pointer");
  if (!key_blob || !key_off || !val_blob || !val_off) return fail(PV_EINVAL, "null device buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  if ((reinterpret_cast<uintptr_t>(key_blob) & 3u) || (reinterpret_cast<uintptr_t>(val_blob) & 3u))
    return fail(PV_EINVAL, "key_blob and val_blob must be 4-byte aligned");
  if (digests && misaligned16(digests)) return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  StateStore* st = nullptr;
  if (store != -1) {
    st = find_store(store);
    if (!st) return fail(PV_EINVAL, "no state store with id %d", (int)store);
    if (st->dev != en.d->id)
      return fail(PV_EINVAL, "state store %d lives on device %d, not on device %d", (int)store, st->dev, device);
  }
  if (const int rc = en.begin(stream)) return rc;
  return build_core(*en.d, en.s, key_blob, key_off, val_blob, val_off, n, st, root, n_nodes, n_bytes, node_blob,
                    blob_cap, node_off, node_cap, digests, false);
}

// The host form of the same (state/pruning_state.py:60-61; state/trie/pruning_trie.py:1006-1027):
// keys in any order, the last of equal keys wins, as a sequence of sets gives.
int pv_state_build(const uint8_t* key_blob, const uint64_t* key_off, const uint8_t* val_blob, const uint64_t* val_off,
                   uint64_t n, int32_t store, uint8_t* root, uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob,
                   uint64_t blob_cap, uint64_t* node_off, uint64_t node_cap, uint8_t* digests) {
  if (n == 0) {
    Entry en;
    if (const int rc = en.check()) return rc;
    return build_empty(en, nullptr, root, n_nodes, n_bytes, node_off, true);
  }
  // The argument checks and the sorted copy touch no library state: they run
  // before the library lock is taken, so a large sort blocks no other call.
  if (!root) return fail(PV_EINVAL, "null pointer");
  std::vector<uint64_t> ko, vo;
  std::vector<uint8_t> kb, vb;
  if (const int rc = sorted_pairs(key_blob, key_off, val_blob, val_off, n, ko, vo, kb, vb)) return rc;
  const uint64_t m = ko.size() - 1;
  Entry en;
  if (const int rc = en.check()) return rc;
  StateStore* st = nullptr;
  if (store != -1)
    if (const int rc = store_enter(en, store, &st)) return rc;
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dkb, dvb;
  TmpBuf<uint64_t> dko, dvo;
  StreamDrain tail{s};
  HIP_OK(dkb.put(kb.data(), kb.size(), s));
  HIP_OK(dvb.put(vb.data(), vb.size(), s));
  HIP_OK(dko.put(ko.data(), m + 1, s));
  HIP_OK(dvo.put(vo.data(), m + 1, s));
  return build_core(*en.d, s, dkb.p, dko.p, dvb.p, dvo.p, m, st, root, n_nodes, n_bytes, node_blob, blob_cap, node_off,
                    node_cap, digests, true);
}

}  // extern "C"

// ------------------------------------------- sets onto a committed root
namespace {

// No item left: the blank root and no node (the outputs of build_empty, on the call's stream).
int nothing_left(hipStream_t s, uint8_t* root, uint64_t* n_nodes, uint64_t* n_bytes, uint64_t* node_off, bool host_out) {
  memcpy(root, kBlankRoot, 32);
  if (n_nodes) *n_nodes = 0;
  if (n_bytes) *n_bytes = 0;
  if (node_off) {
    if (host_out) node_off[0] = 0;
    else HIP_OK(hipMemsetAsync(node_off, 0, 8, s));
  }
  HIP_OK(hipStreamSynchronize(s));
  return PV_OK;
}

// A batch with removals onto the blank root: the removals are dropped and the rest is a build.
// The batch has passed tb_lcp_one, so its offsets are monotone and bounded.  Not a hot path (a
// ledger's first batch): the pairs are compacted on the host.
int build_without_removals(Device& d, hipStream_t s, const uint8_t* kb, const uint64_t* ko, const uint8_t* vb,
                           const uint64_t* vo, uint64_t n, StateStore* st, uint8_t* root, uint64_t* n_nodes,
                           uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                           uint64_t node_cap, uint8_t* digests, bool host_out) {
  std::vector<uint64_t> hko(n + 1), hvo(n + 1);
  HIP_OK(hipMemcpyAsync(hko.data(), ko, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(hvo.data(), vo, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  uint64_t kept = 0;
  for (uint64_t i = 0; i < n; ++i) kept += hvo[i + 1] > hvo[i];
  if (kept == n)
    return build_core(d, s, kb, ko, vb, vo, n, st, root, n_nodes, n_bytes, node_blob, blob_cap, node_off, node_cap,
                      digests, host_out);
  if (kept == 0) return nothing_left(s, root, n_nodes, n_bytes, node_off, host_out);
  std::vector<uint8_t> hk(hko[n] - hko[0]), hv(hvo[n] - hvo[0]);
  if (!hk.empty()) HIP_OK(hipMemcpyAsync(hk.data(), kb + hko[0], hk.size(), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(hv.data(), vb + hvo[0], hv.size(), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  std::vector<uint64_t> cko(kept + 1, 0), cvo(kept + 1, 0);
  std::vector<uint8_t> ck, cv;
  uint64_t k = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (hvo[i + 1] == hvo[i]) continue;
    ck.insert(ck.end(), hk.begin() + (hko[i] - hko[0]), hk.begin() + (hko[i + 1] - hko[0]));
    cv.insert(cv.end(), hv.begin() + (hvo[i] - hvo[0]), hv.begin() + (hvo[i + 1] - hvo[0]));
    ++k;
    cko[k] = ck.size();
    cvo[k] = cv.size();
  }
  ck.resize(ck.size() + 16, 0);
  cv.resize(cv.size() + 16, 0);
  TmpBuf<uint8_t> dkb, dvb;
  TmpBuf<uint64_t> dko, dvo;
  StreamDrain tail{s};
  HIP_OK(dkb.put(ck.data(), ck.size(), s));
  HIP_OK(dvb.put(cv.data(), cv.size(), s));
  HIP_OK(dko.put(cko.data(), kept + 1, s));
  HIP_OK(dvo.put(cvo.data(), kept + 1, s));
  return build_core(d, s, dkb.p, dko.p, dvb.p, dvo.p, kept, st, root, n_nodes, n_bytes, node_blob, blob_cap, node_off,
                    node_cap, digests, host_out);
}

// The update over device keys and values (sorted, distinct): the merge of
// pv_trie_update.h, then build_core over the merged items.  old_root, root,
// n_nodes and n_bytes are host memory; the node outputs as build_core's.
// removals (pv_state_apply): an empty value removes its key.
int update_core(Device& d, hipStream_t s, StateStore& st, const uint8_t* old_root, const uint8_t* kb,
                const uint64_t* ko, const uint8_t* vb, const uint64_t* vo, uint64_t n, bool insert, uint8_t* root,
                uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                uint64_t node_cap, uint8_t* digests, bool host_out, bool removals = false) {
  const bool blank = memcmp(old_root, kBlankRoot, 32) == 0;
  if (blank && !removals)   // nothing to merge with: the store is not read
    return build_core(d, s, kb, ko, vb, vo, n, insert ? &st : nullptr, root, n_nodes, n_bytes, node_blob, blob_cap,
                      node_off, node_cap, digests, host_out);
  const char* const what = removals ? "state apply" : "state update";
  if (n_nodes) *n_nodes = 0;
  if (n_bytes) *n_bytes = 0;
  const int mb = merkle_blocks(d);
  TmpBuf<uint32_t> h, stats, droot, inib;
  TmpBuf<uint64_t> sizes, ikoff, ivoff;
  TmpBuf<uint8_t> status, ikey, ival, ikind;
  StreamDrain tail{s};
  // the batch's own checks and h[], by the build's first kernel: the same refusals
  pv::TbCtx b{};
  b.key_blob = kb;
  b.key_off = ko;
  b.val_blob = vb;
  b.val_off = vo;
  b.n = n;
  HIP_OK(h.alloc(n + 1));
  b.tree = h.p;
  uint32_t hs[5] = {0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0};   // hs[4]: the batch holds a removal
  HIP_OK(stats.put(hs, 5, s));
  if (removals) b.empty_seen = stats.p + 4;
  HIP_OK(pv::launch_trie_build_lcp(b, stats.p, mb, s));
  HIP_OK(hipMemcpyAsync(hs, stats.p, 20, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (const int rc = lcp_refusal(hs)) return rc;
  // a batch without a removal is a batch of sets: it takes the walk without the removal mode
  const bool opening = removals && hs[4] != 0;
  if (blank)
    return build_without_removals(d, s, kb, ko, vb, vo, n, insert ? &st : nullptr, root, n_nodes, n_bytes, node_blob,
                                  blob_cap, node_off, node_cap, digests, host_out);
  // count, scan, write
  pv::TuCtx c{};
  c.blob = st.blob;
  c.beg = st.beg;
  c.end = st.end;
  c.dig = st.dig;
  c.table = st.table;
  c.slots = st.slots;
  c.n_nodes = (uint32_t)st.n_nodes;
  uint32_t rw[8];
  memcpy(rw, old_root, 32);
  HIP_OK(droot.put(rw, 8, s));
  c.root = droot.p;
  c.key_blob = kb;
  c.key_off = ko;
  c.val_blob = vb;
  c.val_off = vo;
  c.n = n;
  c.h = h.p;
  HIP_OK(sizes.alloc(3 * (n + 1)));
  HIP_OK(hipMemsetAsync(sizes.p, 0, 3 * (n + 1) * 8, s));
  c.cnt = sizes.p;
  c.pbytes = sizes.p + (n + 1);
  c.vbytes = sizes.p + 2 * (n + 1);
  HIP_OK(status.alloc(n));
  c.status = status.p;
  HIP_OK(opening ? pv::launch_trie_apply_count(c, mb, s) : pv::launch_trie_update_count(c, mb, s));
  std::vector<uint8_t> hstat(n);
  HIP_OK(hipMemcpyAsync(hstat.data(), status.p, n, hipMemcpyDeviceToHost, s));
  HIP_OK(d.scan.ensure(pv::scan_sums_words(n + 1)));
  HIP_OK(pv::launch_exclusive_scan(c.cnt, n + 1, d.scan.p, s));
  HIP_OK(pv::launch_exclusive_scan(c.pbytes, n + 1, d.scan.p, s));
  HIP_OK(pv::launch_exclusive_scan(c.vbytes, n + 1, d.scan.p, s));
  uint64_t tot[3] = {0, 0, 0};   // items, path bytes, payload bytes
  for (int k = 0; k < 3; ++k)
    HIP_OK(hipMemcpyAsync(&tot[k], sizes.p + k * (n + 1) + n, 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  for (uint64_t j = 0; j < n; ++j)
    if (hstat[j] != pv::SP_OK)
      return fail(PV_EINVAL,
                  hstat[j] == pv::SP_NODE_MISSING
                      ? "%s: key %llu: the root or a node on its path is not in the store (status %u)"
                      : "%s: key %llu: a node on its path is not a well-formed trie node (status %u)",
                  what, (unsigned long long)j, (unsigned)hstat[j]);
  if ((!removals && tot[0] < n) || tot[0] > pv::TB_MAX_KEYS)
    return fail(PV_EINVAL, "%s: %llu merged items, above the 2^28 of one build", what, (unsigned long long)tot[0]);
  const uint64_t items = tot[0];
  if (items == 0) {   // every key of the state removed: no build launch
    tail.done = true;
    return nothing_left(s, root, n_nodes, n_bytes, node_off, host_out);
  }
  HIP_OK(ikey.alloc(tot[1] + 16));
  HIP_OK(ival.alloc(tot[2] + 16));
  HIP_OK(ikoff.alloc(items + 1));
  HIP_OK(ivoff.alloc(items + 1));
  HIP_OK(inib.alloc(items));
  HIP_OK(ikind.alloc(items));
  HIP_OK(hipMemsetAsync(ikey.p + tot[1], 0, 16, s));
  HIP_OK(hipMemsetAsync(ival.p + tot[2], 0, 16, s));
  HIP_OK(hipMemcpyAsync(ikoff.p + items, c.pbytes + n, 8, hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemcpyAsync(ivoff.p + items, c.vbytes + n, 8, hipMemcpyDeviceToDevice, s));
  c.ikey = ikey.p;
  c.ikoff = ikoff.p;
  c.ival = ival.p;
  c.ivoff = ivoff.p;
  c.inib = inib.p;
  c.ikind = ikind.p;
  HIP_OK(opening ? pv::launch_trie_apply_emit(c, mb, s) : pv::launch_trie_update_emit(c, mb, s));
  return build_core(d, s, ikey.p, ikoff.p, ival.p, ivoff.p, items, insert ? &st : nullptr, root, n_nodes, n_bytes,
                    node_blob, blob_cap, node_off, node_cap, digests, host_out, inib.p, ikind.p);
}

// n == 0: the root stays, no node, no launch for the update; every output that is given is
// written, and, as with the empty build, neither the store nor an input buffer is looked at
int update_empty(Entry& en, void* stream, const uint8_t* old_root, uint8_t* new_root, uint64_t* n_nodes,
                 uint64_t* n_bytes, uint64_t* node_off, bool host_out) {
  if (new_root && old_root) memcpy(new_root, old_root, 32);
  return build_empty(en, stream, nullptr, n_nodes, n_bytes, node_off, host_out);
}

// pv_state_update_device / pv_state_apply_device: device buffers, strictly increasing keys
int update_device_entry(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                        const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* new_root,
                        uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                        uint64_t node_cap, uint8_t* digests, void* stream, bool removals, bool unsorted = false) {
  Entry en;
  if (n == 0) {   // as the empty build: nothing is looked at, the store included
    if (const int rc = en.check()) return rc;
    return update_empty(en, stream, old_root, new_root, n_nodes, n_bytes, node_off, false);
  }
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (!old_root || !new_root) return fail(PV_EINVAL, "null pointer");
  if (!key_blob || !key_off || !val_blob || !val_off) return fail(PV_EINVAL, "null device buffer");
  if (n > pv::TB_MAX_KEYS) return fail(PV_EINVAL, "more than 2^28 keys in one build");
  if ((reinterpret_cast<uintptr_t>(key_blob) & 3u) || (reinterpret_cast<uintptr_t>(val_blob) & 3u))
    return fail(PV_EINVAL, "key_blob and val_blob must be 4-byte aligned");
  if (digests && misaligned16(digests)) return fail(PV_EINVAL, "digest buffers must be 16-byte aligned");
  if (const int rc = en.begin(stream)) return rc;
  if (unsorted) {   // pv_state_apply_unsorted_device: the device sort and the gather first
    if (n_nodes) *n_nodes = 0;
    if (n_bytes) *n_bytes = 0;
    DevicePairs sp;
    StreamDrain tail{en.s};
    if (const int rc = sort_pairs_device(*en.d, en.s, key_blob, key_off, val_blob, val_off, n, removals, sp)) return rc;
    return sort_selfcheck(update_core(*en.d, en.s, *st, old_root, sp.kb.p, sp.ko.p, sp.vb.p, sp.vo.p, sp.m, insert != 0,
                                      new_root, n_nodes, n_bytes, node_blob, blob_cap, node_off, node_cap, digests,
                                      false, removals));
  }
  return update_core(*en.d, en.s, *st, old_root, key_blob, key_off, val_blob, val_off, n, insert != 0, new_root,
                     n_nodes, n_bytes, node_blob, blob_cap, node_off, node_cap, digests, false, removals);
}

// pv_state_update / pv_state_apply: host buffers, keys in any order, the last of equal keys wins
int update_host_entry(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                      const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* new_root,
                      uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                      uint64_t node_cap, uint8_t* digests, bool removals) {
  if (n == 0) {
    Entry en;
    if (const int rc = en.check()) return rc;
    return update_empty(en, nullptr, old_root, new_root, n_nodes, n_bytes, node_off, true);
  }
  // checks and the sorted copy before the library lock, as pv_state_build
  if (!old_root || !new_root) return fail(PV_EINVAL, "null pointer");
  std::vector<uint64_t> ko, vo;
  std::vector<uint8_t> kb, vb;
  if (const int rc = sorted_pairs(key_blob, key_off, val_blob, val_off, n, ko, vo, kb, vb, removals)) return rc;
  const uint64_t m = ko.size() - 1;
  Entry en;
  StateStore* st;
  if (const int rc = store_enter(en, store, &st)) return rc;
  if (const int rc = en.begin()) return rc;
  hipStream_t s = en.s;
  TmpBuf<uint8_t> dkb, dvb;
  TmpBuf<uint64_t> dko, dvo;
  StreamDrain tail{s};
  HIP_OK(dkb.put(kb.data(), kb.size(), s));
  HIP_OK(dvb.put(vb.data(), vb.size(), s));
  HIP_OK(dko.put(ko.data(), m + 1, s));
  HIP_OK(dvo.put(vo.data(), m + 1, s));
  return update_core(*en.d, s, *st, old_root, dkb.p, dko.p, dvb.p, dvo.p, m, insert != 0, new_root, n_nodes, n_bytes,
                     node_blob, blob_cap, node_off, node_cap, digests, true, removals);
}

}  // namespace

extern "C" {

// A 3PC batch of PruningState.set onto the state at a committed root, and the new headHash
// (state/pruning_state.py:60-61, 136; Trie.update, state/trie/pruning_trie.py:1006-1027), as one
// batch over device buffers; see include/plenum_verify.h.
int pv_state_update_device(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                           const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert,
                           uint8_t* new_root, uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob,
                           uint64_t blob_cap, uint64_t* node_off, uint64_t node_cap, uint8_t* digests, void* stream) {
  return update_device_entry(store, old_root, key_blob, key_off, val_blob, val_off, n, insert, new_root, n_nodes,
                             n_bytes, node_blob, blob_cap, node_off, node_cap, digests, stream, false);
}

// The host form of the same (state/pruning_state.py:60-61; state/trie/pruning_trie.py:1006-1027):
// keys in any order, the last of equal keys wins, as a sequence of sets gives.
int pv_state_update(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                    const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* new_root,
                    uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                    uint64_t node_cap, uint8_t* digests) {
  return update_host_entry(store, old_root, key_blob, key_off, val_blob, val_off, n, insert, new_root, n_nodes,
                           n_bytes, node_blob, blob_cap, node_off, node_cap, digests, false);
}

// A 3PC batch of PruningState.set and PruningState.remove onto the state at a committed root, and
// the new headHash (state/pruning_state.py:60-61, 84-85, 136; Trie.update and Trie.delete,
// state/trie/pruning_trie.py:1006-1027, 683-848), as one batch over device buffers: an empty
// value removes its key; see include/plenum_verify.h.
int pv_state_apply_device(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                          const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* new_root,
                          uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap,
                          uint64_t* node_off, uint64_t node_cap, uint8_t* digests, void* stream) {
  return update_device_entry(store, old_root, key_blob, key_off, val_blob, val_off, n, insert, new_root, n_nodes,
                             n_bytes, node_blob, blob_cap, node_off, node_cap, digests, stream, true);
}

// pv_state_apply_device over pairs in any order, the last of equal keys winning (a later removal
// over an earlier set as a later set over an earlier removal): the device sort, the gather, then
// the same apply; see include/plenum_verify.h.
int pv_state_apply_unsorted_device(int32_t store, const uint8_t* old_root, const uint8_t* key_blob,
                                   const uint64_t* key_off, const uint8_t* val_blob, const uint64_t* val_off,
                                   uint64_t n, int insert, uint8_t* new_root, uint64_t* n_nodes, uint64_t* n_bytes,
                                   uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off, uint64_t node_cap,
                                   uint8_t* digests, void* stream) {
  return update_device_entry(store, old_root, key_blob, key_off, val_blob, val_off, n, insert, new_root, n_nodes,
                             n_bytes, node_blob, blob_cap, node_off, node_cap, digests, stream, true, true);
}

// The host form of the same (state/pruning_state.py:60-61, 84-85; state/trie/pruning_trie.py:683-848,
// 1006-1027): keys in any order, the last of equal keys wins, a removal over a set as a set over a
// removal, as the sequence of calls gives.
int pv_state_apply(int32_t store, const uint8_t* old_root, const uint8_t* key_blob, const uint64_t* key_off,
                   const uint8_t* val_blob, const uint64_t* val_off, uint64_t n, int insert, uint8_t* new_root,
                   uint64_t* n_nodes, uint64_t* n_bytes, uint8_t* node_blob, uint64_t blob_cap, uint64_t* node_off,
                   uint64_t node_cap, uint8_t* digests) {
  return update_host_entry(store, old_root, key_blob, key_off, val_blob, val_off, n, insert, new_root, n_nodes,
                           n_bytes, node_blob, blob_cap, node_off, node_cap, digests, true);
}

}  // extern "C"

namespace {
void release_stores() {
  for (auto& st : g_stores) store_release(st);
  g_stores.clear();
}
}  // namespace
