// The resident trie node store on the host -- test tooling only.  It includes
// the product header indy-plenum_amd/csrc/pv_trie_store.h unchanged and runs
// what the kernels run, sequentially: the layout rule of k_trie_store_layout,
// ts_insert per new node (k_trie_store_insert), the growth rule of
// pv_state_store_add (double the table before the nodes exceed slots / 2,
// k_trie_store_rehash), sg_walk per query (k_trie_prove) and the byte gather of
// k_trie_proof_pack.  Shared by libstatestorecheck.so and statestorecheck_asan.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#ifndef PV_HD
#define PV_HD static inline
#endif
#include "../../indy-plenum_amd/csrc/pv_sha3.h"
#include "../../indy-plenum_amd/csrc/pv_trie_store.h"

namespace ssh {

struct Store {
  std::vector<uint8_t> blob;   // n_bytes + 16 (the over-read contract of pv_sha3.h)
  std::vector<uint64_t> beg, end;
  std::vector<uint32_t> dig;
  std::vector<uint8_t> dup;
  std::vector<uint32_t> table;
  uint64_t n_bytes = 0, n_unique = 0;
  uint64_t nodes() const { return beg.size(); }
};

inline void init(Store& st, uint64_t node_hint) {
  uint64_t slots = pv::TS_MIN_SLOTS;
  while (node_hint > slots / 2) slots *= 2;
  st.table.assign(slots, 0);
  st.blob.assign(16, 0);
}

// ids 0 .. n - 1 that hold a slot, into an empty table of `slots` slots
inline void rehash(Store& st, uint64_t slots, uint64_t n) {
  st.table.assign(slots, 0);
  for (uint64_t i = 0; i < n; ++i)
    if (!st.dup[i]) (void)pv::ts_insert(st.table.data(), (uint32_t)slots, st.dig.data(), st.dup.data(), (uint32_t)i);
}

// the table part of an add: ids first .. first + n_new - 1 are in dig already
inline uint64_t insert_new(Store& st, uint64_t first, uint64_t n_new) {
  const uint64_t nodes = first + n_new;
  st.dup.resize(nodes, 0);
  if (nodes > st.table.size() / 2) {
    uint64_t ns = st.table.size();
    while (nodes > ns / 2) ns *= 2;
    rehash(st, ns, first);
  }
  uint64_t added = 0;
  for (uint64_t i = 0; i < n_new; ++i)
    added += pv::ts_insert(st.table.data(), (uint32_t)st.table.size(), st.dig.data(), st.dup.data(),
                           (uint32_t)(first + i));
  st.n_unique += added;
  return added;
}

// n_new nodes, node i = node_blob[node_off[i] .. node_off[i + 1]); -> nodes new to the store
inline uint64_t add(Store& st, const uint8_t* node_blob, const uint64_t* node_off, uint64_t n_new) {
  if (n_new == 0) return 0;
  const uint64_t first = st.nodes(), base = st.n_bytes, o0 = node_off[0];
  const uint64_t total = node_off[n_new] - o0;
  st.blob.resize(base + total + 16);
  if (total) memcpy(st.blob.data() + base, node_blob + o0, total);
  memset(st.blob.data() + base + total, 0, 16);
  st.n_bytes += total;
  st.dig.resize(8 * (first + n_new));
  for (uint64_t i = 0; i < n_new; ++i) {
    const uint64_t a = node_off[i] - o0, b = node_off[i + 1] - o0;
    const bool ok = a < b && b <= total;
    st.beg.push_back(base + (ok ? a : 0));
    st.end.push_back(base + (ok ? b : 0));
    pv::sha3_256_msg(&st.dig[8 * (first + i)], st.blob.data() + st.beg.back(), st.end.back() - st.beg.back());
  }
  return insert_new(st, first, n_new);
}

// n_new raw digests (32 bytes each) as nodes without bytes: the table alone
inline uint64_t add_digests(Store& st, const uint8_t* digests, uint64_t n_new) {
  const uint64_t first = st.nodes();
  st.dig.resize(8 * (first + n_new));
  if (n_new) memcpy(&st.dig[8 * first], digests, 32 * n_new);
  for (uint64_t i = 0; i < n_new; ++i) {
    st.beg.push_back(st.n_bytes);
    st.end.push_back(st.n_bytes);
  }
  return insert_new(st, first, n_new);
}

// The arrays a walk and a pack read; the sanitizer build points them at
// exact-size copies.
struct View {
  const uint8_t* blob;
  const uint64_t *beg, *end;
  const uint32_t *dig, *table;
  uint32_t slots, n_nodes;
};

inline View view(const Store& st) {
  return View{st.blob.data(), st.beg.data(), st.end.data(), st.dig.data(), st.table.data(), (uint32_t)st.table.size(),
              (uint32_t)st.nodes()};
}

// pv_state_store_prove on the host.  0, or -22 when proof_blob is given and
// proof_cap is below the proofs' bytes (proof_off and the rest are written).
inline int prove(const View& v, const uint8_t* roots, const uint32_t* root_idx, uint64_t n_roots,
                 const uint8_t* key_blob, const uint64_t* key_off, uint64_t n_queries, uint32_t max_nodes,
                 uint8_t* status, uint32_t* node_count, uint32_t* node_ids, uint64_t* proof_off, uint64_t* val_rel,
                 uint64_t* val_len, uint8_t* proof_blob, uint64_t proof_cap) {
  proof_off[0] = 0;
  for (uint64_t q = 0; q < n_queries; ++q) {
    const uint64_t p = root_idx ? root_idx[q] : q;
    pv::SgResult r;
    r.status = pv::SP_MALFORMED;
    r.node_count = 0;
    r.body_len = r.last_beg = r.val_beg = r.val_len = 0;
    if (p < n_roots) {
      uint32_t rt[8];
      memcpy(rt, roots + 32 * p, 32);
      pv::sg_walk(v.blob, v.beg, v.end, v.dig, v.table, v.slots, v.n_nodes, rt, key_blob + key_off[q],
                  key_off[q + 1] - key_off[q], node_ids + q * max_nodes, max_nodes, r);
    }
    uint64_t pl;
    pv::sg_outputs(r, pl, val_rel[q], val_len[q]);
    status[q] = (uint8_t)r.status;
    node_count[q] = r.node_count;
    proof_off[q + 1] = proof_off[q] + pl;
  }
  if (!proof_blob) return 0;
  if (proof_cap < proof_off[n_queries]) return -22;
  for (uint64_t q = 0; q < n_queries; ++q) {
    const uint64_t o = proof_off[q], len = proof_off[q + 1] - o;
    const uint32_t* ids = node_ids + q * max_nodes;
    uint64_t body;
    if (!pv::sg_pack_check(v.beg, v.end, v.n_nodes, ids, node_count[q], max_nodes, len, body)) continue;
    const uint32_t hl = pv::rlp_header_len(body);
    for (uint32_t k = 0; k < hl; ++k) proof_blob[o + k] = pv::rlp_header_byte(192, body, hl, k);
    uint64_t w = o + hl;
    for (uint32_t k = node_count[q]; k-- > 0;) {
      const uint64_t b = v.beg[ids[k]], n = v.end[ids[k]] - b;
      if (n) memcpy(proof_blob + w, v.blob + b, n);
      w += n;
    }
  }
  return 0;
}

}  // namespace ssh
