// RFC 6962 Merkle audit paths and consistency proofs, one proof per lane.
//
// Verification restates ledger/merkle_verifier.py: mp_verify_inclusion is
// MerkleVerifier._calculate_root_hash_from_audit_path plus the root compare of
// verify_leaf_hash_inclusion (:155-238), mp_verify_consistency is
// verify_tree_consistency (:47-153) with the same order of decisions.
//
// Generation reads a resident level-wise tree (lv[l][j] = node j of level l,
// level 0 = the leaf hashes, an odd last node moves up unchanged: what
// k_merkle_level builds).  For a prefix of s leaves every node of the prefix
// tree is either a node of the resident tree or lies on the prefix's right
// edge; the right edge is one bottom-up chain
//   e_0 = lv[0][s-1],  e_{l+1} = (last_l & 1) ? H(lv[l][last_l - 1], e_l) : e_l,
//   last_l = (s-1) >> l,
// whose top is MTH(0, s).  CompactMerkleTree.inclusion_proof(m, s) and
// consistency_proof(a, b) (ledger/compact_merkle_tree.py:213-249) are then a
// gather of level nodes with e_l substituted at index last_l.  The chain is
// walked in lock step with the path: one current e in registers, no
// per-level array.
//
// Digests stay in memory word order (8 little-endian words, as k_merkle_level
// keeps them); every index and size is 64-bit.
#pragma once
#include <stdint.h>
#include "pv_sha256.h"

namespace pv {

// == PV_MP_* of include/plenum_verify.h (pv_kernels.hip asserts it)
constexpr uint32_t MP_OK = 0;
constexpr uint32_t MP_BAD_RANGE = 1;      // index >= tree_size, old_size > new_size
constexpr uint32_t MP_TOO_SHORT = 2;
constexpr uint32_t MP_TOO_LONG = 3;
constexpr uint32_t MP_ROOT_MISMATCH = 4;  // inclusion; consistency: the new root differs
constexpr uint32_t MP_INCONSISTENT = 5;   // the old root differs / equal sizes, different roots

// len_out of a refused request (the generation kernels never clamp)
constexpr uint32_t MP_LEN_REFUSED = 0xffffffffu;

// walk phases of the two verifier state machines
constexpr uint32_t MP_WALK = 0;    // more levels to go
constexpr uint32_t MP_CLOSE = 1;   // walk finished, roots still to compare
constexpr uint32_t MP_FINAL = 2;   // status decided

// one 32-byte node as two 16-byte accesses (p 16-byte aligned on the device)
PV_HD void mp_load(uint32_t h[8], const uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
  h[0] = a.x; h[1] = a.y; h[2] = a.z; h[3] = a.w;
  h[4] = b.x; h[5] = b.y; h[6] = b.z; h[7] = b.w;
#else
  for (int k = 0; k < 8; ++k) h[k] = p[k];
#endif
}

PV_HD void mp_store(uint32_t* p, const uint32_t h[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  reinterpret_cast<uint4*>(p)[0] = make_uint4(h[0], h[1], h[2], h[3]);
  reinterpret_cast<uint4*>(p)[1] = make_uint4(h[4], h[5], h[6], h[7]);
#else
  for (int k = 0; k < 8; ++k) p[k] = h[k];
#endif
}

PV_HD void mp_copy(uint32_t d[8], const uint32_t s[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = s[k];
}

PV_HD bool mp_equal(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t d = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) d |= a[k] ^ b[k];
  return d == 0;
}

// h <- right ? H(sib || h) : H(h || sib): the operand order is a select, so a
// wave hashing left and right children together does not branch
PV_HD void mp_hash_sel(uint32_t h[8], const uint32_t sib[8], bool right) {
  uint32_t lr[16];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    lr[k] = right ? sib[k] : h[k];
    lr[8 + k] = right ? h[k] : sib[k];
  }
  sha256_node(h, lr);
}

PV_HD uint32_t mp_ctz64(uint64_t x) { return (uint32_t)__builtin_ctzll(x); }

// ------------------------------------------------------------ audit path check
// State of one walk.  Every step consumes exactly one proof node and does one
// node hash: levels where the node is the last of its level and a left child
// (no sibling, nothing consumed) are skipped in one shift, so the lanes of a
// wave differ in trip count only.  nxt holds the node the next step consumes,
// loaded one step ahead of the compression that needs it.
struct MpIncl {
  uint32_t h[8], nxt[8];
  uint64_t node, last, pos, end, stop;
  uint32_t phase, status;
};

PV_HD void mp_incl_begin(MpIncl& s, const uint32_t leaf[8], uint64_t index, uint64_t tree_size, const uint32_t* nodes,
                         uint64_t n_nodes) {
  mp_copy(s.h, leaf);
#pragma unroll
  for (int k = 0; k < 8; ++k) s.nxt[k] = 0;
  s.node = index;
  s.last = tree_size - 1;
  s.pos = 0;
  s.end = n_nodes;
  s.stop = 0;
  s.status = MP_OK;
  if (index >= tree_size) {
    s.status = MP_BAD_RANGE;
    s.phase = MP_FINAL;
    return;
  }
  s.phase = s.last > 0 ? MP_WALK : MP_CLOSE;
  if (s.phase == MP_WALK && n_nodes) mp_load(s.nxt, nodes);
}

// one consumed node; requires phase == MP_WALK
PV_HD void mp_incl_step(MpIncl& s, const uint32_t* nodes) {
  if (s.pos == s.end) {   // the reference tests this at every level, consuming or not
    s.status = MP_TOO_SHORT;
    s.stop = s.node;
    s.phase = MP_FINAL;
    return;
  }
  if (!(s.node & 1) && s.node == s.last) {   // last of its level and a left child: up to the first odd level
    const uint32_t sh = mp_ctz64(s.node);    // node == last > 0
    s.node >>= sh;
    s.last >>= sh;
  }
  uint32_t sib[8];
  mp_copy(sib, s.nxt);
  ++s.pos;
  if (s.pos < s.end) mp_load(s.nxt, nodes + 8 * s.pos);
  mp_hash_sel(s.h, sib, (s.node & 1) != 0);
  s.node >>= 1;
  s.last >>= 1;
  if (s.last == 0) s.phase = MP_CLOSE;
}

PV_HD uint32_t mp_incl_finish(const MpIncl& s, const uint32_t root[8]) {
  if (s.phase == MP_FINAL) return s.status;
  if (s.pos < s.end) return MP_TOO_LONG;
  return mp_equal(s.h, root) ? MP_OK : MP_ROOT_MISMATCH;
}

// nodes = this proof's n_nodes nodes.  computed <- the hash the walk reached
// (the root candidate); *stop <- the node index a too-short walk stopped at.
PV_HD uint32_t mp_verify_inclusion(const uint32_t leaf_hash[8], uint64_t index, uint64_t tree_size,
                                   const uint32_t* nodes, uint64_t n_nodes, const uint32_t root[8],
                                   uint32_t computed[8], uint64_t* stop) {
  MpIncl s;
  mp_incl_begin(s, leaf_hash, index, tree_size, nodes, n_nodes);
  while (s.phase == MP_WALK) mp_incl_step(s, nodes);
  mp_copy(computed, s.h);
  *stop = s.stop;
  return mp_incl_finish(s, root);
}

// ----------------------------------------------------------- consistency check
struct MpCons {
  uint32_t oh[8], nh[8], nxt[8];
  uint64_t node, last, pos, end;
  uint32_t phase, status;
};

PV_HD void mp_cons_begin(MpCons& s, uint64_t old_size, uint64_t new_size, const uint32_t old_root[8],
                         const uint32_t new_root[8], const uint32_t* nodes, uint64_t n_nodes) {
  mp_copy(s.oh, old_root);
  mp_copy(s.nh, new_root);
#pragma unroll
  for (int k = 0; k < 8; ++k) s.nxt[k] = 0;
  s.node = s.last = s.pos = 0;
  s.end = n_nodes;
  s.phase = MP_FINAL;
  s.status = MP_OK;
  if (old_size > new_size) {
    s.status = MP_BAD_RANGE;
    return;
  }
  if (old_size == new_size) {   // identical trees: the proof is ignored
    s.status = mp_equal(old_root, new_root) ? MP_OK : MP_INCONSISTENT;
    return;
  }
  if (old_size == 0) return;    // anything is consistent with the empty tree
  s.node = old_size - 1;
  s.last = new_size - 1;
  const uint32_t sh = mp_ctz64(~s.node);   // right children: in both trees, move up (node < last <= 2^64 - 1)
  s.node >>= sh;
  s.last >>= sh;                           // still node < last
  if (s.node) {
    if (n_nodes == 0) {
      s.status = MP_TOO_SHORT;
      return;
    }
    mp_load(s.oh, nodes);
    mp_copy(s.nh, s.oh);
    s.pos = 1;
  } else {
    mp_copy(s.nh, s.oh);        // the old tree was balanced: start from its root
  }
  s.phase = MP_WALK;
  if (s.pos < s.end) mp_load(s.nxt, nodes + 8 * s.pos);
}

// one consumed node.  The reference's second loop (node == 0, last > 0) is the
// left-child rule of its first with node = 0, so one loop on `last` serves both.
PV_HD void mp_cons_step(MpCons& s, const uint32_t* nodes) {
  if (!(s.node & 1) && s.node == s.last) {   // a left child without a sibling in either tree
    const uint32_t sh = mp_ctz64(s.node);
    s.node >>= sh;
    s.last >>= sh;
  }
  if (s.pos == s.end) {
    s.status = MP_TOO_SHORT;
    s.phase = MP_FINAL;
    return;
  }
  uint32_t sib[8];
  mp_copy(sib, s.nxt);
  ++s.pos;
  if (s.pos < s.end) mp_load(s.nxt, nodes + 8 * s.pos);
  const bool right = (s.node & 1) != 0;
  if (right) mp_hash_sel(s.oh, sib, true);   // the left sibling is in both trees
  mp_hash_sel(s.nh, sib, right);
  s.node >>= 1;
  s.last >>= 1;
  if (s.last == 0) s.phase = MP_CLOSE;
}

// "new root differs" wins over "old root differs"; extra nodes are accepted
PV_HD uint32_t mp_cons_finish(const MpCons& s, const uint32_t old_root[8], const uint32_t new_root[8]) {
  if (s.phase == MP_FINAL) return s.status;
  if (!mp_equal(s.nh, new_root)) return MP_ROOT_MISMATCH;
  if (!mp_equal(s.oh, old_root)) return MP_INCONSISTENT;
  return MP_OK;
}

PV_HD uint32_t mp_verify_consistency(uint64_t old_size, uint64_t new_size, const uint32_t old_root[8],
                                     const uint32_t new_root[8], const uint32_t* nodes, uint64_t n_nodes,
                                     uint32_t old_computed[8], uint32_t new_computed[8]) {
  MpCons s;
  mp_cons_begin(s, old_size, new_size, old_root, new_root, nodes, n_nodes);
  while (s.phase == MP_WALK) mp_cons_step(s, nodes);
  mp_copy(old_computed, s.oh);
  mp_copy(new_computed, s.nh);
  return mp_cons_finish(s, old_root, new_root);
}

// ------------------------------------------------- generation over the levels
// e_l -> e_{l+1} (last = last_l > 0).  full: the prefix is the whole resident
// tree, whose level l + 1 already holds the chain -- nothing is hashed.
PV_HD void mp_chain_step(uint32_t e[8], const uint32_t* const* lv, uint32_t l, uint64_t last, bool full) {
  if (full) {
    mp_load(e, lv[l + 1] + 8 * (last >> 1));
  } else if (last & 1) {
    uint32_t left[8];
    mp_load(left, lv[l] + 8 * (last - 1));
    mp_hash_sel(e, left, true);
  }
}

// the node at (l, i) of the prefix tree whose last index at level l is `last`
PV_HD void mp_node_at(uint32_t t[8], const uint32_t e[8], const uint32_t* const* lv, uint32_t l, uint64_t i,
                      uint64_t last) {
  if (i == last) mp_copy(t, e);
  else mp_load(t, lv[l] + 8 * i);
}

// CompactMerkleTree.inclusion_proof(m, s) over a resident tree of n leaves
// (m < s, 1 <= s <= n: checked by the caller).  out <- the path, bottom-up;
// root <- MTH(0, s); returns the length (<= depth of the resident tree).
PV_HD uint32_t mp_audit_path(const uint32_t* const* lv, uint64_t n, uint64_t m, uint64_t s, uint32_t* out,
                             uint32_t root[8]) {
  const bool full = s == n;
  uint64_t last = s - 1, idx = m;
  uint32_t l = 0, cnt = 0;
  uint32_t e[8];
  mp_load(e, lv[0] + 8 * last);
  while (last > 0) {
    const uint64_t sib = idx ^ 1;
    if (sib <= last) {
      uint32_t t[8];
      mp_node_at(t, e, lv, l, sib, last);
      mp_store(out + 8 * (uint64_t)cnt, t);
      ++cnt;
    }
    mp_chain_step(e, lv, l, last, full);
    ++l;
    idx >>= 1;
    last >>= 1;
  }
  mp_copy(root, e);
  return cnt;
}

// CompactMerkleTree.consistency_proof(a, b), a <= b <= n, b >= 1 or a == 0
// (checked by the caller), driven by the verifier's own walk; returns the
// length (<= depth + 1), 0 for a == 0 or a == b
PV_HD uint32_t mp_cons_proof(const uint32_t* const* lv, uint64_t n, uint64_t a, uint64_t b, uint32_t* out) {
  if (a == 0 || a == b) return 0;
  const bool full = b == n;
  uint64_t node = a - 1, last = b - 1;
  uint32_t l = 0, cnt = 0;
  uint32_t e[8], t[8];
  mp_load(e, lv[0] + 8 * last);
  while (node & 1) {   // node < last, so last > 0 on every trip
    mp_chain_step(e, lv, l, last, full);
    ++l;
    node >>= 1;
    last >>= 1;
  }
  if (node) {
    mp_node_at(t, e, lv, l, node, last);
    mp_store(out + 8 * (uint64_t)cnt, t);
    ++cnt;
  }
  while (last > 0) {
    if (node & 1) {
      mp_load(t, lv[l] + 8 * (node - 1));
      mp_store(out + 8 * (uint64_t)cnt, t);
      ++cnt;
    } else if (node < last) {
      mp_node_at(t, e, lv, l, node + 1, last);
      mp_store(out + 8 * (uint64_t)cnt, t);
      ++cnt;
    }
    mp_chain_step(e, lv, l, last, full);
    ++l;
    node >>= 1;
    last >>= 1;
  }
  return cnt;
}

}  // namespace pv
