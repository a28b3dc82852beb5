// The ledger write cycle over the resident level-wise Merkle tree: the
// right-edge rebuild behind stage / discard, CompactMerkleTree's frontier, and
// the order in which the reference's hash store receives leaves and nodes.
//
// The tree is the one of pv_merkle_proof.h: lv[l][j] = node j of level l,
// level 0 = the leaf hashes, an odd last node moves up unchanged.  Node j of
// level l covers leaves [j << l, min(n, (j + 1) << l)); it is *complete* when
// (j + 1) << l <= n, and a complete node never changes again.
//
// Edge rebuild.  When the leaves from f0 on change (appended: f0 = the old
// size; removed down to n_new: f0 = n_new - 1, whose ancestors lose their
// right parts), exactly the nodes [f0 >> l, level_count(n_new, l)) of every
// level l change.  Level l + 1 is recomputed from the changed nodes of level
// l, handed over in a buffer of the group (LDS on the device), plus at most
// one node the group did not write: the complete left sibling f_l - 1 when
// f_l is odd.  Nothing the rebuild stored is read back from the levels.
//
// Hash store.  Appending leaf e (sequence number, 1-based) completes one node
// per trailing zero bit of e: height h = 1 .. ctz(e), which is lv[h][(e >> h) - 1].
// CompactMerkleTree._push_subtree (ledger/compact_merkle_tree.py:95-136) writes
// them in that order after the leaf hash, so with e - 1 leaves in, e - 1 -
// popcount(e - 1) nodes are in, and the node of height h lands at the 1-based
// position (e - 1) - popcount(e - 1) + h == HashStore.getNodePosition(e, h).
//
// Frontier.  CompactMerkleTree.hashes of a tree of s leaves: for every set bit
// b of s, largest first, the complete node lv[b][(s >> b) - 1].
#pragma once
#include <stdint.h>
#include "pv_merkle_proof.h"

namespace pv {

constexpr uint32_t ML_EDGE_MAX = 1024;   // n_new - f0 one group serves
constexpr uint32_t ML_EDGE_BUF = 513;    // changed nodes of one level above the leaves, at most
constexpr uint32_t ML_LEVELS = 48;       // level pointers handed to the edge kernel by value (trees hold <= 2^40 leaves)

struct MlLevels {
  uint32_t* lv[ML_LEVELS];
};

PV_HD uint64_t ml_level_count(uint64_t n, uint32_t l) { return n == 0 ? 0 : ((n - 1) >> l) + 1; }
PV_HD uint32_t ml_popc64(uint64_t x) { return (uint32_t)__builtin_popcountll(x); }

// nodes in the hash store once e leaves were appended one by one
PV_HD uint64_t ml_nodes_upto(uint64_t e) { return e - ml_popc64(e); }

// One level of the rebuild: nodes [f >> 1, ceil(cnt / 2)) of the level above a
// level of cnt nodes whose nodes f .. cnt - 1 changed (f < cnt).  `changed`
// holds those, node f first; `in` is the level itself and is read at f - 1
// only.  Node i goes to out[i] and to keep[i - (f >> 1)], the hand-over to the
// next level.  Thread tid of nthreads takes every nthreads-th node.
PV_HD void ml_edge_level(const uint32_t* in, const uint32_t* changed, uint64_t f, uint64_t cnt, uint32_t* out,
                         uint32_t* keep, uint32_t tid, uint32_t nthreads) {
  const uint64_t fo = f >> 1, todo = ((cnt + 1) >> 1) - fo;
  for (uint64_t j = tid; j < todo; j += nthreads) {
    const uint64_t i = fo + j, a = 2 * i;
    uint32_t lr[16], h[8];
    if (a >= f) mp_load(lr, changed + 8 * (a - f));
    else mp_load(lr, in + 8 * a);   // a == f - 1: complete, not written here
    if (a + 1 < cnt) {
      mp_load(lr + 8, changed + 8 * (a + 1 - f));
      sha256_node(h, lr);
    } else {
      mp_copy(h, lr);               // the odd last node moves up
    }
    mp_store(keep + 8 * j, h);
    mp_store(out + 8 * i, h);
  }
}

// Every ancestor of the leaves [f0, n_new) of a tree of n_new leaves, f0 <
// n_new <= f0 + ML_EDGE_MAX, by one group of nthreads threads that share buf0
// and buf1 (ML_EDGE_BUF nodes each) and meet at barrier().  lv[l] has room for
// ml_level_count(n_new, l) nodes.  Returns the depth of the tree.
template <class Levels, class Barrier>
PV_HD uint32_t ml_edge_rebuild(const Levels& lv, uint64_t f0, uint64_t n_new, uint32_t* buf0, uint32_t* buf1,
                               uint32_t tid, uint32_t nthreads, Barrier barrier) {
  if (n_new <= 1) return 0;
  uint64_t f = f0, cnt = n_new;
  ml_edge_level(lv[0], lv[0] + 8 * f, f, cnt, lv[1], buf0, tid, nthreads);   // the leaves are read in place
  barrier();
  f >>= 1;
  cnt = (cnt + 1) >> 1;
  uint32_t l = 1;
  uint32_t *cur = buf0, *nxt = buf1;
  while (cnt > 1) {
    ml_edge_level(lv[l], cur, f, cnt, lv[l + 1], nxt, tid, nthreads);
    barrier();   // one per level: the next level writes the buffer this one has finished reading
    uint32_t* t = cur;
    cur = nxt;
    nxt = t;
    f >>= 1;
    cnt = (cnt + 1) >> 1;
    ++l;
  }
  return l;
}

// What the hash store receives for leaf e of the range (first, last]: its hash
// at leaf_out[e - first - 1] and its ctz(e) nodes from node_out[ml_nodes_upto(e - 1)
// - ml_nodes_upto(first)] on.  Either output may be null.
PV_HD void ml_hs_gather(const uint32_t* const* lv, uint64_t first, uint64_t e, uint32_t* leaf_out,
                        uint32_t* node_out) {
  uint32_t t[8];
  if (leaf_out) {
    mp_load(t, lv[0] + 8 * (e - 1));
    mp_store(leaf_out + 8 * (e - first - 1), t);
  }
  if (!node_out) return;
  const uint64_t pos = ml_nodes_upto(e - 1) - ml_nodes_upto(first);
  const uint32_t nh = mp_ctz64(e);
  for (uint32_t h = 1; h <= nh; ++h) {
    mp_load(t, lv[h] + 8 * ((e >> h) - 1));
    mp_store(node_out + 8 * (pos + h - 1), t);
  }
}

// the same walk comparing: returns how many of leaf e's nodes differ from
// `nodes` (laid out as ml_hs_gather writes them); *lowest <- the smallest
// differing index, untouched when none differ
PV_HD uint32_t ml_hs_check(const uint32_t* const* lv, uint64_t first, uint64_t e, const uint32_t* nodes,
                           uint64_t* lowest) {
  const uint64_t pos = ml_nodes_upto(e - 1) - ml_nodes_upto(first);
  const uint32_t nh = mp_ctz64(e);
  uint32_t bad = 0;
  for (uint32_t h = nh; h >= 1; --h) {   // downwards: the last hit is the lowest index
    uint32_t t[8], g[8];
    mp_load(t, lv[h] + 8 * ((e >> h) - 1));
    mp_load(g, nodes + 8 * (pos + h - 1));
    if (!mp_equal(t, g)) {
      ++bad;
      *lowest = pos + h - 1;
    }
  }
  return bad;
}

// frontier node of bit b of size (set): out[popcount of the bits above b]
PV_HD void ml_frontier_node(const uint32_t* const* lv, uint64_t size, uint32_t b, uint32_t* out) {
  uint32_t t[8];
  mp_load(t, lv[b] + 8 * ((size >> b) - 1));
  mp_store(out + 8 * (uint64_t)ml_popc64(b < 63 ? size >> (b + 1) : 0), t);
}

}  // namespace pv
