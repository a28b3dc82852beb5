// Pruning the resident trie node store (pv_trie_store.h), shared by device and
// host: the mark rule.  The reference prunes by reference counts, a death row
// and an epoch ttl (state/trie/pruning_trie.py:208-230, 681;
// state/db/refcount_db.py).  Here the caller names the roots it keeps
// (committedHeadHash, the heads of uncommitted batches, every root still served
// to readers; state/pruning_state.py:87-102) and the store keeps exactly the
// nodes some sg_walk from one of those roots can fetch by hash.
//
// Mark rule, for one stored node (the grammar is in pv_trie_node.h):
//   branch      items 0 .. 15 are children; item 16 is a value, never a reference
//   leaf        no child
//   extension   item 1 is its child (an extension over no nibble ends every walk
//               SP_MALFORMED and has no child either)
//   child       a list: an inline node, visited in place by the same rule, never
//               looked up and never counted; a string of exactly 32 bytes: a
//               reference, resolved with ts_find -- found: the slot holder (the
//               lowest id among duplicates) is marked, not found: counted as
//               missing (a store filled from proofs is partial by design, and a
//               walk that needs that node answered SP_NODE_MISSING before and
//               still does); any other string: no reference
// A node, or an inline node, that does not parse at its own level (tn_scan or
// tn_path refuses it, or it has another item count than 2 or 17) contributes no
// children: every walk through it ended SP_MALFORMED without fetching further.
// The stored node that holds it is still kept.  A 32-byte leaf value or branch
// value is never followed.
//
// Inline nesting.  A well-formed trie nests inline nodes at most 3 deep under a
// hashed node (extension -> branch -> leaf: an inline node is under 32 bytes and
// a branch has 17 items, so one branch fits in a chain); junk added with
// pv_state_store_add may nest deeper.  The visit is a template over the levels
// left, so that every level's cursor lives in registers (no per-lane stack, no
// scratch): a hashed node and TP_MAX_INLINE inline levels under it.  A deeper
// list sets the caller's overflow flag, which the entry point turns into a
// refusal with the store unchanged, never into a smaller kept set.
//
// Marking is level-synchronous over one queue: every hashed node is marked
// (tp_mark: atomicOr on a word bitmap / its sequential meaning) and enqueued by
// the one lane that flipped its bit, so the queue holds each id at most once
// and n_unique entries cannot overflow; a level is the window of ids appended
// by the level before.
#pragma once
#include <stdint.h>

#include "pv_trie_store.h"

namespace pv {

constexpr int TP_MAX_INLINE = 7;   // inline levels under a hashed node (a well-formed trie needs 3)

struct TpCtx {
  const uint8_t* blob;
  const uint64_t *beg, *end;
  const uint32_t *dig, *table;
  uint32_t slots, n_nodes;
  uint32_t* bits;                // (n_nodes + 31) / 32 words: the mark bitmap
  uint32_t* queue;               // marked ids in marking order
  unsigned long long* counts;    // [0] queue tail, [1] missing references, [2] inline nesting above the limit
};

enum : int { TP_TAIL = 0, TP_MISSING = 1, TP_OVERFLOW = 2, TP_COUNTS = 3 };

// bit `id` <- 1; true for the caller that flipped it
PV_HD bool tp_mark(uint32_t* bits, uint32_t id) {
  const uint32_t m = 1u << (id & 31u);
#if defined(__HIP_DEVICE_COMPILE__)
  return (atomicOr(bits + (id >> 5), m) & m) == 0;
#else
  const uint32_t old = bits[id >> 5];
  bits[id >> 5] = old | m;
  return (old & m) == 0;
#endif
}

PV_HD bool tp_marked(const uint32_t* bits, uint32_t id) { return (bits[id >> 5] >> (id & 31u)) & 1u; }

// Append id to the queue.  Device: the lanes of the wave that are here together
// take their places with one atomic (the first of them adds, the others read
// its result and add their rank).
PV_HD void tp_push(const TpCtx& c, uint32_t id) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned long long m = __builtin_amdgcn_ballot_w64(true);
  const int leader = __ffsll(m) - 1;
  const uint32_t lane = __lane_id();
  unsigned long long b = 0;
  if ((int)lane == leader) b = atomicAdd(c.counts + TP_TAIL, (unsigned long long)__popcll(m));
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, leader);
  c.queue[lo + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = id;
#else
  c.queue[c.counts[TP_TAIL]++] = id;
#endif
}

PV_HD void tp_count(unsigned long long* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, 1ull);
#else
  ++*p;
#endif
}

// a root or a 32-byte child: the id it resolves to (marked and, when this call
// flipped the bit, enqueued), or TS_ABSENT
PV_HD uint32_t tp_resolve(const TpCtx& c, const uint32_t t[8]) {
  const uint32_t j = ts_find(c.table, c.slots, c.dig, c.n_nodes, t);
  if (j != TS_ABSENT && tp_mark(c.bits, j)) tp_push(c, j);
  return j;
}

template <int LEVELS>
PV_HD void tp_visit(const TpCtx& c, uint64_t cb, uint64_t ce);

// one child item
template <int LEVELS>
PV_HD void tp_child(const TpCtx& c, const TnItem& it) {
  if (it.l) {
    if constexpr (LEVELS == 0) tp_count(c.counts + TP_OVERFLOW);
    else tp_visit<LEVELS - 1>(c, it.s, it.e);
    return;
  }
  if (it.e - it.b != 32) return;
  uint32_t t[8];
  tn_load_ref(c.blob + it.b, t);
  if (tp_resolve(c, t) == TS_ABSENT) tp_count(c.counts + TP_MISSING);
}

// The node blob[cb, ce) with LEVELS inline levels allowed under it.  The first
// scan decides whether the node parses at its own level (and finds item 1);
// only then are its children visited, by a second scan over the same items.
template <int LEVELS>
PV_HD void tp_visit(const TpCtx& c, uint64_t cb, uint64_t ce) {
  const uint8_t* blob = c.blob;
  TnScan n;
  if (!tn_scan(blob, cb, ce, TN_NO_SLOT, n)) return;
  if (n.count == 2) {
    TnPath h;
    if (!tn_path(blob, n.i0, h)) return;
    if (h.leaf) return;      // item 1 is its value
    if (h.pn == 0) return;   // an extension over no nibble
    tp_child<LEVELS>(c, n.i1);
    return;
  }
  if (n.count != 17) return;
  TnItem it;
  it.e = n.pb;
  for (uint32_t k = 0; k < 16; ++k) {
    it.s = it.e;
    if (!rlp_item(blob, it.s, n.pe, it.l, it.b, it.e)) return;   // parsed by the first scan: never
    tp_child<LEVELS>(c, it);
  }
}

// keep root i: its status, SP_OK (held, or the blank root, which reaches nothing) or SP_NODE_MISSING
PV_HD uint32_t tp_seed(const TpCtx& c, const uint32_t root[8]) {
  if (sp_is_blank_root(root)) return SP_OK;
  return tp_resolve(c, root) == TS_ABSENT ? SP_NODE_MISSING : SP_OK;
}

// queue entry q: the children of the hashed node it names
PV_HD void tp_expand(const TpCtx& c, uint64_t q) {
  const uint32_t id = c.queue[q];
  tp_visit<TP_MAX_INLINE>(c, c.beg[id], c.end[id]);
}

// smallest power of two >= max(lo, v)
PV_HD uint64_t tp_pow2(uint64_t v, uint64_t lo) {
  uint64_t p = lo;
  while (p < v) p *= 2;
  return p;
}

}  // namespace pv
