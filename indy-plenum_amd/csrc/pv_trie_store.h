// Resident trie node store, shared by device and host: the serving side of the
// state proof.  The reference's trie database is content-addressed and
// append-only: a node is stored under sha3(rlp(node)) and never changes
// (state/trie/pruning_trie.py:346-353, _decode_to_node -> _db.get(hash)), and
// generate_state_proof (:1043-1050, :1075-1098) is Trie._get (:376-407) from a
// root plus a record of every node it fetched by hash, with the root appended.
// So the store only grows ("add these node RLPs") between two prunes
// (pv_trie_prune.h: keep what the named roots reach, renumber, rebuild the
// table) and a proof at any root it holds, current or historical, is a walk
// over hash lookups.
//
// Layout.  Node id j is the byte range blob[beg[j], end[j]) of one blob, its
// SHA3-256 digest is dig[8 j .. 8 j + 7] (little-endian words, from
// k_sha3_256).  The blob keeps the over-read contract of pv_sha3.h: 4-byte
// aligned base and 16 readable bytes after the last node.
//
// Table.  Open addressing with linear probing over uint32_t slots: 0 = empty,
// otherwise node id + 1.  `slots` is a power of two >= TS_MIN_SLOTS; the start
// slot is digest word 0 & (slots - 1); a probe compares the full 8 words, first
// word first, as sp_find does.  The callers keep the load at or below 1/2, which
// already ends every probe at an empty slot; the loops still carry the explicit
// bound of `slots` trips, as sp_verify carries its step bound.
//
// Insert.  One routine for both builds: ts_claim / ts_lower are atomicCAS /
// atomicMin on the device and their sequential meaning on the host.  A lane
// claims the first empty slot of its chain.  At an occupied slot (or a lost
// CAS) it compares digests: different -> next slot; equal -> a duplicate, and
// the LOWER id keeps the slot (atomicMin), the other id is flagged in dup[].
// Slots only go from empty to a digest and keep that digest, so two lanes that
// insert the same new digest in one launch walk the same chain, meet in the
// same slot and end with exactly one slot; "lower id wins" makes the table and
// the flags independent of the order the lanes ran in, which is also what the
// sequential host twin (ids ascending) gives.  Only 1 is ever written to dup[]
// (it is zeroed before the launch), each flagged id by exactly one lane.
//
// The walk (sg_walk) descends by the step sp_verify takes (tn_step,
// pv_trie_node.h), at most 2 len(key) + 1 times, but resolves 32-byte child
// references with ts_find and records, instead of a verdict, the id of every
// node fetched by hash in walk order (root first), the byte range of the
// terminal value and a status.  Inline nodes are walked in place and are not
// proof nodes, as in the reference (spv_grabbing runs only on db fetches).
//
// The serialized proof is rlp(list of nodes) (Trie.serialize_proof,
// :1164-1170) with the nodes in REVERSE walk order: terminal node first, root
// last.  Root last is the one ordering property _generate_state_proof has
// (pf.append(root), and the NOTE at :1102); the rest of the reference's order
// is Python set order, so only the multiset of nodes and "root last" can agree.
// Blank root: the proof here is the empty list 0xc0 (what the fixture's
// blank_root row and the project's verifier use); the reference would
// serialize [b''] = 0xc1 0x80.
#pragma once
#include <stdint.h>

#include "pv_trie_proof.h"

namespace pv {

enum : uint32_t { SP_PATH_TOO_LONG = 4 };   // more hashed nodes than max_nodes; node_count is the true count

constexpr uint32_t TS_ABSENT = 0xffffffffu;
constexpr uint32_t TS_MIN_SLOTS = 64;
constexpr uint64_t TS_MAX_NODES = 0xfffffffeull;   // ids 0 .. 2^32 - 3: id + 1 fits a slot, TS_ABSENT is no id

// slot <- v if it is empty; the value seen before (0 = this call claimed it)
PV_HD uint32_t ts_claim(uint32_t* slot, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(slot, 0u, v);
#else
  const uint32_t old = *slot;
  if (old == 0) *slot = v;
  return old;
#endif
}

// slot <- min(slot, v); the value seen before
PV_HD uint32_t ts_lower(uint32_t* slot, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicMin(slot, v);
#else
  const uint32_t old = *slot;
  if (v < old) *slot = v;
  return old;
#endif
}

PV_HD bool ts_same(const uint32_t* a, const uint32_t* b) {
  if (a[0] != b[0]) return false;
  return a[1] == b[1] && a[2] == b[2] && a[3] == b[3] && a[4] == b[4] && a[5] == b[5] && a[6] == b[6] &&
         a[7] == b[7];
}

// id of the node with digest t among ids below n_nodes, or TS_ABSENT
PV_HD uint32_t ts_find(const uint32_t* table, uint32_t slots, const uint32_t* dig, uint32_t n_nodes,
                       const uint32_t t[8]) {
  const uint32_t mask = slots - 1;
  uint32_t s = t[0] & mask;
  for (uint32_t trip = 0; trip < slots; ++trip) {
    const uint32_t v = table[s];
    if (v == 0) return TS_ABSENT;
    if (v <= n_nodes && ts_same(dig + 8 * (uint64_t)(v - 1), t)) return v - 1;
    s = (s + 1) & mask;
  }
  return TS_ABSENT;
}

// Insert node `id` (its digest is dig[8 id ..]).  true: it claimed an empty
// slot (a digest the table did not hold).  false: a duplicate -- the lower of
// the two ids keeps the slot and the other is flagged in dup[] -- or, with no
// empty slot on the chain (the callers' load bound excludes it), not inserted
// and flagged.
PV_HD bool ts_insert(uint32_t* table, uint32_t slots, const uint32_t* dig, uint8_t* dup, uint32_t id) {
  const uint32_t mask = slots - 1;
  const uint32_t* t = dig + 8 * (uint64_t)id;
  uint32_t s = t[0] & mask;
  for (uint32_t trip = 0; trip < slots; ++trip) {
    const uint32_t v = ts_claim(table + s, id + 1);
    if (v == 0) return true;
    if (v == id + 1) return false;   // already there (a repeated launch)
    if (ts_same(dig + 8 * (uint64_t)(v - 1), t)) {
      const uint32_t seen = ts_lower(table + s, id + 1);   // equal digests only ever share this slot
      dup[seen > id + 1 ? seen - 1 : id] = 1;
      return false;
    }
    s = (s + 1) & mask;
  }
  dup[id] = 1;
  return false;
}

struct SgResult {
  uint32_t status;       // SP_OK, SP_NODE_MISSING, SP_MALFORMED or SP_PATH_TOO_LONG
  uint32_t node_count;   // hashed nodes fetched (the true count, also above max_nodes)
  uint64_t body_len;     // sum of their byte lengths
  uint64_t last_beg;     // blob offset of the last hashed node fetched (the terminal node)
  uint64_t val_beg;      // blob range of the value, inside the terminal node; val_len == 0: absent
  uint64_t val_len;
};

// The generation walk for one (root, key).  ids[0 .. min(node_count, max_nodes))
// receives the hashed nodes' ids, root first; ids goes straight to the caller's
// (global) memory, so no per-lane array is indexed at run time.  RECORD false is
// the read of pv_trie_get.h: the same descent, ids and max_nodes are not looked
// at, and no walk is SP_PATH_TOO_LONG.
template <bool RECORD>
PV_HD void sg_walk_t(const uint8_t* blob, const uint64_t* beg, const uint64_t* end, const uint32_t* dig,
                     const uint32_t* table, uint32_t slots, uint32_t n_nodes, const uint32_t root[8],
                     const uint8_t* key, uint64_t klen, uint32_t* ids, uint32_t max_nodes, SgResult& r) {
  r.status = SP_OK;
  r.node_count = 0;
  r.body_len = r.last_beg = r.val_beg = r.val_len = 0;
  if (sp_is_blank_root(root)) return;   // no lookup: 0 nodes, absent
  uint32_t j = ts_find(table, slots, dig, n_nodes, root);
  if (j == TS_ABSENT) {
    r.status = SP_NODE_MISSING;
    return;
  }
  uint64_t cb = beg[j], ce = end[j];   // the current node's RLP
  if (RECORD && max_nodes) ids[0] = j;
  r.node_count = 1;
  r.body_len = ce - cb;
  r.last_beg = cb;
  const uint64_t total = 2 * klen;
  uint64_t nib = 0;   // key nibbles consumed
  uint32_t st = SP_MALFORMED;   // the step bound ran out
  for (uint64_t step = 0; step <= total; ++step) {
    uint64_t ob, oe;
    uint32_t t[8];
    const uint32_t next = tn_step(blob, cb, ce, key, total, nib, ob, oe, t);
    if (next == TN_INLINE) {   // walked in place, and no proof node
      cb = ob;
      ce = oe;
      continue;
    }
    if (next != TN_HASHED) {   // the walk ends here; TN_ABSENT: proven absent
      if (next == TN_VALUE) {
        r.val_beg = ob;
        r.val_len = oe - ob;
      }
      st = next == TN_MALFORMED ? SP_MALFORMED : next == TN_MISSING ? SP_NODE_MISSING : SP_OK;
      break;
    }
    j = ts_find(table, slots, dig, n_nodes, t);
    if (j == TS_ABSENT) {
      st = SP_NODE_MISSING;
      break;
    }
    cb = beg[j];
    ce = end[j];
    if (RECORD && r.node_count < max_nodes) ids[r.node_count] = j;
    ++r.node_count;   // counted on above max_nodes, without storing
    r.body_len += ce - cb;
    r.last_beg = cb;
  }
  if (RECORD && st == SP_OK && r.node_count > max_nodes) st = SP_PATH_TOO_LONG;
  r.status = st;
}

PV_HD void sg_walk(const uint8_t* blob, const uint64_t* beg, const uint64_t* end, const uint32_t* dig,
                   const uint32_t* table, uint32_t slots, uint32_t n_nodes, const uint32_t root[8],
                   const uint8_t* key, uint64_t klen, uint32_t* ids, uint32_t max_nodes, SgResult& r) {
  sg_walk_t<true>(blob, beg, end, dig, table, slots, n_nodes, root, key, klen, ids, max_nodes, r);
}

// What a query's outputs are, from its walk: the serialized length (list header
// + node bytes; 1 for the blank root's 0xc0; 0 when no proof is emitted) and the
// value's offset inside those bytes.  The terminal node is serialized first.
PV_HD void sg_outputs(const SgResult& r, uint64_t& proof_len, uint64_t& val_rel, uint64_t& val_len) {
  proof_len = val_rel = val_len = 0;
  if (r.status != SP_OK) return;
  const uint32_t h = rlp_header_len(r.body_len);
  proof_len = h + r.body_len;
  if (r.val_len) {
    val_rel = h + (r.val_beg - r.last_beg);
    val_len = r.val_len;
  }
}

// Byte i of proof q's serialization: header, then nodes ids[count-1] .. ids[0].
// One proof's bytes [first, first + stride * k) are written by the caller's
// lanes; this is the sequential form the host build and one lane share.
// Returns false (nothing to write) when the ids or the length do not describe
// exactly `len` bytes: an id >= n_nodes, count > max_nodes, or header + body != len.
PV_HD bool sg_pack_check(const uint64_t* beg, const uint64_t* end, uint32_t n_nodes, const uint32_t* ids,
                         uint32_t count, uint32_t max_nodes, uint64_t len, uint64_t& body) {
  body = 0;
  if (len == 0 || count > max_nodes) return false;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t id = ids[i];
    if (id >= n_nodes) return false;
    body += end[id] - beg[id];
  }
  return rlp_header_len(body) + body == len;
}

}  // namespace pv
