// Reads from the resident trie node store, shared by device and host:
// PruningState.get / get_for_root_hash (state/pruning_state.py:63-77) for a
// batch of (root, key).  A read is the walk of a proof (sg_walk_t<false>,
// pv_trie_store.h, over tn_step, pv_trie_node.h) without the record of the
// nodes it fetched: no node ids, no max_nodes bound, and what leaves the device
// is the value alone, not the ~2 KB of nodes around it.
//
// Per query: a status, `found`, and the blob range of the value.  Without
// `decode` the range is the value as the trie stores it, rlp([v]) (what
// get_value=True of a proof returns); with `decode` it is the payload
// PruningState.get_decoded returns, rlp_decode(value)[0] (:162-163).  The range
// lies inside the terminal node; for an inline node that is inside its parent's
// bytes, a blob range like any other.
//
// found = 1 with an empty range (a stored rlp([b'']), which a host trie can
// hand over through pv_state_store_add) is a present key with an empty payload;
// found = 0 is an absent key, a blank root, or a status other than SP_OK.
//
// The decode (tg_decode).  Accepted: the stored value is ONE RLP list whose
// header length equals the rest of the value (short form 0xc0 + len, or long
// form 0xf7 + ll with ll length bytes), and the list's first item is a string:
// a single byte below 0x80 (its own payload), a short string 0x80 + len, or a
// long string 0xb7 + ll with ll length bytes.  Items after the first are not
// looked at.  Lengths are decoded as rlp_item does (pv_trie_node.h, the lenient
// state/util/fast_rlp.py:47-71): up to 8 length bytes, leading zeros and a long
// form over a short length pass -- no canonical-form check -- but every header
// and every payload is checked against the enclosing range before it is used,
// so nothing outside the value's range is read.  Everything else is
// SP_MALFORMED with found = 0: a bare string, an empty list, a first item that
// is a list, a list shorter or longer than the value, a length that overruns.
//
// The copy (tg_copy_group).  Values are tens to hundreds of bytes, so a group
// of TG_GROUP lanes, not a wave, gathers one value: lane l of the group moves
// bytes l, l + TG_GROUP, ...  The host build runs the same routine with one
// "lane" per group member in turn.
#pragma once
#include <stdint.h>

#include "pv_trie_store.h"

namespace pv {

constexpr uint32_t TG_GROUP = 16;   // lanes per value in k_trie_get_copy

// The payload [pb, pe) of the first item of the list blob[vb, ve); false: not the accepted form.
PV_HD bool tg_decode(const uint8_t* blob, uint64_t vb, uint64_t ve, uint64_t& pb, uint64_t& pe) {
  bool is_list;
  uint64_t lb, le;
  if (!rlp_item(blob, vb, ve, is_list, lb, le) || !is_list || le != ve) return false;
  return rlp_item(blob, lb, le, is_list, pb, pe) && !is_list;   // an empty list has no first item
}

struct TgResult {
  uint32_t status;   // SP_OK, SP_NODE_MISSING or SP_MALFORMED
  uint32_t found;    // 1: the key has a value, blob[beg, beg + len)
  uint64_t beg, len;
};

// The read of one (root, key).
PV_HD void tg_get(const uint8_t* blob, const uint64_t* beg, const uint64_t* end, const uint32_t* dig,
                  const uint32_t* table, uint32_t slots, uint32_t n_nodes, const uint32_t root[8], const uint8_t* key,
                  uint64_t klen, bool decode, TgResult& o) {
  SgResult r;
  sg_walk_t<false>(blob, beg, end, dig, table, slots, n_nodes, root, key, klen, nullptr, 0, r);
  o.status = r.status;
  o.found = 0;
  o.beg = o.len = 0;
  if (r.status != SP_OK || r.val_len == 0) return;   // val_len == 0: proven absent
  if (!decode) {
    o.found = 1;
    o.beg = r.val_beg;
    o.len = r.val_len;
    return;
  }
  uint64_t pb, pe;
  if (!tg_decode(blob, r.val_beg, r.val_beg + r.val_len, pb, pe)) {
    o.status = SP_MALFORMED;
    return;
  }
  o.found = 1;
  o.beg = pb;
  o.len = pe - pb;
}

// Member `lane` of the group that gathers value q: out[val_off[q] ..] <- blob[src[q] ..].
// Nothing is written for a value whose offsets run backwards.
PV_HD void tg_copy_group(const uint8_t* blob, const uint64_t* src, const uint64_t* val_off, uint64_t q, uint32_t lane,
                         uint8_t* out) {
  const uint64_t o = val_off[q], e = val_off[q + 1];
  if (e <= o) return;
  const uint8_t* from = blob + src[q];
  for (uint64_t x = lane; x < e - o; x += TG_GROUP) out[o + x] = from[x];
}

}  // namespace pv
