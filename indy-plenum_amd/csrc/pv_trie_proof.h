// Patricia-trie state-proof check for one query, shared by device and host:
// Trie.verify_spv_proof (state/trie/pruning_trie.py:1100-1119) over nodes that
// are already hashed.  It restates Trie._get (:376-407) with _decode_to_node
// (:346-353), unpack_to_nibbles (:163-177) and _get_node_type (:359-374)
// directly on RLP bytes; the lenient, bounds-checked length decoding follows
// state/util/fast_rlp.py:47-71 (no canonical-form checks).
//
// A query is (proof, key, expected encoded value).  The proof is a set of
// nodes: byte ranges [node_beg[j], node_end[j]) of one blob, each holding one
// RLP list, with their SHA3-256 digests (8 little-endian words each).  The walk
// starts at the node whose digest equals the root and descends by the key's
// nibbles:
//   17 items  branch: key exhausted -> item 16, else the item at the next nibble
//   2 items   leaf (terminator flag in the first nibble of item 0) or extension
//   child     empty string -> blank; list -> an inline node, walked in place;
//             32-byte string -> the proof node with that digest (linear scan,
//             first word first: the nodes are an unordered set, duplicates and
//             unrelated nodes are legal), absent -> SP_NODE_MISSING; any other
//             string length -> SP_NODE_MISSING (the reference's db lookup fails)
// The result bytes are compared with the expected value; blank and "value is
// None" are both the empty string, so a valid proof of absence is SP_OK.
//
// Bounds: every length is checked against the end of the enclosing node before
// a byte is read; an overrun is SP_MALFORMED.  A step that consumes no nibble
// and does not end the walk (an extension with an empty path) is SP_MALFORMED,
// so a walk takes at most 2 * len(key) + 1 steps; the loop carries that bound.
//
// Malformed nodes: a node reached from a trusted root is malformed only if
// someone found a SHA3 preimage, so for such inputs the rule is "False, never
// read out of bounds"; parity with the exception pyrlp would raise does not
// apply.  (Item 0 that is a list or empty, a value that is a list, an item
// count other than 2 or 17, bytes after the list: all SP_MALFORMED.)
#pragma once
#include <stdint.h>

#ifndef PV_HD
#define PV_HD __host__ __device__ __forceinline__
#endif

namespace pv {

enum : uint32_t { SP_OK = 0, SP_VALUE_MISMATCH = 1, SP_NODE_MISSING = 2, SP_MALFORMED = 3 };

// SHA3-256(0x80): BLANK_ROOT (pruning_trie.py:206-207), as little-endian words
PV_HD bool sp_is_blank_root(const uint32_t r[8]) {
  return r[0] == 0xa47120bcu && r[1] == 0x286f84deu && r[2] == 0x7f440257u && r[3] == 0x16dd8925u &&
         r[4] == 0x97e07836u && r[5] == 0x0d1b8a2au && r[6] == 0xd54eb028u && r[7] == 0x7f5494c0u;
}

// One RLP item starting at pos inside [pos, lim): its payload [pbeg, pend) and
// whether it is a list.  false when the header or the payload overruns lim.
PV_HD bool rlp_item(const uint8_t* b, uint64_t pos, uint64_t lim, bool& is_list, uint64_t& pbeg, uint64_t& pend) {
  if (pos >= lim) return false;
  const uint32_t b0 = b[pos];
  uint32_t ll = 0;
  uint64_t len = 0;
  if (b0 < 128) {   // the byte is its own payload
    is_list = false;
    pbeg = pos;
    pend = pos + 1;
    return true;
  } else if (b0 < 184) {
    is_list = false;
    len = b0 - 128;
  } else if (b0 < 192) {
    is_list = false;
    ll = b0 - 183;
  } else if (b0 < 248) {
    is_list = true;
    len = b0 - 192;
  } else {
    is_list = true;
    ll = b0 - 247;
  }
  if (ll > lim - pos - 1) return false;   // ll <= 8
  for (uint32_t i = 0; i < ll; ++i) len = (len << 8) | b[pos + 1 + i];
  pbeg = pos + 1 + ll;
  if (len > lim - pbeg) return false;
  pend = pbeg + len;
  return true;
}

// nibble i of a byte string starting at p
PV_HD uint32_t sp_nibble(const uint8_t* p, uint64_t i) {
  const uint32_t v = p[i >> 1];
  return (i & 1) ? (v & 15u) : (v >> 4);
}

// index in [first, last) of the proof node whose digest is t, or `last`
PV_HD uint64_t sp_find(const uint32_t* dig, uint64_t first, uint64_t last, const uint32_t t[8]) {
  for (uint64_t j = first; j < last; ++j) {
    const uint32_t* d = dig + 8 * j;
    if (d[0] != t[0]) continue;
    if (d[1] == t[1] && d[2] == t[2] && d[3] == t[3] && d[4] == t[4] && d[5] == t[5] && d[6] == t[6] &&
        d[7] == t[7])
      return j;
  }
  return last;
}

PV_HD uint32_t sp_compare(const uint8_t* a, uint64_t alen, const uint8_t* v, uint64_t vlen) {
  if (alen != vlen) return SP_VALUE_MISMATCH;
  uint32_t diff = 0;
  for (uint64_t i = 0; i < alen; ++i) diff |= (uint32_t)(a[i] ^ v[i]);
  return diff ? SP_VALUE_MISMATCH : SP_OK;
}

// The walk.  blob + node_beg / node_end / dig describe every node of the call;
// this query's proof is nodes first .. last - 1.
PV_HD uint32_t sp_verify(const uint8_t* blob, const uint64_t* node_beg, const uint64_t* node_end, const uint32_t* dig,
                         uint64_t first, uint64_t last, const uint32_t root[8], const uint8_t* key, uint64_t klen,
                         const uint8_t* val, uint64_t vlen) {
  if (sp_is_blank_root(root)) return vlen == 0 ? SP_OK : SP_VALUE_MISMATCH;
  uint64_t j = sp_find(dig, first, last, root);
  if (j == last) return SP_NODE_MISSING;
  uint64_t cb = node_beg[j], ce = node_end[j];   // the current node's RLP
  const uint64_t total = 2 * klen;
  uint64_t nib = 0;                              // key nibbles consumed
  for (uint64_t step = 0; step <= total; ++step) {
    bool is_list;
    uint64_t pb, pe;
    if (!rlp_item(blob, cb, ce, is_list, pb, pe) || !is_list || pe != ce) return SP_MALFORMED;
    // the items: extents of item 0, item 1 and the item a branch would take
    const uint32_t sel = nib < total ? sp_nibble(key, nib) : 16u;
    uint64_t i0b = 0, i0e = 0, i1s = 0, i1b = 0, i1e = 0, sls = 0, slb = 0, sle = 0;
    bool i0l = false, i1l = false, sll = false;
    uint32_t count = 0;
    uint64_t pos = pb;
    while (pos < pe) {
      if (count == 17) return SP_MALFORMED;
      bool il;
      uint64_t ib, ie;
      if (!rlp_item(blob, pos, pe, il, ib, ie)) return SP_MALFORMED;
      if (count == 0) {
        i0b = ib;
        i0e = ie;
        i0l = il;
      }
      if (count == 1) {
        i1s = pos;
        i1b = ib;
        i1e = ie;
        i1l = il;
      }
      if (count == sel) {
        sls = pos;
        slb = ib;
        sle = ie;
        sll = il;
      }
      pos = ie;
      ++count;
    }
    uint64_t rs, rb, re;   // the child reference (or, with `done`, the result): start, payload
    bool rl, done = false;
    if (count == 17) {
      rs = sls;
      rb = slb;
      re = sle;
      rl = sll;
      if (nib == total) done = true;
      else ++nib;
    } else if (count == 2) {
      if (i0l || i0e == i0b) return SP_MALFORMED;
      const uint8_t* p = blob + i0b;
      const uint32_t flags = p[0] >> 4;
      const uint32_t odd = flags & 1u;
      const uint64_t pn = 2 * (i0e - i0b - 1) + odd;   // path nibbles
      const uint64_t skip = 2 - odd;
      const uint64_t left = total - nib;
      const bool leaf = (flags & 2u) != 0;
      if (!leaf && pn == 0) return SP_MALFORMED;
      bool match = leaf ? pn == left : pn <= left;
      if (match) {
        uint32_t diff = 0;
        for (uint64_t i = 0; i < pn; ++i) diff |= sp_nibble(p, skip + i) ^ sp_nibble(key, nib + i);
        match = diff == 0;
      }
      if (!match) return vlen == 0 ? SP_OK : SP_VALUE_MISMATCH;   // blank
      rs = i1s;
      rb = i1b;
      re = i1e;
      rl = i1l;
      if (leaf) done = true;
      else nib += pn;
    } else {
      return SP_MALFORMED;
    }
    if (done) {
      if (rl) return SP_MALFORMED;
      return sp_compare(blob + rb, re - rb, val, vlen);
    }
    if (rl) {   // an inline node: its RLP is the item itself
      cb = rs;
      ce = re;
      continue;
    }
    const uint64_t rlen = re - rb;
    if (rlen == 0) return vlen == 0 ? SP_OK : SP_VALUE_MISMATCH;   // blank
    if (rlen != 32) return SP_NODE_MISSING;
    uint32_t t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint8_t* q = blob + rb + 4 * k;
      t[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    }
    j = sp_find(dig, first, last, t);
    if (j == last) return SP_NODE_MISSING;
    cb = node_beg[j];
    ce = node_end[j];
  }
  return SP_MALFORMED;
}

// The top-level items of one RLP list rlp[0 .. len), in place: item k is
// rlp[item_beg[k] .. item_end[k]) including its own header.  false when the
// input is not one list whose items end exactly at its end, or holds more
// than cap items (*count then holds the number seen so far).
PV_HD bool rlp_split_list(const uint8_t* rlp, uint64_t len, uint64_t* item_beg, uint64_t* item_end, uint64_t cap,
                          uint64_t* count) {
  *count = 0;
  bool is_list;
  uint64_t pb, pe;
  if (!rlp_item(rlp, 0, len, is_list, pb, pe) || !is_list || pe != len) return false;
  uint64_t pos = pb, k = 0;
  while (pos < pe) {
    bool il;
    uint64_t ib, ie;
    if (!rlp_item(rlp, pos, pe, il, ib, ie)) return false;
    if (k == cap) return false;
    item_beg[k] = pos;
    item_end[k] = ie;
    pos = ie;
    *count = ++k;
  }
  return true;
}

}  // namespace pv
