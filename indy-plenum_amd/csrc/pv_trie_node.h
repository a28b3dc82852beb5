// The bytes of a Patricia-trie node, shared by device and host: the one place
// that parses them.  The five state walks (sp_verify, sg_walk, tp_visit, tu_open,
// tu_walk_t) share this parser, not a policy: what each answers on a node that
// parses here but is no canonical trie node stays with the walk.
//
// Grammar.  A node is one RLP list whose payload fills its byte range exactly
// (_decode_to_node, state/trie/pruning_trie.py:346-353; _get_node_type
// :359-374); the lenient, bounds-checked length decoding follows
// state/util/fast_rlp.py:47-71 (no canonical-form checks).
//   17 items  branch: items 0 .. 15 are children, item 16 is a value
//   2 items   item 0 is a non-empty string in hex-prefix form
//             (unpack_to_nibbles :163-177): its first nibble holds the flags,
//             1 = an odd number of path nibbles (they start at nibble 1, else at
//             nibble 2), 2 = a leaf, whose item 1 is a value; otherwise an
//             extension, whose item 1 is its child
//   child     empty string: blank; a list: an inline node, its RLP is the item
//             itself; a 32-byte string: the SHA3-256 of a stored node
//
// Bounds.  No length is read before it is checked against the enclosing node:
// rlp_item refuses a header or a payload that overruns its limit, and the scan
// hands out only extents that passed it.  A node with an 18th item, an item
// that overruns the list, or bytes after the list does not scan.
//
// The scan's result is a struct of scalars (four extents and a count): no lane
// keeps an array it indexes at run time, and a caller that ignores an extent
// leaves the compiler free to drop it.  Walks that need all sixteen children
// (tp_visit, tu_walk_t) scan once for the shape and then loop over rlp_item.
#pragma once
#include <stdint.h>

#ifndef PV_HD
#define PV_HD __host__ __device__ __forceinline__
#endif

namespace pv {

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

// length (1 .. 9) of the RLP header over a payload of `body` bytes ...
PV_HD uint32_t rlp_header_len(uint64_t body) {
  if (body < 56) return 1;
  uint32_t ll = 0;
  for (uint64_t v = body; v; v >>= 8) ++ll;
  return 1 + ll;
}

// ... and its byte k < hl (hl = that length); base 128: a string, 192: a list.
// No array, so that one lane per byte can write it.
PV_HD uint8_t rlp_header_byte(uint32_t base, uint64_t body, uint32_t hl, uint32_t k) {
  if (hl == 1) return (uint8_t)(base + body);
  if (k == 0) return (uint8_t)(base + 55 + (hl - 1));
  return (uint8_t)(body >> (8 * (hl - 1 - k)));
}

// the 32 bytes at q as a digest: eight little-endian words, as k_sha3_256 writes them
PV_HD void tn_load_ref(const uint8_t* q, uint32_t t[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k, q += 4)
    t[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
}

// One item of a node: it starts at s (its header) and its payload is [b, e).
struct TnItem {
  uint64_t s, b, e;
  bool l;   // a list
};

// What one pass over a node's items keeps.  An item the node does not have is
// all zero: an empty string.
struct TnScan {
  uint64_t pb, pe;   // the list's payload
  uint32_t count;    // items, at most 17; the callers test it for 2 or 17
  TnItem i0, i1, sel, i16;
};

constexpr uint32_t TN_NO_SLOT = 0xffffffffu;   // a `sel` that selects nothing

// Scan the node blob[cb, ce), keeping item 0, item 1, item `sel` and item 16.
// false: not a list that fills its range, an item that overruns it or an 18th item.
PV_HD bool tn_scan(const uint8_t* blob, uint64_t cb, uint64_t ce, uint32_t sel, TnScan& n) {
  n = TnScan{};
  bool is_list;
  uint64_t pb, pe;
  if (!rlp_item(blob, cb, ce, is_list, pb, pe) || !is_list || pe != ce) return false;
  n.pb = pb;
  n.pe = pe;
  uint32_t count = 0;
  uint64_t pos = pb;
  while (pos < pe) {
    bool il;
    uint64_t ib, ie;
    if (count == 17 || !rlp_item(blob, pos, pe, il, ib, ie)) return false;
    const TnItem it{pos, ib, ie, il};
    if (count == 0) n.i0 = it;
    if (count == 1) n.i1 = it;
    if (count == sel) n.sel = it;
    if (count == 16) n.i16 = it;
    pos = ie;
    ++count;
  }
  n.count = count;
  return true;
}

// The hex-prefix path in item 0 of a two-item node: pn nibbles of p from nibble `skip`.
struct TnPath {
  const uint8_t* p;
  uint64_t skip, pn;
  bool leaf;
};

// false: item 0 is a list or empty.  An extension over no nibble (pn == 0, not
// a leaf) decodes; the callers refuse it where their rule says so.
PV_HD bool tn_path(const uint8_t* blob, const TnItem& i0, TnPath& h) {
  if (i0.l || i0.e == i0.b) return false;
  h.p = blob + i0.b;
  const uint32_t flags = h.p[0] >> 4, odd = flags & 1u;
  h.pn = 2 * (i0.e - i0.b - 1) + odd;
  h.skip = 2 - odd;
  h.leaf = (flags & 2u) != 0;
  return true;
}

// One step of the descent by a key's nibbles (Trie._get, pruning_trie.py:376-407),
// for the walks that only read: sp_verify and sg_walk.
enum : uint32_t {
  TN_MALFORMED,   // the node does not parse, or breaks a rule below
  TN_ABSENT,      // proven absent: a blank child, or a path that leaves the key
  TN_VALUE,       // the key's value is blob[ob, oe) (empty: a branch without a value)
  TN_MISSING,     // a child reference that is neither blank, a list nor 32 bytes: no stored node has it
  TN_HASHED,      // the child is the stored node with digest t
  TN_INLINE       // the child is the inline node blob[ob, oe)
};

// The node blob[cb, ce) with `nib` of the key's `total` nibbles consumed; nib
// advances past the nibbles this node takes.  An extension over no nibble
// consumes nothing and ends nothing: TN_MALFORMED, so a walk takes at most
// total + 1 steps.  A value that is a list is TN_MALFORMED.
PV_HD uint32_t tn_step(const uint8_t* blob, uint64_t cb, uint64_t ce, const uint8_t* key, uint64_t total,
                       uint64_t& nib, uint64_t& ob, uint64_t& oe, uint32_t t[8]) {
  TnScan n;
  if (!tn_scan(blob, cb, ce, nib < total ? sp_nibble(key, nib) : 16u, n)) return TN_MALFORMED;
  TnItem r;   // the child reference or, with `done`, the value
  bool done = false;
  if (n.count == 17) {
    r = n.sel;
    if (nib == total) done = true;
    else ++nib;
  } else if (n.count == 2) {
    TnPath h;
    if (!tn_path(blob, n.i0, h) || (!h.leaf && h.pn == 0)) return TN_MALFORMED;
    const uint64_t left = total - nib;
    bool match = h.leaf ? h.pn == left : h.pn <= left;
    if (match) {
      uint32_t diff = 0;
      for (uint64_t i = 0; i < h.pn; ++i) diff |= sp_nibble(h.p, h.skip + i) ^ sp_nibble(key, nib + i);
      match = diff == 0;
    }
    if (!match) return TN_ABSENT;
    r = n.i1;
    if (h.leaf) done = true;
    else nib += h.pn;
  } else {
    return TN_MALFORMED;
  }
  ob = r.b;
  oe = r.e;
  if (done) return r.l ? TN_MALFORMED : TN_VALUE;
  if (r.l) {
    ob = r.s;
    return TN_INLINE;
  }
  if (r.e == r.b) return TN_ABSENT;
  if (r.e - r.b != 32) return TN_MISSING;
  tn_load_ref(blob + r.b, t);
  return TN_HASHED;
}

}  // namespace pv
