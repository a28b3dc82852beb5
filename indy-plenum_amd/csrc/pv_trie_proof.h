// Patricia-trie state-proof check for one query, shared by device and host:
// Trie.verify_spv_proof (state/trie/pruning_trie.py:1100-1119) over nodes that
// are already hashed.  It restates Trie._get (:376-407) directly on RLP bytes;
// the node grammar, the parser and the step by the key's nibbles are in
// pv_trie_node.h.
//
// A query is (proof, key, expected encoded value).  The proof is a set of
// nodes: byte ranges [node_beg[j], node_end[j]) of one blob, each holding one
// RLP list, with their SHA3-256 digests (8 little-endian words each).  The walk
// starts at the node whose digest equals the root and descends by the key's
// nibbles (tn_step).  A 32-byte child is the proof node with that digest
// (linear scan, first word first: the nodes are an unordered set, duplicates
// and unrelated nodes are legal), absent -> SP_NODE_MISSING; any other string
// length -> SP_NODE_MISSING (the reference's db lookup fails).
// The result bytes are compared with the expected value; blank and "value is
// None" are both the empty string, so a valid proof of absence is SP_OK.
//
// Bounds: an overrun is SP_MALFORMED.  A step that consumes no nibble and does
// not end the walk is SP_MALFORMED, so a walk takes at most 2 * len(key) + 1
// steps; the loop carries that bound.
//
// Malformed nodes: a node reached from a trusted root is malformed only if
// someone found a SHA3 preimage, so for such inputs the rule is "False, never
// read out of bounds"; parity with the exception pyrlp would raise does not
// apply.  (Item 0 that is a list or empty, a value that is a list, an item
// count other than 2 or 17, bytes after the list: all SP_MALFORMED.)
#pragma once
#include <stdint.h>

#include "pv_trie_node.h"

namespace pv {

enum : uint32_t { SP_OK = 0, SP_VALUE_MISMATCH = 1, SP_NODE_MISSING = 2, SP_MALFORMED = 3 };

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
    uint64_t ob, oe;
    uint32_t t[8];
    switch (tn_step(blob, cb, ce, key, total, nib, ob, oe, t)) {
      case TN_MALFORMED: return SP_MALFORMED;
      case TN_ABSENT: return vlen == 0 ? SP_OK : SP_VALUE_MISMATCH;   // blank
      case TN_VALUE: return sp_compare(blob + ob, oe - ob, val, vlen);
      case TN_MISSING: return SP_NODE_MISSING;
      case TN_INLINE:   // walked in place
        cb = ob;
        ce = oe;
        continue;
      default: break;   // TN_HASHED
    }
    j = sp_find(dig, first, last, t);
    if (j == last) return SP_NODE_MISSING;
    cb = node_beg[j];
    ce = node_end[j];
  }
  return SP_MALFORMED;
}

}  // namespace pv
