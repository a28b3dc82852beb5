// Batch construction of a state trie, shared by device and host: the write side
// of pv_trie_store.h.  The reference computes a state root with one
// PruningState.set per key (state/pruning_state.py:60-61 -> Trie.update,
// state/trie/pruning_trie.py:1006-1027).  A Merkle-Patricia root depends on the
// final key/value set alone, so the result of any sequence of sets is one batch
// computation over the sorted distinct keys.
//
// Input.  n keys, strictly increasing bytewise with a proper prefix first (the
// nibble order of bin_to_nibbles), and n non-empty values, the bytes the trie
// stores (rlp([v]) from PruningState.set).
//
// Structure, from the adjacent-pair nibble LCPs alone.  h[i] = 1 + LCP(key i-1,
// key i) for 0 < i < n and h[0] = h[n] = 0, so every search below ends at a
// sentinel.  A branch at nibble depth d is a maximal run of keys that share d
// nibbles and split at nibble d: an "LCP interval" of value d.  Its
// representative is the leftmost position p of the run with h[p] = d + 1, so
// position p is a representative iff the nearest j < p with h[j] <= h[p] has
// h[j] < h[p]; that j is the run's first key l.  The run ends before r1, the
// nearest position after p with h[r1] < h[p].  The node above is the branch at
// depth max(h[l], h[r1]) - 1 (none for 0: this is the top), reached through the
// slot nibble of key l at that depth; nibbles between the slot and d make the
// extension above the branch.  A key equal to the run's common prefix (it can
// only be key l) is the branch's value (item 16) and has no leaf.  Every other
// key is a leaf under the branch at depth max(h[i], h[i+1]) - 1.  The "nearest
// position below a threshold" searches run on a 64-ary min tree over h (level
// k + 1 entry j = min of level k entries 64 j .. 64 j + 63): at most 64 steps
// per level up and per level down, instead of a scan of up to n positions.
//
// Entities.  Position i owns three node slots: e = 3 i the extension above the
// branch at i, 3 i + 1 that branch, 3 i + 2 the leaf of key i.  lvl[e] is the
// nibble depth at which the node starts (TB_VOID: no such node); a child starts
// strictly deeper than its parent.  A child registers itself in
// child[16 p + slot] = e + 1 of its parent branch p; each entry has exactly one
// writer, so no atomics order anything.
//
// Encoding, bottom-up by level.  A node's length needs its children's lengths
// only through "under 32 bytes: embedded, else a 33-byte hash reference", so a
// size pass per level (deepest first) fixes every length before a byte is
// written.  Emitted are the nodes of >= 32 bytes and the root whatever its
// length (_encode_node(..., is_root=True), pruning_trie.py:334-344).  Two
// exclusive scans in entity order give each emitted node its index and its byte
// offset, so order and bytes do not depend on the order lanes ran in.  The write
// pass per level (deepest first) writes each node (emitted: into the blob;
// embedded: into a 32-byte cell the parent copies from) and hashes the emitted
// ones in place with sha3_256_msg.  Two byte-identical nodes are both emitted.
//
// Bounds.  Every loop is bounded by a key length, 64 (a tree block), the level
// count, 16 slots, 9 header bytes or a length fixed by the size pass; no lane
// keeps an array it indexes at run time (digests go straight to global memory).
// The blob keeps the over-read contract of pv_sha3.h: 4-byte aligned base and
// 16 readable bytes after the last node.
//
// A merged item list (pv_trie_update.h) instead of plain keys: with knib set,
// path i has knib[i] nibbles (any parity; an odd path ends in a zero pad nibble)
// and tb_lcp_one compares by nibble; with kind set, kind[i] == 1 marks a carried
// child reference.  Such an item is never a branch value and a prefix of no
// other path (tb_lcp_one refuses it).  Its entity 3 i + 2 is, with no nibble left
// below its slot, the reference itself: elen is the reference's length, nothing
// is emitted or hashed and tb_put_ref copies the payload bytes; with nibbles left
// it is an extension node over them with the payload as its second item.  With
// both null every routine does what it did for plain keys.
//
// The host twin is these routines called in index order.
#pragma once
#include <stdint.h>

#include "pv_sha3.h"
#include "pv_trie_store.h"

namespace pv {

constexpr uint32_t TB_VOID = 0xffffffffu;
constexpr uint64_t TB_MAX_KEYS = 1ull << 28;       // 3 n entity ids + 1 and positions fit 32 bits
constexpr uint64_t TB_MAX_KEY_BYTES = 1ull << 20;
constexpr uint64_t TB_MAX_VAL_BYTES = 1ull << 30;  // a node's length fits 32 bits
constexpr uint32_t TB_MAX_LEVELS = 8;              // 64-ary levels over n + 1 <= 2^28 + 1 entries: 6

enum : uint32_t { TB_BAD_ORDER = 1, TB_BAD_VALUE = 2, TB_BAD_OFFSET = 4 };

struct TbCtx {
  const uint8_t* key_blob;
  const uint64_t* key_off;
  const uint8_t* val_blob;
  const uint64_t* val_off;
  uint64_t n;
  uint32_t* tree;          // the min tree; level 0 is h[0 .. n]
  const uint64_t* lvoff;   // level k = tree[lvoff[k] .. lvoff[k + 1]), k < nlv; the last level has one entry
  uint32_t nlv;
  uint32_t* child;         // 16 n: entity + 1 under slot s of the branch at position p, 0 = blank
  uint32_t* lvl;           // 3 n
  uint32_t* aux;           // 3 n: extension -> the key its path is read from; branch -> value key + 1, 0 = none
  uint32_t* elen;          // 3 n: the node's RLP length
  uint64_t* off;           // 3 n + 1: emitted length, scanned to the byte offset
  uint64_t* idx;           // 3 n + 1: 1 if emitted, scanned to the output index
  uint8_t* inl;            // 32 x 3 n: the RLP of the nodes under 32 bytes
  const uint32_t* root_e;  // the root's entity
  uint8_t* out_blob;
  uint64_t* node_off;
  uint32_t* dig;           // 8 words per emitted node
  // A merged item list (pv_trie_update.h) instead of plain keys; both null for a plain build.
  const uint32_t* knib;    // n: the nibble length of path i (an odd path ends in a zero pad nibble); null: 2 per byte
  const uint8_t* kind;     // n: 1 = the value of item i is a child reference carried as it is (TU_SUBTREE); null: none
  // The batch check of pv_state_apply alone.  Non-null: tb_lcp_one admits an empty value (a removal) and
  // sets *empty_seen to 1 when it meets one (every writer stores the same word).  Null for every build.
  uint32_t* empty_seen;
};

// number of tree levels over n keys and their offsets (lvoff[0 .. nlv]); the words of the whole tree
inline uint32_t tb_tree_layout(uint64_t n, uint64_t lvoff[TB_MAX_LEVELS + 1]) {
  uint64_t size = n + 1, at = 0;
  uint32_t k = 0;
  lvoff[0] = 0;
  while (true) {
    at += size;
    lvoff[++k] = at;
    if (size == 1 || k == TB_MAX_LEVELS) break;
    size = (size + 63) / 64;
  }
  return k;
}

PV_HD uint64_t tb_knib(const TbCtx& c, uint64_t i) {
  return c.knib ? c.knib[i] : 2 * (c.key_off[i + 1] - c.key_off[i]);
}

// item i is a carried child reference
PV_HD bool tb_subtree(const TbCtx& c, uint64_t i) { return c.kind && c.kind[i] == 1; }

// entity e is a carried reference with no nibble left below its slot: the reference itself, no node
PV_HD bool tb_is_ref(const TbCtx& c, uint32_t e) { return c.kind && e % 3 == 2 && c.aux[e] != 0; }

// h[i], 0 <= i <= n, with the order check of the pair (i - 1, i) and the checks of value i
PV_HD uint32_t tb_lcp_one(const TbCtx& c, uint64_t i, uint32_t& bad) {
  bad = 0;
  if (i < c.n) {
    const uint64_t a = c.val_off[i], b = c.val_off[i + 1];
    if (b < a) bad |= TB_BAD_OFFSET;
    else if (b == a && c.empty_seen) *c.empty_seen = 1;
    else if (b == a || b - a > TB_MAX_VAL_BYTES || (tb_subtree(c, i) && b - a > 33)) bad |= TB_BAD_VALUE;
    const uint64_t ka = c.key_off[i], kb = c.key_off[i + 1];
    if (kb < ka || kb - ka > TB_MAX_KEY_BYTES) bad |= TB_BAD_OFFSET;
  }
  if (i == 0 || i == c.n) return 0;
  const uint64_t o0 = c.key_off[i - 1], o1 = c.key_off[i], o2 = c.key_off[i + 1];
  if (o1 < o0 || o2 < o1 || o1 - o0 > TB_MAX_KEY_BYTES || o2 - o1 > TB_MAX_KEY_BYTES) {
    bad |= TB_BAD_OFFSET;   // also flagged by the lanes that own these offsets; no key byte is read
    return 1;
  }
  const uint8_t *a = c.key_blob + o0, *b = c.key_blob + o1;
  if (c.knib) {   // paths of any parity, compared by nibble; a carried reference is a prefix of nothing
    const uint64_t na = c.knib[i - 1], nb = c.knib[i], nm = na < nb ? na : nb;
    if (na > 2 * (o1 - o0) || nb > 2 * (o2 - o1)) {
      bad |= TB_BAD_OFFSET;
      return 1;
    }
    uint64_t x = 0;
    while (x < nm && sp_nibble(a, x) == sp_nibble(b, x)) ++x;
    if (x == nm) {
      if (na >= nb || tb_subtree(c, i - 1)) bad |= TB_BAD_ORDER;
    } else if (sp_nibble(a, x) > sp_nibble(b, x)) {
      bad |= TB_BAD_ORDER;
    }
    return (uint32_t)(x + 1);
  }
  const uint64_t la = o1 - o0, lb = o2 - o1, m = la < lb ? la : lb;
  uint64_t k = 0;
  while (k < m && a[k] == b[k]) ++k;
  if (k == m) {
    if (la >= lb) bad |= TB_BAD_ORDER;   // equal, or key i a proper prefix of key i - 1
    return (uint32_t)(2 * k + 1);
  }
  if (a[k] > b[k]) bad |= TB_BAD_ORDER;
  return (uint32_t)(2 * k + ((a[k] >> 4) == (b[k] >> 4) ? 1 : 0) + 1);
}

// entry j of tree level lv >= 1
PV_HD void tb_min_one(const TbCtx& c, uint32_t lv, uint64_t j) {
  const uint32_t* lo = c.tree + c.lvoff[lv - 1];
  const uint64_t size = c.lvoff[lv] - c.lvoff[lv - 1];
  uint32_t m = 0xffffffffu;
  for (uint32_t t = 0; t < 64; ++t) {
    const uint64_t x = 64 * j + t;
    if (x < size && lo[x] < m) m = lo[x];
  }
  c.tree[c.lvoff[lv] + j] = m;
}

// the largest j <= i with h[j] < thr; thr >= 1 and h[0] = 0, so there is one
PV_HD uint64_t tb_prev_below(const TbCtx& c, uint64_t i, uint32_t thr) {
  uint64_t pos = i;
  uint32_t lv = 0;
  bool found = false;
  for (; lv < c.nlv; ++lv) {
    const uint32_t* L = c.tree + c.lvoff[lv];
    const uint64_t base = pos & ~63ull;
    uint64_t j = pos;
    for (uint32_t t = 0; t < 64; ++t) {
      if (L[j] < thr) {
        found = true;
        break;
      }
      if (j == base) break;
      --j;
    }
    if (found) {
      pos = j;
      break;
    }
    if (base == 0) return 0;
    pos = (base >> 6) - 1;   // the blocks before this one, one level up
  }
  if (!found) return 0;
  while (lv > 0) {
    --lv;
    const uint32_t* L = c.tree + c.lvoff[lv];
    const uint64_t size = c.lvoff[lv + 1] - c.lvoff[lv], lo = 64 * pos;
    uint64_t j = lo + 63 < size ? lo + 63 : size - 1;
    for (uint32_t t = 0; t < 64; ++t) {
      if (L[j] < thr || j == lo) break;
      --j;
    }
    pos = j;
  }
  return pos;
}

// the smallest j >= i with h[j] < thr (i <= n); thr >= 1 and h[n] = 0, so there is one
PV_HD uint64_t tb_next_below(const TbCtx& c, uint64_t i, uint32_t thr) {
  uint64_t pos = i;
  uint32_t lv = 0;
  bool found = false;
  for (; lv < c.nlv; ++lv) {
    const uint32_t* L = c.tree + c.lvoff[lv];
    const uint64_t size = c.lvoff[lv + 1] - c.lvoff[lv];
    if (pos >= size) return c.n;
    const uint64_t base = pos & ~63ull, last = base + 63 < size ? base + 63 : size - 1;
    uint64_t j = pos;
    for (uint32_t t = 0; t < 64; ++t) {
      if (L[j] < thr) {
        found = true;
        break;
      }
      if (j == last) break;
      ++j;
    }
    if (found) {
      pos = j;
      break;
    }
    pos = (base >> 6) + 1;   // the blocks after this one, one level up
  }
  if (!found) return c.n;
  while (lv > 0) {
    --lv;
    const uint32_t* L = c.tree + c.lvoff[lv];
    const uint64_t size = c.lvoff[lv + 1] - c.lvoff[lv], lo = 64 * pos;
    const uint64_t last = lo + 63 < size ? lo + 63 : size - 1;
    uint64_t j = lo;
    for (uint32_t t = 0; t < 64; ++t) {
      if (L[j] < thr || j == last) break;
      ++j;
    }
    pos = j;
  }
  return pos;
}

// the representative of the branch with h-value hd whose run holds key i
PV_HD uint64_t tb_branch_of(const TbCtx& c, uint64_t i, uint32_t hd) {
  const uint64_t j = tb_prev_below(c, i, hd);
  return tb_next_below(c, j + 1, hd + 1);
}

// The three entities of position i < n: levels, aux, the registration with the
// parent.  Returns the root's entity + 1 if it is one of them, else 0.
PV_HD uint32_t tb_struct_one(const TbCtx& c, uint64_t i) {
  const uint32_t* h = c.tree;
  const uint32_t hl = h[i], hr = h[i + 1];
  const uint32_t e0 = (uint32_t)(3 * i);
  uint32_t root = 0;
  uint32_t ll = TB_VOID;
  if (!(hr && (uint64_t)(hr - 1) == tb_knib(c, i))) {   // else: the value of the branch at i + 1
    const uint32_t ph = hl > hr ? hl : hr;
    ll = ph;
    if (ph == 0) {
      root = e0 + 3;
    } else {
      const uint64_t p = hr > hl ? i + 1 : tb_branch_of(c, i, ph);
      c.child[16 * p + sp_nibble(c.key_blob + c.key_off[i], ph - 1)] = e0 + 3;
    }
  }
  uint32_t le = TB_VOID, lb = TB_VOID, ae = 0, ab = 0;
  if (i >= 1) {
    const uint64_t l = tb_prev_below(c, i - 1, hl + 1);
    if (h[l] < hl) {
      const uint64_t r1 = tb_next_below(c, i + 1, hl);
      const uint32_t a = h[l], b = h[r1], ph = a > b ? a : b, d = hl - 1;
      lb = d;
      if (tb_knib(c, l) == d) ab = (uint32_t)l + 1;
      uint32_t top = e0 + 1;
      if (d > ph) {
        le = ph;
        ae = (uint32_t)l;
        top = e0;
      }
      if (ph == 0) {
        root = top + 1;
      } else {
        const uint64_t p = b > a ? r1 : tb_branch_of(c, l, ph);
        c.child[16 * p + sp_nibble(c.key_blob + c.key_off[l], ph - 1)] = top + 1;
      }
    }
  }
  c.lvl[e0] = le;
  c.lvl[e0 + 1] = lb;
  c.lvl[e0 + 2] = ll;
  c.aux[e0] = ae;
  c.aux[e0 + 1] = ab;
  c.aux[e0 + 2] = (ll != TB_VOID && tb_subtree(c, i) && tb_knib(c, i) == ll) ? 1u : 0u;
  return root;
}

// ---------------------------------------------------------------- RLP pieces
PV_HD uint8_t* tb_put_hdr(uint8_t* w, uint32_t base, uint64_t body) {
  const uint32_t hl = rlp_header_len(body);
  for (uint32_t k = 0; k < hl && k < 9; ++k) *w++ = rlp_header_byte(base, body, hl, k);
  return w;
}

// a byte string as an RLP item
PV_HD uint64_t tb_str_len(const uint8_t* s, uint64_t len) {
  if (len == 1 && s[0] < 0x80) return 1;
  return rlp_header_len(len) + len;
}

PV_HD uint8_t* tb_put_str(uint8_t* w, const uint8_t* s, uint64_t len) {
  if (!(len == 1 && s[0] < 0x80)) w = tb_put_hdr(w, 128, len);
  for (uint64_t k = 0; k < len; ++k) *w++ = s[k];
  return w;
}

// the hex-prefix path over nibbles [n0, n1) of key, as an RLP item (pack_nibbles)
PV_HD uint64_t tb_hp_len(uint64_t n0, uint64_t n1) {
  const uint64_t hb = (n1 - n0) / 2 + 1;
  return hb == 1 ? 1 : rlp_header_len(hb) + hb;   // one byte is a flag byte below 0x40: itself
}

PV_HD uint8_t* tb_put_hp(uint8_t* w, const uint8_t* key, uint64_t n0, uint64_t n1, bool leaf) {
  const uint64_t pn = n1 - n0, hb = pn / 2 + 1;
  const uint32_t odd = (uint32_t)(pn & 1), flags = (leaf ? 2u : 0u) + odd;
  if (hb > 1) w = tb_put_hdr(w, 128, hb);
  *w++ = (uint8_t)(16 * flags + (odd ? sp_nibble(key, n0) : 0));
  uint64_t x = n0 + odd;
  for (uint64_t k = 1; k < hb; ++k, x += 2) *w++ = (uint8_t)(16 * sp_nibble(key, x) + sp_nibble(key, x + 1));
  return w;
}

// a child reference: blank, the embedded node, or its hash
PV_HD uint32_t tb_ref_len(const TbCtx& c, uint32_t ch) {
  if (!ch) return 1;
  const uint32_t l = c.elen[ch - 1];
  return l >= 32 ? 33 : l;
}

PV_HD uint8_t* tb_put_ref(const TbCtx& c, uint8_t* w, uint32_t ch) {
  if (!ch) {
    *w++ = 0x80;
    return w;
  }
  const uint32_t e = ch - 1, l = c.elen[e];
  if (tb_is_ref(c, e)) {   // the carried bytes: 0xa0 and a hash, or an inline node
    const uint8_t* s = c.val_blob + c.val_off[e / 3];
    for (uint32_t k = 0; k < l && k < 33; ++k) *w++ = s[k];
    return w;
  }
  if (l >= 32) {
    *w++ = 0xa0;
    const uint32_t* d = c.dig + 8 * c.idx[e];
    for (uint32_t k = 0; k < 8; ++k) {
      const uint32_t v = d[k];
      *w++ = (uint8_t)v;
      *w++ = (uint8_t)(v >> 8);
      *w++ = (uint8_t)(v >> 16);
      *w++ = (uint8_t)(v >> 24);
    }
    return w;
  }
  const uint8_t* s = c.inl + 32 * (uint64_t)e;
  for (uint32_t k = 0; k < l && k < 32; ++k) *w++ = s[k];
  return w;
}

// ---------------------------------------------------------------- the nodes
// the payload length of entity e (a leaf, a branch or an extension)
PV_HD uint64_t tb_payload(const TbCtx& c, uint32_t e) {
  const uint64_t i = e / 3;
  const uint32_t k = e - 3 * (uint32_t)i;
  if (k == 2) {
    const uint64_t vo = c.val_off[i];
    if (tb_subtree(c, i)) return tb_hp_len(c.lvl[e], tb_knib(c, i)) + (c.val_off[i + 1] - vo);   // an extension
    return tb_hp_len(c.lvl[e], tb_knib(c, i)) + tb_str_len(c.val_blob + vo, c.val_off[i + 1] - vo);
  }
  if (k == 0) return tb_hp_len(c.lvl[e], c.tree[i] - 1) + tb_ref_len(c, e + 2);
  uint64_t body = 0;
  for (uint32_t s = 0; s < 16; ++s) body += tb_ref_len(c, c.child[16 * i + s]);
  const uint32_t a = c.aux[e];
  if (!a) return body + 1;
  const uint64_t vo = c.val_off[a - 1];
  return body + tb_str_len(c.val_blob + vo, c.val_off[a - 1 + 1] - vo);
}

// size pass: entity e (lvl[e] != TB_VOID, its children sized)
PV_HD void tb_size_one(const TbCtx& c, uint32_t e) {
  if (tb_is_ref(c, e)) {   // no node: its parent copies the reference, nothing is emitted
    const uint64_t i = e / 3;
    c.elen[e] = (uint32_t)(c.val_off[i + 1] - c.val_off[i]);
    return;
  }
  const uint64_t body = tb_payload(c, e);
  const uint64_t len = rlp_header_len(body) + body;
  const bool emit = len >= 32 || e == *c.root_e;
  c.elen[e] = (uint32_t)len;
  c.off[e] = emit ? len : 0;
  c.idx[e] = emit ? 1 : 0;
}

// write pass: entity e (its children written and hashed, off and idx scanned)
PV_HD void tb_emit_one(const TbCtx& c, uint32_t e) {
  if (tb_is_ref(c, e)) return;
  const uint64_t i = e / 3;
  const uint32_t k = e - 3 * (uint32_t)i;
  const uint32_t len = c.elen[e];
  const bool emit = len >= 32 || e == *c.root_e;
  uint8_t* const dst = emit ? c.out_blob + c.off[e] : c.inl + 32 * (uint64_t)e;
  uint32_t hl = 1;   // the list header's length: the one hl with header_len(len - hl) == hl
  for (uint32_t t = 1; t <= 9 && t < len; ++t)
    if (rlp_header_len(len - t) == t) {
      hl = t;
      break;
    }
  uint8_t* w = tb_put_hdr(dst, 192, len - hl);
  if (k == 2) {
    const uint64_t vo = c.val_off[i];
    const bool sub = tb_subtree(c, i);
    w = tb_put_hp(w, c.key_blob + c.key_off[i], c.lvl[e], tb_knib(c, i), !sub);
    if (sub) {
      const uint64_t vl = c.val_off[i + 1] - vo;
      for (uint64_t t = 0; t < vl && t < 33; ++t) *w++ = c.val_blob[vo + t];
    } else {
      w = tb_put_str(w, c.val_blob + vo, c.val_off[i + 1] - vo);
    }
  } else if (k == 0) {
    w = tb_put_hp(w, c.key_blob + c.key_off[c.aux[e]], c.lvl[e], c.tree[i] - 1, false);
    w = tb_put_ref(c, w, e + 2);
  } else {
    for (uint32_t s = 0; s < 16; ++s) w = tb_put_ref(c, w, c.child[16 * i + s]);
    const uint32_t a = c.aux[e];
    if (!a) {
      *w++ = 0x80;
    } else {
      const uint64_t vo = c.val_off[a - 1];
      w = tb_put_str(w, c.val_blob + vo, c.val_off[a - 1 + 1] - vo);
    }
  }
  if (emit) {
    const uint64_t id = c.idx[e];
    c.node_off[id] = c.off[e];
    sha3_256_msg(c.dig + 8 * id, dst, len);
  }
}

}  // namespace pv
