// Sets applied to a committed root, shared by device and host: the merge in
// front of pv_trie_build.h.  The reference applies a 3PC batch with one
// PruningState.set per key (state/pruning_state.py:60-61 -> Trie.update,
// state/trie/pruning_trie.py:1006-1027), each rewriting the path from the root
// to one leaf.  Here the batch is one computation: the old trie at root R (in a
// resident store, pv_trie_store.h) and n sorted batch keys are merged into one
// sorted list of ITEMS, and the builder runs over that list.
//
// Items.  A nibble path of any parity and a payload.  TU_VALUE: the payload is
// a value as the trie stores it.  TU_SUBTREE: the payload is a child reference
// of the old trie kept as it is (0xa0 + 32 hash bytes, or the RLP of an inline
// node under 32 bytes): a whole subtree no batch key enters, which the builder
// puts back without looking inside.
//
// The walk.  One lane per batch key K_j walks from R as sg_walk does (hashed
// children through ts_find, inline children in place) and carries what it
// passes.  h[j] = 1 + LCP(K_{j-1}, K_j) in nibbles (h[0] = h[n] = 0, from
// tb_lcp_one over the batch).  At a node that starts at depth D, `first` means
// h[j] <= D (the previous key is not in the run of keys that visit this node)
// and `last` means h[j + 1] <= D.
//   Branch.  Its value, if `first` and len(K_j) != D, goes BEFORE.  With
//   s = K_j[D] (-1 at the key's end) and s_prev = K_{j-1}[D] (-1 if `first` or
//   K_{j-1} ends here), the non-blank slots s_prev < t < s go BEFORE, and, if
//   `last`, the non-blank slots t > s go AFTER.  The walk descends into slot s.
//   Leaf or extension with path P, Q = K_j[:D] + P.  A leaf with Q == K_j is
//   overwritten; an extension with Q a prefix of K_j is dissolved (the walk
//   goes on below it).  Otherwise the leaf's value or the extension's child
//   reference is an item at path Q: BEFORE if Q < K_j and (`first`, or
//   K_{j-1} < Q without K_{j-1} absorbing Q, see tu_cmp); AFTER if `last` and
//   Q > K_j.
// The lane's output is its BEFORE items in walk order, VALUE(K_j), then its
// AFTER groups, deepest node first.  Concatenated in key order this is strictly
// increasing and prefix-consistent with no sort and no atomic: the order is
// fixed by the inputs alone.
//
// Two passes.  tu_walk in count mode gives each key its number of items, path
// bytes and payload bytes; three exclusive scans give each key its ranges; the
// write mode walks again and fills them.  An AFTER group is placed from the
// range's end backwards (its size is known from the node alone), so the deepest
// group ends up first without a stack.
//
// Bounds.  Every loop is bounded by a key length, a path length checked against
// its node, 17 items or 33 reference bytes; the nodes are read through the
// parser of pv_trie_node.h (tn_scan, tn_path); no lane keeps an array it
// indexes at run time.  A missing or malformed node gives the key a PV_SP_* status and the
// caller refuses the whole call.
//
// Removals (tu_walk_t<true>, behind pv_state_apply).  A batch item with an empty
// value removes its key: PruningState.remove (state/pruning_state.py:84-85 ->
// Trie.delete, state/trie/pruning_trie.py:683-848), the one trie operation that
// restructures upward.  The lane of a removed key walks and carries as above,
// emits no VALUE(K_j), and OPENS every child reference it carries from a branch
// slot at path Q (tu_open: a hashed reference through ts_find, an inline node in
// place).  A branch: the item stays SUBTREE at Q.  A leaf with path P: VALUE at
// Q + P with the leaf's value.  An extension with path P: SUBTREE at Q + P with
// the extension's child reference.  The builder turns a SUBTREE with nibbles left
// below its slot into an extension over its payload, which is canonical only over
// a branch; nibbles are left only where the old branch above the child collapsed,
// and a branch collapses only if every batch key that visits it is a removal (a
// set leaves a VALUE there), so every child that can end up alone was carried by
// a removal lane and is in its canonical item form.  Where nothing collapses the
// opened item re-encodes to the bytes it had.  The child of an extension is
// carried unopened: in a trie the reference wrote it is a branch.  Lanes of set
// keys carry references unopened.  Count mode opens too (path and payload sizes
// depend on it), and so does the sizing pass of an AFTER group.
//
// The host twin is tu_walk called in index order.
#pragma once
#include <stdint.h>

#include "pv_trie_store.h"

namespace pv {

enum : uint8_t { TU_VALUE = 0, TU_SUBTREE = 1 };

struct TuCtx {
  // the store that holds the old trie
  const uint8_t* blob;
  const uint64_t *beg, *end;
  const uint32_t *dig, *table;
  uint32_t slots, n_nodes;
  const uint32_t* root;   // 8 words, not the blank root
  // the batch: sorted distinct keys, values (checked by tb_lcp_one before) non-empty, or empty for a removal
  // where the walk takes removals
  const uint8_t* key_blob;
  const uint64_t* key_off;
  const uint8_t* val_blob;
  const uint64_t* val_off;
  uint64_t n;
  const uint32_t* h;      // n + 1
  // per key, n + 1 entries: sizes from the count mode, scanned to range starts
  uint64_t *cnt, *pbytes, *vbytes;
  uint8_t* status;        // n
  // the merged items (write mode)
  uint8_t* ikey;
  uint64_t* ikoff;
  uint8_t* ival;
  uint64_t* ivoff;
  uint32_t* inib;
  uint8_t* ikind;
};

struct TuCur {
  uint64_t i, k, v;   // item index, path byte offset, payload byte offset (count mode: sizes)
};

// A child reference item: SP_OK and ref_len = 0 (blank) or the bytes to carry
// from its start; hashed = a 32-byte hash.  Stricter than the reading walks: an
// inline node is under 32 bytes and a hash has the one-byte header 0xa0, since
// the bytes are carried into the new trie as they are.
PV_HD uint32_t tu_ref(const TnItem& it, uint64_t& ref_len, bool& hashed) {
  ref_len = 0;
  hashed = false;
  if (it.l) {
    if (it.e - it.s >= 32) return SP_MALFORMED;
    ref_len = it.e - it.s;
    return SP_OK;
  }
  if (it.e == it.b) return SP_OK;
  if (it.e - it.b != 32 || it.b != it.s + 1) return SP_NODE_MISSING;
  ref_len = 33;
  hashed = true;
  return SP_OK;
}

// Q = X[:D] + path (pn nibbles of the hex-prefix bytes p from nibble `skip`)
// against X (xn >= D nibbles).  0: equal; 1: Q a proper prefix of X; 2: X a
// proper prefix of Q; 3: Q < X at a nibble; 4: X < Q at a nibble.  X absorbs a
// leaf's Q on 0 and an extension's Q on 0 or 1; X < Q without absorbing is 2 or 4.
PV_HD uint32_t tu_cmp(const uint8_t* p, uint64_t skip, uint64_t pn, const uint8_t* x, uint64_t D, uint64_t xn) {
  const uint64_t rest = xn - D, m = pn < rest ? pn : rest;
  uint64_t i = 0;
  uint32_t a = 0, b = 0;
  for (; i < m; ++i) {
    a = sp_nibble(p, skip + i);
    b = sp_nibble(x, D + i);
    if (a != b) break;
  }
  if (i == pn) return i == rest ? 0u : 1u;
  if (i == rest) return 2u;
  return a < b ? 3u : 4u;
}

// One item at `at`: the path is key[:D], then the nibble `slot` if it is < 16,
// then pn path nibbles of p (hex-prefix bytes, from nibble `skip`); the payload
// is src[0 .. len).  Count mode (!write) only advances `at`.
PV_HD void tu_put(const TuCtx& c, bool write, TuCur& at, const uint8_t* key, uint64_t D, const uint8_t* p,
                  uint64_t skip, uint64_t pn, uint32_t slot, uint8_t kind, const uint8_t* src, uint64_t len) {
  const uint64_t P = D + (slot < 16 ? 1 : 0), nib = P + pn, nb = (nib + 1) / 2;
  if (write) {
    uint8_t* w = c.ikey + at.k;
    for (uint64_t b = 0; b < nb; ++b) {
      uint32_t v = 0;
      for (uint32_t half = 0; half < 2; ++half) {
        const uint64_t x = 2 * b + half;
        uint32_t q = 0;   // the pad nibble of an odd path
        if (x < D) q = sp_nibble(key, x);
        else if (x < P) q = slot;
        else if (x < nib) q = sp_nibble(p, skip + (x - P));
        v = 16 * v + q;
      }
      w[b] = (uint8_t)v;
    }
    uint8_t* o = c.ival + at.v;
    for (uint64_t t = 0; t < len; ++t) o[t] = src[t];
    c.ikoff[at.i] = at.k;
    c.ivoff[at.i] = at.v;
    c.inib[at.i] = (uint32_t)nib;
    c.ikind[at.i] = kind;
  }
  at.i += 1;
  at.k += nb;
  at.v += len;
}

// The item a child reference stands for once its node is opened.
struct TuOpen {
  uint8_t kind;
  const uint8_t* p;   // the opened node's hex-prefix path: pn nibbles from nibble `skip` (a branch: none)
  uint64_t skip, pn;
  const uint8_t* src;
  uint64_t len;
};

// Open the reference blob[pos .. pos + rlen) (from tu_ref: rlen != 0).  A branch:
// the reference as it is.  A leaf: its path and value.  An extension: its path
// and its child reference.  SP_NODE_MISSING: the node is not in the store;
// SP_MALFORMED: it is no trie node.
PV_HD uint32_t tu_open(const TuCtx& c, uint64_t pos, uint64_t rlen, bool hashed, TuOpen& o) {
  const uint8_t* blob = c.blob;
  o = TuOpen{TU_SUBTREE, blob, 0, 0, blob + pos, rlen};
  uint64_t cb = pos, ce = pos + rlen;
  if (hashed) {
    uint32_t t[8];
    tn_load_ref(blob + pos + 1, t);
    const uint32_t id = ts_find(c.table, c.slots, c.dig, c.n_nodes, t);
    if (id == TS_ABSENT) return SP_NODE_MISSING;
    cb = c.beg[id];
    ce = c.end[id];
  }
  TnScan n;
  if (!tn_scan(blob, cb, ce, TN_NO_SLOT, n)) return SP_MALFORMED;
  if (n.count == 17) return SP_OK;
  TnPath h;
  if (n.count != 2 || !tn_path(blob, n.i0, h)) return SP_MALFORMED;
  if (h.leaf) {
    if (n.i1.l || n.i1.e == n.i1.b) return SP_MALFORMED;
    o = TuOpen{TU_VALUE, h.p, h.skip, h.pn, blob + n.i1.b, n.i1.e - n.i1.b};
    return SP_OK;
  }
  if (h.pn == 0) return SP_MALFORMED;
  uint64_t len;
  bool h2;
  const uint32_t r = tu_ref(n.i1, len, h2);
  if (r != SP_OK) return r;
  if (len == 0) return SP_MALFORMED;
  o = TuOpen{TU_SUBTREE, h.p, h.skip, h.pn, blob + n.i1.s, len};
  return SP_OK;
}

// The child reference blob[pos .. pos + rlen) of slot t of the branch at depth D,
// carried as an item: as it is, or, by the lane of a removed key, opened.
PV_HD uint32_t tu_carry(const TuCtx& c, bool open, bool write, TuCur& at, const uint8_t* key, uint64_t D, uint32_t t,
                        uint64_t pos, uint64_t rlen, bool hashed) {
  if (!open) {
    tu_put(c, write, at, key, D, key, 0, 0, t, TU_SUBTREE, c.blob + pos, rlen);
    return SP_OK;
  }
  TuOpen o;
  const uint32_t r = tu_open(c, pos, rlen, hashed, o);
  if (r != SP_OK) return r;
  tu_put(c, write, at, key, D, o.p, o.skip, o.pn, t, o.kind, o.src, o.len);
  return SP_OK;
}

// The walk of batch key j.  Count mode: cnt / pbytes / vbytes [j] and status[j].
// Write mode (after the scans, every status SP_OK): the items of key j.
// REMOVALS: an empty value removes key j (see the head of this file); without
// it no value is empty and the walk is the one of a batch of sets.
template <bool REMOVALS>
PV_HD uint32_t tu_walk_t(const TuCtx& c, uint64_t j, bool write) {
  const bool rem = REMOVALS && c.val_off[j + 1] == c.val_off[j];
  const uint8_t* key = c.key_blob + c.key_off[j];
  const uint64_t knib = 2 * (c.key_off[j + 1] - c.key_off[j]);
  const uint32_t hl = c.h[j], hr = c.h[j + 1];
  const uint8_t* kp = key;
  uint64_t pnib = 0;
  if (j > 0) {
    kp = c.key_blob + c.key_off[j - 1];
    pnib = 2 * (c.key_off[j] - c.key_off[j - 1]);
  }
  TuCur front{0, 0, 0}, back{0, 0, 0};
  if (write) {
    front = TuCur{c.cnt[j], c.pbytes[j], c.vbytes[j]};
    back = TuCur{c.cnt[j + 1], c.pbytes[j + 1], c.vbytes[j + 1]};
  }
  const uint8_t* blob = c.blob;
  uint32_t id = ts_find(c.table, c.slots, c.dig, c.n_nodes, c.root);
  if (id == TS_ABSENT) return SP_NODE_MISSING;
  uint64_t cb = c.beg[id], ce = c.end[id], D = 0;
  uint32_t st = SP_MALFORMED;   // the step bound ran out
  for (uint64_t step = 0; step <= knib; ++step) {
    const bool first = hl <= D, last = hr <= D;
    const int32_t s = D < knib ? (int32_t)sp_nibble(key, D) : -1;
    const int32_t s_prev = (!first && D < pnib) ? (int32_t)sp_nibble(kp, D) : -1;
    // first scan: the shape, item 0 and 1, slot s, item 16
    TnScan n;
    if (!tn_scan(blob, cb, ce, (uint32_t)s, n) || (n.count != 17 && n.count != 2)) break;
    uint32_t bad = SP_OK;
    TuCur grp{0, 0, 0};   // the AFTER group's size
    TnItem r;             // the child the walk goes on in
    if (n.count == 17) {
      if (n.i16.l) break;
      // second scan: the carried slots, checked; in write mode also written
      if (n.i16.e > n.i16.b && first && knib != D)
        tu_put(c, write, front, key, D, key, 0, 0, 16, TU_VALUE, blob + n.i16.b, n.i16.e - n.i16.b);
      for (uint32_t pass = 0; pass < 2 && bad == SP_OK; ++pass) {
        // pass 0 sizes the AFTER group (and counts BEFORE in count mode); pass 1 writes
        if (pass == 1 && !write) break;
        TuCur w = back;
        if (pass == 1) {
          back.i -= grp.i, back.k -= grp.k, back.v -= grp.v;
          w = back;
        }
        uint64_t pos = n.pb;
        for (int32_t t = 0; t < 16; ++t) {
          TnItem it;
          it.s = pos;
          uint64_t rlen;
          bool hashed;
          if (!rlp_item(blob, pos, n.pe, it.l, it.b, it.e)) {   // parsed by the first scan: never
            bad = SP_MALFORMED;
            break;
          }
          const bool before = t > s_prev && t < s, after = last && t > s;
          if (before || after) {
            const uint32_t rr = tu_ref(it, rlen, hashed);
            if (rr != SP_OK) {
              bad = rr;
              break;
            }
            if (rlen) {
              uint32_t ro = SP_OK;
              if (pass == 0) {
                if (after) ro = tu_carry(c, rem, false, grp, key, D, (uint32_t)t, pos, rlen, hashed);
                else if (!write) ro = tu_carry(c, rem, false, front, key, D, (uint32_t)t, pos, rlen, hashed);
              } else {
                ro = tu_carry(c, rem, true, before ? front : w, key, D, (uint32_t)t, pos, rlen, hashed);
              }
              if (ro != SP_OK) {
                bad = ro;
                break;
              }
            }
          }
          pos = it.e;
        }
      }
      if (bad != SP_OK) {
        st = bad;
        break;
      }
      if (!write) front.i += grp.i, front.k += grp.k, front.v += grp.v;
      if (s < 0) {
        st = SP_OK;
        break;
      }
      r = n.sel;
      D += 1;
    } else {
      TnPath h;
      if (!tn_path(blob, n.i0, h)) break;
      const bool leaf = h.leaf;
      if (!leaf && h.pn == 0) break;
      if (leaf && (n.i1.l || n.i1.e == n.i1.b)) break;
      const uint32_t cq = tu_cmp(h.p, h.skip, h.pn, key, D, knib);
      if (leaf && cq == 0) {   // overwritten
        st = SP_OK;
        break;
      }
      if (!leaf && cq <= 1) {   // dissolved
        r = n.i1;
        D += h.pn;
      } else {
        const uint8_t* src = blob + n.i1.b;
        uint64_t len = n.i1.e - n.i1.b;
        if (!leaf) {
          bool hashed;
          const uint32_t rr = tu_ref(n.i1, len, hashed);
          if (rr != SP_OK || len == 0) {
            st = rr != SP_OK ? rr : (uint32_t)SP_MALFORMED;
            break;
          }
          src = blob + n.i1.s;
        }
        const uint8_t kind = leaf ? TU_VALUE : TU_SUBTREE;
        if (cq == 1 || cq == 3) {
          bool mine = first;
          if (!mine) {
            const uint32_t cp = tu_cmp(h.p, h.skip, h.pn, kp, D, pnib);
            mine = cp == 2 || cp == 4;
          }
          if (mine) tu_put(c, write, front, key, D, h.p, h.skip, h.pn, 16, kind, src, len);
        } else if (last) {
          if (write) {
            TuCur one{0, 0, 0};
            tu_put(c, false, one, key, D, h.p, h.skip, h.pn, 16, kind, src, len);
            back.i -= one.i, back.k -= one.k, back.v -= one.v;
            TuCur w = back;
            tu_put(c, true, w, key, D, h.p, h.skip, h.pn, 16, kind, src, len);
          } else {
            tu_put(c, false, front, key, D, h.p, h.skip, h.pn, 16, kind, src, len);
          }
        }
        st = SP_OK;
        break;
      }
    }
    uint64_t rlen;
    bool hashed;
    const uint32_t rr = tu_ref(r, rlen, hashed);
    if (rr != SP_OK) {
      st = rr;
      break;
    }
    if (rlen == 0) {   // a blank slot ends the walk; an extension over nothing is no node
      st = n.count == 17 ? (uint32_t)SP_OK : (uint32_t)SP_MALFORMED;
      break;
    }
    if (!hashed) {
      cb = r.s;
      ce = r.e;
      continue;
    }
    uint32_t t[8];
    tn_load_ref(blob + r.b, t);
    id = ts_find(c.table, c.slots, c.dig, c.n_nodes, t);
    if (id == TS_ABSENT) {
      st = SP_NODE_MISSING;
      break;
    }
    cb = c.beg[id];
    ce = c.end[id];
  }
  if (st != SP_OK) return st;
  if (!rem)
    tu_put(c, write, front, key, knib, key, 0, 0, 16, TU_VALUE, c.val_blob + c.val_off[j], c.val_off[j + 1] - c.val_off[j]);
  if (!write) {
    c.cnt[j] = front.i;
    c.pbytes[j] = front.k;
    c.vbytes[j] = front.v;
  }
  return SP_OK;
}

// a batch of sets (pv_state_update): no value is empty
PV_HD uint32_t tu_walk(const TuCtx& c, uint64_t j, bool write) { return tu_walk_t<false>(c, j, write); }

}  // namespace pv
