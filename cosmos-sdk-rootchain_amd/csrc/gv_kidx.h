// gv_kidx.h -- the pubkey index of the two resident key arenas (options
// "keys_index" and "ed_keys_index"): the key-bytes -> row loader, the hash, the
// probe sequence, insert and lookup over one table word per probe, each a
// template over the row length R.  Shared by the kernels (gv_kidx.hip) and,
// compiled by g++, by the host model the CPU tests run
// (tools/fe29/kidx_host.cpp) -- one routine on both sides, as ed_comb_digit in
// ed_scalar.cuh.
//
// A row holds a key's bytes as sent: a lookup matches bytes, not points.
//   secp256k1, R = GV_KIDX_ROW = 9: the SEC1 prefix byte, then the 8 x words
//     k_unpack writes to in_pfx / in_x (word i = big-endian bytes 29 - 4 i ..
//     32 - 4 i of the 33, least significant word first) -- a key ParsePubKey
//     rejects included.  The index keeps these rows itself (k_kidx_rows).
//   ed25519, R = GV_KIDX_ROW_ED = 8: word i = the little-endian bytes 4 i ..
//     4 i + 3 of the 32 -- a non-canonical encoding and its canonical twin are
//     different keys, as they are to the hash of a verify.  These are the
//     arena's own ekpub rows (k_ed_keys / k_ed_keys_chain write them).
//
// The table is T u32 words (T a power of two), GV_KIDX_EMPTY or a slot
// number; open addressing, linear probing from the key's home word, at most
// GV_KIDX_PROBE words per insert or lookup.  Contract: a
// lookup returns a slot only after all R words of its row compared equal, and
// the lowest such slot; a miss is always safe (the batch takes the route it
// takes without an index), so an insert that finds no word within the bound
// leaves the key out, and nothing is ever deleted -- a replacement refills the
// table from the rows.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GV_KIDX_FN __host__ __device__ inline
#else
#define GV_KIDX_FN inline
#endif

#define GV_KIDX_PROBE 64
#define GV_KIDX_EMPTY 0xFFFFFFFFu
#define GV_KIDX_ROW 9
#define GV_KIDX_ROW_ED 8

// Bytes of the key a row of R words holds.
template <int R>
struct gv_kidx_key {
  static_assert(R == GV_KIDX_ROW || R == GV_KIDX_ROW_ED, "a pub33 or a pub32 row");
  static constexpr int bytes = R == GV_KIDX_ROW ? 33 : 32;
};

// Row of the key bytes at p (any alignment): what k_kidx_rows and k_ed_keys
// write for a slot, and what a lookup forms from an item's bytes.  One case is
// not here: k_kidx_find reads a pub32 batch on a 4-byte aligned base as whole
// words, a kernel-uniform branch written in the kernel (inside this inlined
// loader it changed the kernel's code), so the host model compiles only the
// byte-wise load; the GPU tests run aligned and misaligned bases against it.
template <int R>
GV_KIDX_FN void gv_kidx_row_n(const uint8_t* p, uint32_t* row) {
  if constexpr (R == GV_KIDX_ROW) {
    row[0] = p[0];
    for (int i = 0; i < 8; ++i) {
      const uint8_t* q = p + 1 + 4 * (7 - i);
      row[1 + i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
    }
  } else {
    for (int i = 0; i < R; ++i) {
      const uint8_t* q = p + 4 * i;
      row[i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    }
  }
}

template <int R>
GV_KIDX_FN bool gv_kidx_equal_n(const uint32_t* a, const uint32_t* b) {
  bool eq = true;
  for (int i = 0; i < R; ++i) eq &= a[i] == b[i];
  return eq;
}

// key_hash (gv_kernels.hip) over all R words, started from the context's
// 64-bit seed and closed with it: accounts are chosen by whoever sends
// transactions and the index outlives a batch, so the home word of a key must
// not be computable without the seed.  (The probe bound, not the hash, is what
// keeps run time and verdicts independent of the keys.)
template <int R>
GV_KIDX_FN uint32_t gv_kidx_hash_n(const uint32_t* row, uint64_t seed) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ seed;
  for (int i = 0; i < R; ++i) {
    h ^= row[i];
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 29;
  }
  h ^= (seed << 32) | (seed >> 32);
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return (uint32_t)(h ^ (h >> 32));
}

// Probe step i (0 .. GV_KIDX_PROBE - 1) of a key whose hash is h: the table
// word it looks at.  Linear, wrapping at T = tmask + 1.
GV_KIDX_FN uint32_t gv_kidx_word(uint32_t h, uint32_t i, uint32_t tmask) { return (h + i) & tmask; }

// Compare-and-swap and minimum on one table word: atomics in a kernel (the
// table word is the only datum the lanes of a launch share), plain code in
// the sequential host model.
GV_KIDX_FN uint32_t gv_kidx_cas(uint32_t* w, uint32_t expect, uint32_t val) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(w, expect, val);
#else
  const uint32_t cur = *w;
  if (cur == expect) *w = val;
  return cur;
#endif
}
GV_KIDX_FN void gv_kidx_min(uint32_t* w, uint32_t val) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(w, val);
#else
  if (val < *w) *w = val;
#endif
}

// Enter slot `slot` (its row already in rows, R words per slot).
// An empty word is taken; a word whose slot holds the same bytes keeps the
// lower of the two slots (the same key in two slots is legal: the index names
// the lowest); another key's word sends the probe on.  Returns false when the
// bound ran out: the key stays out of the index.
template <int R>
GV_KIDX_FN bool gv_kidx_put_n(uint32_t* table, uint32_t tmask, const uint32_t* rows, uint32_t slot, uint64_t seed) {
  const uint32_t* row = rows + (size_t)slot * R;
  const uint32_t h = gv_kidx_hash_n<R>(row, seed);
  for (uint32_t i = 0; i < GV_KIDX_PROBE; ++i) {
    uint32_t* w = table + gv_kidx_word(h, i, tmask);
    const uint32_t cur = gv_kidx_cas(w, GV_KIDX_EMPTY, slot);
    if (cur == GV_KIDX_EMPTY || cur == slot) return true;
    if (gv_kidx_equal_n<R>(rows + (size_t)cur * R, row)) {
      gv_kidx_min(w, slot);
      return true;
    }
  }
  return false;
}

// The slot whose row equals `row` (the lowest, by gv_kidx_put), or
// GV_KIDX_EMPTY: an empty word ends the probe, and so does the bound.  A
// table word at or past `count` (never written by gv_kidx_put over
// [0, count)) is passed over like another key's.
template <int R>
GV_KIDX_FN uint32_t gv_kidx_find_n(const uint32_t* table, uint32_t tmask, const uint32_t* rows, uint32_t count,
                                   const uint32_t* row, uint64_t seed) {
  const uint32_t h = gv_kidx_hash_n<R>(row, seed);
  for (uint32_t i = 0; i < GV_KIDX_PROBE; ++i) {
    const uint32_t cur = table[gv_kidx_word(h, i, tmask)];
    if (cur == GV_KIDX_EMPTY) return GV_KIDX_EMPTY;
    if (cur < count && gv_kidx_equal_n<R>(rows + (size_t)cur * R, row)) return cur;
  }
  return GV_KIDX_EMPTY;
}
