// Host model of the key arenas' pubkey index: csrc/gv_kidx.h -- the row
// loader, the hash, the probe sequence, insert and lookup the kernels of
// gv_kidx.hip run -- compiled by g++ and driven one key at a time, in slot
// order (the device enters a launch's slots concurrently; which slot a table
// word ends up naming does not depend on the order, only which keys of an
// over-full probe window are left out may).  One template per routine over the
// row length, exported twice: kidx_* for the secp256k1 arena's 33-byte keys
// (9-word rows), edkidx_* for the ed25519 arena's 32-byte keys (8-word rows).
// tests/kidx_model.py loads it with ctypes; tests/kidx/kidx_harness.cpp
// includes it under ASan + UBSan.
//   g++ -O2 -std=c++17 -shared -fPIC -o kidx_host.so tools/fe29/kidx_host.cpp
#include <stdint.h>
#include <string.h>

#include "../../cosmos-sdk-rootchain_amd/csrc/gv_kidx.h"

namespace kidx_host {
// Key g of the AoS at `keys` -> its row.
template <int R>
void row_of(const uint8_t* keys, size_t g, uint32_t* row) {
  gv_kidx_row_n<R>(keys + g * gv_kidx_key<R>::bytes, row);
}

// k_kidx_rows, and what k_ed_keys writes to ekpub: key g's row into slot
// base + g, or slots[g].
template <int R>
void rows(const uint8_t* keys, uint32_t n, uint32_t base, const uint32_t* slots, uint32_t* out) {
  for (uint32_t g = 0; g < n; ++g) row_of<R>(keys, g, out + (size_t)(slots ? slots[g] : base + g) * R);
}

// The table word a key's probe starts at.
template <int R>
uint32_t home(const uint8_t* key, uint64_t seed, uint32_t tslots) {
  uint32_t row[R];
  row_of<R>(key, 0, row);
  return gv_kidx_word(gv_kidx_hash_n<R>(row, seed), 0, tslots - 1);
}

// k_kidx_put over slots base.. (or slots[g]); returns the keys left out.
template <int R>
uint32_t put(uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t n, uint32_t base, const uint32_t* slots,
             uint64_t seed) {
  uint32_t left = 0;
  for (uint32_t g = 0; g < n; ++g) left += !gv_kidx_put_n<R>(table, tslots - 1, rows, slots ? slots[g] : base + g, seed);
  return left;
}

// k_kidx_find; returns the misses.
template <int R>
uint32_t find(const uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t count, uint64_t seed,
              const uint8_t* keys, uint32_t n, uint32_t* slot_out) {
  uint32_t miss = 0;
  for (uint32_t g = 0; g < n; ++g) {
    uint32_t row[R];
    row_of<R>(keys, g, row);
    slot_out[g] = gv_kidx_find_n<R>(table, tslots - 1, rows, count, row, seed);
    miss += slot_out[g] == GV_KIDX_EMPTY;
  }
  return miss;
}

// `want` distinct pseudo-random keys (32 bytes from a splitmix64 stream
// started at rng, then for a pub33 the prefix 02 / 03; bytes, not points: the
// index never decodes a key) whose home word under (seed, tslots) is `home`,
// into out; returns how many were found within max_tries.
template <int R>
uint32_t search_home(uint64_t seed, uint32_t tslots, uint32_t home_word, uint32_t want, uint64_t rng,
                     uint64_t max_tries, uint8_t* out) {
  const int KB = gv_kidx_key<R>::bytes;
  uint32_t found = 0;
  for (uint64_t t = 0; t < max_tries && found < want; ++t) {
    uint8_t key[KB];
    for (int w = 0; w < 4 + (KB - 32); ++w) {
      uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      if (w == 4) key[0] = (uint8_t)(2 + (z & 1));
      else memcpy(key + (KB - 32) + 8 * w, &z, 8);
    }
    if (home<R>(key, seed, tslots) == home_word) memcpy(out + (size_t)found++ * KB, key, KB);
  }
  return found;
}
}  // namespace kidx_host

extern "C" {
void kidx_clear(uint32_t* table, uint32_t tslots) { memset(table, 0xFF, (size_t)tslots * 4); }
void edkidx_clear(uint32_t* table, uint32_t tslots) { kidx_clear(table, tslots); }

#define KIDX_EXPORTS(P, R)                                                                                             \
  uint32_t P##_probe_bound(void) { return GV_KIDX_PROBE; }                                                             \
  uint32_t P##_row_words(void) { return R; }                                                                           \
  void P##_rows(const uint8_t* keys, uint32_t n, uint32_t base, const uint32_t* slots, uint32_t* rows) {               \
    kidx_host::rows<R>(keys, n, base, slots, rows);                                                                    \
  }                                                                                                                    \
  uint32_t P##_home(const uint8_t* key, uint64_t seed, uint32_t tslots) { return kidx_host::home<R>(key, seed, tslots); } \
  uint32_t P##_put(uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t n, uint32_t base,                  \
                   const uint32_t* slots, uint64_t seed) {                                                             \
    return kidx_host::put<R>(table, tslots, rows, n, base, slots, seed);                                               \
  }                                                                                                                    \
  uint32_t P##_find(const uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t count, uint64_t seed,       \
                    const uint8_t* keys, uint32_t n, uint32_t* slot_out) {                                             \
    return kidx_host::find<R>(table, tslots, rows, count, seed, keys, n, slot_out);                                    \
  }                                                                                                                    \
  uint32_t P##_search_home(uint64_t seed, uint32_t tslots, uint32_t home, uint32_t want, uint64_t rng,                 \
                           uint64_t max_tries, uint8_t* out) {                                                         \
    return kidx_host::search_home<R>(seed, tslots, home, want, rng, max_tries, out);                                   \
  }
KIDX_EXPORTS(kidx, GV_KIDX_ROW)
KIDX_EXPORTS(edkidx, GV_KIDX_ROW_ED)
#undef KIDX_EXPORTS
}
