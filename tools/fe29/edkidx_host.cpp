// Host model of the ed25519 key arena's pubkey index (option "ed_keys_index"):
// csrc/gv_kidx.h at the ed25519 row length -- the hash, the probe sequence,
// insert and lookup k_edkidx_put / k_edkidx_find run -- compiled by g++ and
// driven one key at a time, in slot order (as tools/fe29/kidx_host.cpp: which
// slot a table word ends up naming does not depend on the order, only which
// keys of an over-full probe window are left out may).
// tests/edkidx_model.py loads it with ctypes; tests/edkidx/edkidx_harness.cpp
// includes it under ASan + UBSan.
//   g++ -O2 -std=c++17 -shared -fPIC -o edkidx_host.so tools/fe29/edkidx_host.cpp
#include <stdint.h>
#include <string.h>

#include "../../cosmos-sdk-rootchain_amd/csrc/gv_kidx.h"

extern "C" {

uint32_t edkidx_probe_bound(void) { return GV_KIDX_PROBE; }
uint32_t edkidx_row_words(void) { return GV_EDKIDX_ROW; }

// What k_ed_keys writes to ekpub: key g's row into slot base + g, or slots[g].
void edkidx_rows(const uint8_t* pub32, uint32_t n, uint32_t base, const uint32_t* slots, uint32_t* rows) {
  for (uint32_t g = 0; g < n; ++g)
    gv_edkidx_row(pub32 + (size_t)g * 32, rows + (size_t)(slots ? slots[g] : base + g) * GV_EDKIDX_ROW);
}

// The table word a key's probe starts at.
uint32_t edkidx_home(const uint8_t* pub32, uint64_t seed, uint32_t tslots) {
  uint32_t row[GV_EDKIDX_ROW];
  gv_edkidx_row(pub32, row);
  return gv_kidx_word(gv_kidx_hash_n<GV_EDKIDX_ROW>(row, seed), 0, tslots - 1);
}

void edkidx_clear(uint32_t* table, uint32_t tslots) { memset(table, 0xFF, (size_t)tslots * 4); }

// k_edkidx_put over slots base.. (or slots[g]); returns the keys left out.
uint32_t edkidx_put(uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t n, uint32_t base,
                    const uint32_t* slots, uint64_t seed) {
  uint32_t left = 0;
  for (uint32_t g = 0; g < n; ++g)
    left += !gv_kidx_put_n<GV_EDKIDX_ROW>(table, tslots - 1, rows, slots ? slots[g] : base + g, seed);
  return left;
}

// k_edkidx_find; returns the misses.
uint32_t edkidx_find(const uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t count, uint64_t seed,
                     const uint8_t* pub32, uint32_t n, uint32_t* slot_out) {
  uint32_t miss = 0;
  for (uint32_t g = 0; g < n; ++g) {
    uint32_t row[GV_EDKIDX_ROW];
    gv_edkidx_row(pub32 + (size_t)g * 32, row);
    slot_out[g] = gv_kidx_find_n<GV_EDKIDX_ROW>(table, tslots - 1, rows, count, row, seed);
    miss += slot_out[g] == GV_KIDX_EMPTY;
  }
  return miss;
}

// `want` distinct pseudo-random 32-byte strings (a splitmix64 stream started
// at rng; bytes, not points: the index never decodes a key) whose home word
// under (seed, tslots) is `home`, into out_pub32; returns how many were found
// within max_tries.
uint32_t edkidx_search_home(uint64_t seed, uint32_t tslots, uint32_t home, uint32_t want, uint64_t rng,
                            uint64_t max_tries, uint8_t* out_pub32) {
  uint32_t found = 0;
  for (uint64_t t = 0; t < max_tries && found < want; ++t) {
    uint8_t key[32];
    for (int w = 0; w < 4; ++w) {
      uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      memcpy(key + 8 * w, &z, 8);
    }
    if (edkidx_home(key, seed, tslots) == home) memcpy(out_pub32 + (size_t)found++ * 32, key, 32);
  }
  return found;
}
}
