// Host model of the resident key arena's pubkey index: csrc/gv_kidx.h -- the
// hash, the probe sequence, insert and lookup the kernels of gv_kidx.hip run
// -- compiled by g++ and driven one key at a time, in slot order (the device
// enters a launch's slots concurrently; which slot a table word ends up
// naming does not depend on the order, only which keys of an over-full probe
// window are left out may).  tests/test_keys_index_host.py loads it with
// ctypes; tests/kidx/kidx_harness.cpp includes it under ASan + UBSan.
//   g++ -O2 -std=c++17 -shared -fPIC -o kidx_host.so tools/fe29/kidx_host.cpp
#include <stdint.h>
#include <string.h>

#include "../../cosmos-sdk-rootchain_amd/csrc/gv_kidx.h"

extern "C" {

uint32_t kidx_probe_bound(void) { return GV_KIDX_PROBE; }
uint32_t kidx_row_words(void) { return GV_KIDX_ROW; }

// k_kidx_rows: key g's row into slot base + g, or slots[g].
void kidx_rows(const uint8_t* pub33, uint32_t n, uint32_t base, const uint32_t* slots, uint32_t* rows) {
  for (uint32_t g = 0; g < n; ++g)
    gv_kidx_row(pub33 + (size_t)g * 33, rows + (size_t)(slots ? slots[g] : base + g) * GV_KIDX_ROW);
}

// The table word a key's probe starts at.
uint32_t kidx_home(const uint8_t* pub33, uint64_t seed, uint32_t tslots) {
  uint32_t row[GV_KIDX_ROW];
  gv_kidx_row(pub33, row);
  return gv_kidx_word(gv_kidx_hash(row, seed), 0, tslots - 1);
}

void kidx_clear(uint32_t* table, uint32_t tslots) { memset(table, 0xFF, (size_t)tslots * 4); }

// k_kidx_put over slots base.. (or slots[g]); returns the keys left out.
uint32_t kidx_put(uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t n, uint32_t base,
                  const uint32_t* slots, uint64_t seed) {
  uint32_t left = 0;
  for (uint32_t g = 0; g < n; ++g) left += !gv_kidx_put(table, tslots - 1, rows, slots ? slots[g] : base + g, seed);
  return left;
}

// k_kidx_find; returns the misses.
uint32_t kidx_find(const uint32_t* table, uint32_t tslots, const uint32_t* rows, uint32_t count, uint64_t seed,
                   const uint8_t* pub33, uint32_t n, uint32_t* slot_out) {
  uint32_t miss = 0;
  for (uint32_t g = 0; g < n; ++g) {
    uint32_t row[GV_KIDX_ROW];
    gv_kidx_row(pub33 + (size_t)g * 33, row);
    slot_out[g] = gv_kidx_find(table, tslots - 1, rows, count, row, seed);
    miss += slot_out[g] == GV_KIDX_EMPTY;
  }
  return miss;
}

// `want` distinct pseudo-random keys (prefix 02 / 03, 32 bytes from a
// splitmix64 stream started at rng) whose home word under (seed, tslots) is
// `home`, into out_pub33; returns how many were found within max_tries.
uint32_t kidx_search_home(uint64_t seed, uint32_t tslots, uint32_t home, uint32_t want, uint64_t rng,
                          uint64_t max_tries, uint8_t* out_pub33) {
  uint32_t found = 0;
  for (uint64_t t = 0; t < max_tries && found < want; ++t) {
    uint8_t key[33];
    for (int w = 0; w < 5; ++w) {
      uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
      z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
      z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
      z ^= z >> 31;
      if (w == 4) key[0] = (uint8_t)(2 + (z & 1));
      else memcpy(key + 1 + 8 * w, &z, 8);
    }
    if (kidx_home(key, seed, tslots) == home) memcpy(out_pub33 + (size_t)found++ * 33, key, 33);
  }
  return found;
}
}
