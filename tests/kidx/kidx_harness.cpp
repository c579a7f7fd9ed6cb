// The pubkey index's host model (tools/fe29/kidx_host.cpp over csrc/gv_kidx.h)
// as a program of its own, for ASan + UBSan: the scenarios of
// tests/test_keys_index_host.py against a std::map.  Exit 0 and "kidx ok" when
// every check holds.  Test infrastructure only.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tests/kidx/kidx_harness.cpp -o kidx_harness && ./kidx_harness
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../../tools/fe29/kidx_host.cpp"

namespace {
typedef std::array<uint8_t, 33> Key;
const uint64_t kSeed = 0x0123456789ABCDEFull;
const uint32_t kNone = 0xFFFFFFFFu;
int failures = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
  } while (0)

struct Model {
  uint32_t T;
  std::vector<Key> keys;                               // by slot
  std::vector<uint32_t> rows, table;
  uint32_t left = 0;
  explicit Model(uint32_t t) : T(t), table(t, kNone) {}
  void load(const std::vector<Key>& ks) {
    const uint32_t base = (uint32_t)keys.size();
    keys.insert(keys.end(), ks.begin(), ks.end());
    rows.resize(keys.size() * GV_KIDX_ROW);
    kidx_rows(ks[0].data(), (uint32_t)ks.size(), base, nullptr, rows.data());
    left += kidx_put(table.data(), T, rows.data(), (uint32_t)ks.size(), base, nullptr, kSeed);
  }
  void replace(uint32_t slot, const Key& k) {          // the row, then the table refilled from every row
    keys[slot] = k;
    kidx_rows(k.data(), 1, 0, &slot, rows.data());
    kidx_clear(table.data(), T);
    left = kidx_put(table.data(), T, rows.data(), (uint32_t)keys.size(), 0, nullptr, kSeed);
  }
  uint32_t find(const Key& k) const {
    uint32_t out = 12345;
    kidx_find(table.data(), T, rows.data(), (uint32_t)keys.size(), kSeed, k.data(), 1, &out);
    return out;
  }
  // every resident key finds its lowest slot (or, when keys were left out,
  // nothing); nothing ever finds a slot with other bytes; returns the misses
  uint32_t check() const {
    std::map<Key, uint32_t> lowest;
    for (uint32_t s = (uint32_t)keys.size(); s-- > 0;) lowest[keys[s]] = s;
    uint32_t miss = 0;
    for (const auto& kv : lowest) {
      const uint32_t got = find(kv.first);
      if (got == kNone) ++miss;
      else CHECK(got == kv.second && keys[got] == kv.first);
    }
    if (left == 0) CHECK(miss == 0);
    return miss;
  }
};

std::mt19937_64 rng(20240611);
Key random_key() {
  Key k;
  for (auto& b : k) b = (uint8_t)rng();
  k[0] = (uint8_t)(2 + (k[0] & 1));
  return k;
}
std::vector<Key> homed(uint32_t T, uint32_t home, uint32_t want, uint64_t stream) {
  std::vector<uint8_t> buf((size_t)want * 33);
  const uint32_t got = kidx_search_home(kSeed, T, home, want, stream, 1ull << 26, buf.data());
  CHECK(got == want);
  std::vector<Key> ks(got);
  for (uint32_t i = 0; i < got; ++i) memcpy(ks[i].data(), &buf[(size_t)i * 33], 33);
  return ks;
}
}  // namespace

int main() {
  {                                                    // random keys, unknown keys
    Model m(8192);
    std::vector<Key> ks(2000);
    for (auto& k : ks) k = random_key();
    m.load(ks);
    CHECK(m.left == 0 && m.check() == 0);
    for (int i = 0; i < 500; ++i) CHECK(m.find(random_key()) == kNone);
    for (uint32_t s = 0; s < 2000; ++s) CHECK(m.find(ks[s]) == s);
  }
  {                                                    // bytes 1..16 shared, the tail differs
    Model m(8192);
    const Key head = random_key();
    std::vector<Key> ks(300, head);
    for (auto& k : ks)
      for (int i = 17; i < 33; ++i) k[i] = (uint8_t)rng();
    m.load(ks);
    CHECK(m.left == 0 && m.check() == 0);
  }
  {                                                    // one-byte neighbours: prefix, last byte, first x byte
    Model m(512);
    Key a = random_key(), b = a, c = a, d = a;
    a[0] = 2; b[0] = 3; c[32] ^= 1; d[1] ^= 0x80;
    m.load({a, b, c, d});
    CHECK(m.find(a) == 0 && m.find(b) == 1 && m.find(c) == 2 && m.find(d) == 3);
    Key e = a;
    e[16] ^= 4;
    CHECK(m.find(e) == kNone);
  }
  {                                                    // the same bytes in three slots
    Model m(512);
    const Key k = random_key(), x = random_key(), y = random_key();
    m.load({x, k, y, k, k});
    CHECK(m.find(k) == 1);
    m.replace(1, random_key());
    CHECK(m.find(k) == 3 && m.check() == 0);
    m.replace(3, random_key());
    CHECK(m.find(k) == 4);
    m.replace(4, random_key());
    CHECK(m.find(k) == kNone && m.check() == 0);
  }
  {                                                    // home word T - 1: the probe wraps to word 0
    Model m(512);
    const std::vector<Key> ks = homed(512, 511, 3, 7);
    m.load(ks);
    CHECK(m.table[511] == 0 && m.table[0] == 1 && m.table[1] == 2);
    CHECK(m.left == 0 && m.check() == 0);
  }
  {                                                    // the bound: PROBE + 6 keys of one home word
    Model m(512);
    const std::vector<Key> ks = homed(512, 100, GV_KIDX_PROBE + 6, 11);
    m.load(ks);
    CHECK(m.left == 6);
    CHECK(m.check() == 6);
    for (uint32_t s = 0; s < ks.size(); ++s) CHECK(m.find(ks[s]) == (s < GV_KIDX_PROBE ? s : kNone));
  }
  if (failures) return 1;
  printf("kidx ok\n");
  return 0;
}
