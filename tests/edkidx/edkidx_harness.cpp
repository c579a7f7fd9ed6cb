// The ed25519 pubkey index's host model (tools/fe29/edkidx_host.cpp over
// csrc/gv_kidx.h at 8-word rows) as a program of its own, for ASan + UBSan:
// the scenarios of tests/test_ed_keys_index_host.py against a std::map.  Exit
// 0 and "edkidx ok" when every check holds.  Test infrastructure only.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tests/edkidx/edkidx_harness.cpp -o edkidx_harness && ./edkidx_harness
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../../tools/fe29/edkidx_host.cpp"

namespace {
typedef std::array<uint8_t, 32> Key;
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
    rows.resize(keys.size() * GV_EDKIDX_ROW);
    edkidx_rows(ks[0].data(), (uint32_t)ks.size(), base, nullptr, rows.data());
    left += edkidx_put(table.data(), T, rows.data(), (uint32_t)ks.size(), base, nullptr, kSeed);
  }
  void replace(uint32_t slot, const Key& k) {          // the row, then the table refilled from every row
    keys[slot] = k;
    edkidx_rows(k.data(), 1, 0, &slot, rows.data());
    edkidx_clear(table.data(), T);
    left = edkidx_put(table.data(), T, rows.data(), (uint32_t)keys.size(), 0, nullptr, kSeed);
  }
  uint32_t find(const Key& k, uint32_t count) const {
    uint32_t out = 12345;
    edkidx_find(table.data(), T, rows.data(), count, kSeed, k.data(), 1, &out);
    return out;
  }
  uint32_t find(const Key& k) const { return find(k, (uint32_t)keys.size()); }
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

std::mt19937_64 rng(20240613);
Key random_key() {
  Key k;
  for (auto& b : k) b = (uint8_t)rng();
  return k;
}
std::vector<Key> random_keys(size_t n) {
  std::vector<Key> ks(n);
  for (auto& k : ks) k = random_key();
  return ks;
}
std::vector<Key> homed(uint32_t T, uint32_t home, uint32_t want, uint64_t stream) {
  std::vector<uint8_t> buf((size_t)want * 32);
  const uint32_t got = edkidx_search_home(kSeed, T, home, want, stream, 1ull << 26, buf.data());
  CHECK(got == want);
  std::vector<Key> ks(got);
  for (uint32_t i = 0; i < got; ++i) memcpy(ks[i].data(), &buf[(size_t)i * 32], 32);
  return ks;
}
}  // namespace

int main() {
  CHECK(edkidx_row_words() == 8 && edkidx_probe_bound() == 64);
  {                                                    // loads of 1 / 255 / 256 / 257 keys in turn
    Model m(2048);
    const std::vector<Key> pool = random_keys(769 + 200);
    uint32_t lo = 0;
    for (uint32_t n : {1u, 255u, 256u, 257u}) {
      m.load(std::vector<Key>(pool.begin() + lo, pool.begin() + lo + n));
      lo += n;
      CHECK(m.left == 0 && m.check() == 0);
      for (uint32_t s = 0; s < lo; ++s) CHECK(m.find(pool[s]) == s);
      for (uint32_t s = lo; s < pool.size(); ++s) CHECK(m.find(pool[s]) == kNone);
    }
    // one-bit variants: byte 0, the sign bit (byte 31 bit 7), byte 31 bit 0
    for (uint32_t s = 0; s < lo; s += 7) {
      Key a = pool[s], b = pool[s], c = pool[s];
      a[0] ^= 1; b[31] ^= 0x80; c[31] ^= 1;
      CHECK(m.find(a) == kNone && m.find(b) == kNone && m.find(c) == kNone);
    }
    // a count below a stored slot passes over it
    CHECK(m.find(pool[600], 601) == 600 && m.find(pool[600], 600) == kNone && m.find(pool[0], 0) == kNone);
  }
  {                                                    // the same bytes in slots 17 / 200 / 299
    Model m(1024);
    std::vector<Key> ks = random_keys(300);
    ks[200] = ks[17];
    ks[299] = ks[17];
    const Key k = ks[17];
    m.load(ks);
    CHECK(m.find(k) == 17 && m.left == 0);
    m.replace(17, random_key());
    CHECK(m.find(k) == 200 && m.check() == 0);
    m.replace(200, random_key());
    CHECK(m.find(k) == 299);
    m.replace(299, random_key());
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
  printf("edkidx ok\n");
  return 0;
}
