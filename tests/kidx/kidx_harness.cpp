// The pubkey index's host model (tools/fe29/kidx_host.cpp over csrc/gv_kidx.h)
// as a program of its own, for ASan + UBSan: the scenarios of
// tests/test_keys_index_host.py and tests/test_ed_keys_index_host.py against a
// std::map, once per arena -- 9-word rows of 33-byte keys, 8-word rows of
// 32-byte keys.  Exit 0 and one line per arena, "kidx ok" and "edkidx ok", when
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
const uint64_t kSeed = 0x0123456789ABCDEFull;
const uint32_t kNone = 0xFFFFFFFFu;
int failures = 0;
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) { printf("FAIL %s:%d (R = %d): %s\n", __FILE__, __LINE__, R, #c); ++failures; } \
  } while (0)

// One arena's scenarios: R words per row, KB key bytes.
template <int R>
struct Arena {
  static constexpr int KB = gv_kidx_key<R>::bytes;
  typedef std::array<uint8_t, KB> Key;

  struct Model {
    uint32_t T;
    std::vector<Key> keys;                             // by slot
    std::vector<uint32_t> rows, table;
    uint32_t left = 0;
    explicit Model(uint32_t t) : T(t), table(t, kNone) {}
    void load(const std::vector<Key>& ks) {
      const uint32_t base = (uint32_t)keys.size();
      keys.insert(keys.end(), ks.begin(), ks.end());
      rows.resize(keys.size() * R);
      kidx_host::rows<R>(ks[0].data(), (uint32_t)ks.size(), base, nullptr, rows.data());
      left += kidx_host::put<R>(table.data(), T, rows.data(), (uint32_t)ks.size(), base, nullptr, kSeed);
    }
    void replace(uint32_t slot, const Key& k) {        // the row, then the table refilled from every row
      keys[slot] = k;
      kidx_host::rows<R>(k.data(), 1, 0, &slot, rows.data());
      kidx_clear(table.data(), T);
      left = kidx_host::put<R>(table.data(), T, rows.data(), (uint32_t)keys.size(), 0, nullptr, kSeed);
    }
    // (the key at offset 0 and at offset 1 of a buffer: the row loader takes
    // any alignment)
    uint32_t find(const Key& k, uint32_t count) const {
      alignas(4) uint8_t buf[KB + 1];
      uint32_t out[2] = {12345, 12345};
      for (int o = 0; o < 2; ++o) {
        memcpy(buf + o, k.data(), KB);
        kidx_host::find<R>(table.data(), T, rows.data(), count, kSeed, buf + o, 1, &out[o]);
      }
      CHECK(out[0] == out[1]);
      return out[0];
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

  std::mt19937_64 rng{20240611u + R};
  Key random_key() {
    Key k;
    for (auto& b : k) b = (uint8_t)rng();
    if (KB == 33) k[0] = (uint8_t)(2 + (k[0] & 1));
    return k;
  }
  std::vector<Key> random_keys(size_t n) {
    std::vector<Key> ks(n);
    for (auto& k : ks) k = random_key();
    return ks;
  }
  std::vector<Key> homed(uint32_t T, uint32_t home, uint32_t want, uint64_t stream) {
    std::vector<uint8_t> buf((size_t)want * KB);
    const uint32_t got = kidx_host::search_home<R>(kSeed, T, home, want, stream, 1ull << 26, buf.data());
    CHECK(got == want);
    std::vector<Key> ks(got);
    for (uint32_t i = 0; i < got; ++i) memcpy(ks[i].data(), &buf[(size_t)i * KB], KB);
    return ks;
  }

  void run() {
    {                                                  // random keys, unknown keys
      Model m(8192);
      const std::vector<Key> ks = random_keys(2000);
      m.load(ks);
      CHECK(m.left == 0 && m.check() == 0);
      for (int i = 0; i < 500; ++i) CHECK(m.find(random_key()) == kNone);
      for (uint32_t s = 0; s < 2000; ++s) CHECK(m.find(ks[s]) == s);
    }
    {                                                  // the leading bytes shared, the last 16 differ
      Model m(8192);
      std::vector<Key> ks(300, random_key());
      for (auto& k : ks)
        for (int i = KB - 16; i < KB; ++i) k[i] = (uint8_t)rng();
      m.load(ks);
      CHECK(m.left == 0 && m.check() == 0);
    }
    {                                                  // loads of 1 / 255 / 256 / 257 keys in turn
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
      // one-bit variants: byte 0 (a pub33's prefix), the last byte's bit 7 (a
      // pub32's sign bit) and bit 0, the byte behind a pub33's prefix
      for (uint32_t s = 0; s < lo; s += 7) {
        Key a = pool[s], b = pool[s], c = pool[s], d = pool[s];
        a[0] ^= 1; b[KB - 1] ^= 0x80; c[KB - 1] ^= 1; d[1] ^= 0x80;
        CHECK(m.find(a) == kNone && m.find(b) == kNone && m.find(c) == kNone && m.find(d) == kNone);
      }
      // a count below a stored slot passes over it
      CHECK(m.find(pool[600], 601) == 600 && m.find(pool[600], 600) == kNone && m.find(pool[0], 0) == kNone);
    }
    {                                                  // one-byte neighbours side by side in the table
      Model m(512);
      Key a = random_key(), b = a, c = a, d = a;
      b[0] ^= 1; c[KB - 1] ^= 1; d[1] ^= 0x80;
      m.load({a, b, c, d});
      CHECK(m.find(a) == 0 && m.find(b) == 1 && m.find(c) == 2 && m.find(d) == 3);
      Key e = a;
      e[16] ^= 4;
      CHECK(m.find(e) == kNone);
    }
    {                                                  // the same bytes in three slots, few keys
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
    {                                                  // ... and in slots 17 / 200 / 299 of 300
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
    {                                                  // home word T - 1: the probe wraps to word 0
      Model m(512);
      const std::vector<Key> ks = homed(512, 511, 3, 7);
      m.load(ks);
      CHECK(m.table[511] == 0 && m.table[0] == 1 && m.table[1] == 2);
      CHECK(m.left == 0 && m.check() == 0);
    }
    {                                                  // the bound: PROBE + 6 keys of one home word
      Model m(512);
      const std::vector<Key> ks = homed(512, 100, GV_KIDX_PROBE + 6, 11);
      m.load(ks);
      CHECK(m.left == 6);
      CHECK(m.check() == 6);
      for (uint32_t s = 0; s < ks.size(); ++s) CHECK(m.find(ks[s]) == (s < GV_KIDX_PROBE ? s : kNone));
    }
  }
};
}  // namespace

int main() {
  if (kidx_row_words() != 9 || edkidx_row_words() != 8 || kidx_probe_bound() != 64 || edkidx_probe_bound() != 64) {
    printf("FAIL: row words or probe bound\n");
    return 1;
  }
  Arena<GV_KIDX_ROW>().run();
  if (!failures) printf("kidx ok\n");
  const int before = failures;
  Arena<GV_KIDX_ROW_ED>().run();
  if (failures == before) printf("edkidx ok\n");
  return failures ? 1 : 0;
}
