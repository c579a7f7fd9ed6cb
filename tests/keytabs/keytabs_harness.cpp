// csrc/gv_keytabs.h (the key table sets' layouts, bytes, growth rule, wide
// layout list and promotion arithmetic) as a program of its own: prints one
// "name = value(s)" line per evaluated case; tests/test_keytabs_host.py holds the
// expected numbers and also runs this under ASan + UBSan.  Test infrastructure only.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM/include -Icsrc tests/keytabs/keytabs_harness.cpp
#include <cstdio>

#include "gv_keytabs.h"

using namespace gvkt;

static void put(const char* name, unsigned long long v) { printf("%s = %llu\n", name, v); }

int main() {
  put("slot k4", slot_bytes(lay_k4()) + 4);
  put("resident k4", resident_slot_bytes(false));
  put("resident k4+kn", resident_slot_bytes(true));
  for (const WideLayout& w : kWideLayouts) {
    char name[64];
    snprintf(name, sizeof name, "slot wide %d %d", w.qw, w.ng);
    put(name, slot_bytes(lay_wide(w)));
    snprintf(name, sizeof name, "qw wide %d %d", w.qw, w.ng);
    put(name, (unsigned long long)lay_wide(w).qw());
  }
  put("slot none", slot_bytes(lay_wide(0, 0)));
  put("qw k4", (unsigned long long)lay_k4().qw());
  put("qw kn", (unsigned long long)lay_kn().qw());
  put("table words 3328", kidx_table_words(3328));
  put("table words 0", kidx_table_words(0));
  put("table words 256", kidx_table_words(256));
  put("table words 257", kidx_table_words(257));
  put("group k4", group_bytes(3328, lay_k4()));
  put("group kg4", group_bytes(3328, lay_kg(4)));
  put("group kg6", group_bytes(3328, lay_kg(6)));
  put("group kg7", group_bytes(3328, lay_kg(7)));
  put("group kg9", group_bytes(3328, lay_kg(9)));
  put("group k6", group_bytes(3328, lay_k6()));
  const size_t grow[][4] = {{0, 1, 4194304, 4096},       {4096, 4097, 4194304, 4096}, {4096, 20000, 4194304, 4096},
                            {4096, 4097, 5000, 4096},    {4194304, 4194305, 4194304, 4096},
                            {0, 1, 65536, 256},          {256, 300, 65536, 256}};
  for (const auto& g : grow) {
    char name[96];
    snprintf(name, sizeof name, "grow %zu %zu %zu %zu", g[0], g[1], g[2], g[3]);
    put(name, arena_grow_cap(g[0], g[1], g[2], g[3]));
  }
  put("layouts", kWideLayoutCount);
  for (int from = 0; from <= 4; ++from)
    for (int only : {0, 9, 11})
      for (int wpg : {1, 2}) {
        char name[64];
        snprintf(name, sizeof name, "next %d %d %d", from, only, wpg);
        put(name, (unsigned long long)wide_layout_next(from, only, wpg));
      }
  put("replace 1000 300 50", budget_replace(1000, 300, 50));
  put("replace 1000 1000 0", budget_replace(1000, 1000, 0));
  put("replace 1000 1001 7", budget_replace(1000, 1001, 7));
  put("replace 0 5 0", budget_replace(0, 5, 0));
  put("replace big", budget_replace((size_t)1 << 40, ((size_t)1 << 40) - 1, (size_t)3 << 40));
  put("promote rows", sizeof kPromoteCost / sizeof kPromoteCost[0]);
  put("promote none", promote_cost(4) == nullptr && promote_cost(0) == nullptr && promote_cost(8) == nullptr);
  const size_t n = 16384;
  const size_t built[][5] = {{6, 460, 461, 921, 922}, {7, 567, 568, 1135, 1136}, {9, 444, 445, 889, 890}};
  for (const auto& b : built) {
    const PromoteCost* c = promote_cost((int)b[0]);
    if (!c) return 1;
    char name[64];
    snprintf(name, sizeof name, "cost %d", c->ng);
    printf("%s = %llu %llu\n", name, (unsigned long long)c->key_ps, (unsigned long long)c->item_ps);
    for (int i = 1; i < 5; ++i) {
      snprintf(name, sizeof name, "promote %d %zu", c->ng, b[i]);
      printf("%s = %d %d\n", name, (int)promote_below_up(*c, b[i], n), (int)promote_above_down(*c, b[i], n));
    }
  }
  printf("keytabs ok\n");
  return 0;
}
