// The host-side pieces of "keys_index_split" as a program of its own: the
// option's row in csrc/gv_options.h, and the split decision, the buffers'
// growth rule and their layout in csrc/gv_keytabs.h.  Prints one
// "name = value(s)" line per case; tests/test_keys_index_split_host.py holds
// the expected numbers and also runs this under ASan + UBSan.  Test
// infrastructure only.
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM/include -Icsrc tests/kidx/split_harness.cpp
#include <cstdio>

#include "gv_keytabs.h"
#include "gv_options.h"

bool gvopt::kg_layout_ok(int ng) { return ng == 0 || ng == 4 || ng == 6 || ng == 7 || ng == 9; }
bool gvopt::kw_width_ok(int qw) { return qw == 11 || qw == 9; }

using namespace gvopt;
using namespace gvkt;

static void put(const char* name, long long v) { printf("%s = %lld\n", name, v); }

int main() {
  const char* key = "keys_index_split";
  const Row* r = opt_find(key);
  put("found", r != nullptr);
  if (!r) return 1;
  bool in_first = false, in_later = false;
  for (const Row& q : kRows) in_first |= q.name && !strcmp(q.name, key);
  for (const Row& q : kRowsLater) in_later |= q.name && !strcmp(q.name, key);
  put("in kRows", in_first);
  put("in kRowsLater", in_later);
  put("env", r->env != nullptr);
  put("env rule", r->env_rule);
  put("readable", r->readable);
  put("max items", (long long)kMaxItems);
  Options o;
  put("default", opt_read(o, *r));
  const long long vals[] = {-1, 0, 1, 4096, (long long)kMaxItems, (long long)kMaxItems + 1};
  for (long long v : vals) {
    Options p;
    p.keys_index_split = 77;
    const int fx = opt_check_and_store(p, *r, v);
    char name[64];
    snprintf(name, sizeof name, "set %lld", v);
    printf("%s = %d %lld\n", name, fx < 0 ? 0 : 1, opt_read(p, *r));
  }
  // every variable of the environment at "5": the option keeps its default
  Options e;
  opt_from_env(e, [](const char*) { return "5"; });
  put("after env", (long long)e.keys_index_split);

  // the decision: (bound, miss, live, buffers)
  const struct {
    size_t bound, miss;
    bool live, buffers;
  } cases[] = {{0, 0, true, true},  {0, 1, true, true},   {8, 0, true, true},  {8, 1, true, true},
               {8, 8, true, true},  {8, 9, true, true},   {8, 1, false, true}, {8, 8, false, true},
               {8, 1, true, false}, {8, 8, true, false},  {1, 1, true, true},  {1, 2, true, true},
               {kMaxItems, kMaxItems, true, true},        {kMaxItems, 1, false, false}};
  for (const auto& c : cases) {
    char name[96];
    snprintf(name, sizeof name, "split %zu %zu %d %d", c.bound, c.miss, (int)c.live, (int)c.buffers);
    put(name, kidx_split_ok(c.bound, c.miss, c.live, c.buffers));
  }
  const size_t rows[][2] = {{0, 1}, {0, 256}, {0, 257}, {256, 1}, {256, 256}, {256, 257}, {256, 600}, {512, 513},
                            {1024, 100}, {0, 65536}};
  for (const auto& g : rows) {
    char name[64];
    snprintf(name, sizeof name, "rows %zu %zu", g[0], g[1]);
    put(name, (long long)kidx_split_rows(g[0], g[1]));
  }
  for (size_t c : {(size_t)0, (size_t)256, (size_t)512, (size_t)65536}) {
    const SplitLayout L = kidx_split_layout(c);
    char name[64];
    snprintf(name, sizeof name, "layout %zu", c);
    printf("%s = %zu %zu %zu %zu %zu %zu %zu\n", name, L.idx, L.pub, L.sig, L.third, L.len, L.bits, L.total);
  }
  printf("split ok\n");
  return 0;
}
