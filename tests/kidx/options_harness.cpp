// The rows of "ed_keys_index" and "ed_keys_index_seed" in csrc/gv_options.h as
// a program of its own.  Prints one "name = value(s)" line per case;
// tests/test_ed_keys_index_host.py holds the expected numbers.  Test
// infrastructure only.
//   g++ -std=c++17 -Icosmos-sdk-rootchain_amd/csrc tests/kidx/options_harness.cpp
#include <cstdio>
#include <initializer_list>

#include "gv_options.h"

bool gvopt::kg_layout_ok(int ng) { return ng == 0 || ng == 4 || ng == 6 || ng == 7 || ng == 9; }
bool gvopt::kw_width_ok(int qw) { return qw == 11 || qw == 9; }

using namespace gvopt;

int main() {
  for (const char* key : {"ed_keys_index", "ed_keys_index_seed"}) {
    const Row* r = opt_find(key);
    printf("%s found = %d\n", key, r != nullptr);
    if (!r) return 1;
    bool in_first = false, in_later = false;
    for (const Row& q : kRows) in_first |= q.name && !strcmp(q.name, key);
    for (const Row& q : kRowsLater) in_later |= q.name && !strcmp(q.name, key);
    printf("%s in kRows = %d\n", key, (int)in_first);
    printf("%s in kRowsLater = %d\n", key, (int)in_later);
    printf("%s env = %s\n", key, r->env ? r->env : "-");
    printf("%s env rule = %d\n", key, (int)(r->env_rule == E_IS1));
    printf("%s readable = %d\n", key, (int)r->readable);
    printf("%s effect = %s\n", key,
           r->fx == FX_ED_KEYS_MU ? "ed_keys_mu" : r->fx == FX_ED_KEYS_EMPTY ? "ed_keys_empty" : "other");
  }
  const Row* r = opt_find("ed_keys_index");
  Options o;
  printf("default = %lld\n", opt_read(o, *r));
  const long long vals[] = {-2, -1, 0, 1, 2, 3, 6, 8, 255, 256, 1ll << 32, (1ll << 32) + 1, -(1ll << 32)};
  for (long long v : vals) {
    Options p;
    const int fx = opt_check_and_store(p, *r, v);
    printf("set %lld = %d %lld\n", v, fx < 0 ? 0 : 1, opt_read(p, *r));
  }
  // the variable alone: on for exactly "1"
  for (const char* s : {"0", "1", "2", "11", "abc", "", " 1", "true"}) {
    Options e;
    opt_from_env(e, [&](const char* name) -> const char* { return !strcmp(name, "GV_ED_KEYS_INDEX") ? s : nullptr; });
    printf("env '%s' = %d %d\n", s, (int)e.ed_keys_index, (int)e.keys_index);
  }
  // every other variable at "1" leaves it off
  Options e;
  opt_from_env(e, [](const char* name) -> const char* { return strcmp(name, "GV_ED_KEYS_INDEX") ? "1" : nullptr; });
  printf("others = %d\n", (int)e.ed_keys_index);
  printf("options ok\n");
  return 0;
}
