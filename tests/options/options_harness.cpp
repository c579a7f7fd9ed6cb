// Drives csrc/gv_options.h (the runtime's option table; host-only) for
// tests/test_options_host.py, built by g++:
//
//   options_harness rows              one line per row: its name, environment
//                                     name, effect tag and readable flag
//   options_harness probe V...        what gv_set_option / gv_get_option do
//                                     over a fresh Options for every named row
//                                     and probe value V, in the record format
//                                     of tools/record_options.py
//   options_harness env S             each row's environment variable alone at
//                                     the string S: the raw member afterwards
//
// The two build facts the table asks for are the library's (gv_kernels.h
// GV_KG_NGS, GV_KW_QW / GV_KWN_QW), written out here: gv_kernels.h needs HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../cosmos-sdk-rootchain_amd/csrc/gv_options.h"

bool gvopt::kg_layout_ok(int ng) { return ng == 0 || ng == 4 || ng == 6 || ng == 7 || ng == 9; }
bool gvopt::kw_width_ok(int qw) { return qw == 11 || qw == 9; }

using namespace gvopt;

static const char* or_dash(const char* s) { return s ? s : "-"; }

// gv_get_option over the table: the return code and the value.
static void get(const Options& o, const char* key, int* rc, long long* v) {
  const Row* r = key ? opt_find(key) : nullptr;
  *rc = r && r->readable ? GV_OK : GV_EINVAL;
  *v = *rc == GV_OK ? opt_read(o, *r) : 0;
}

static long long raw(const Options& o, const Row& r) {
  return r.f.b ? (long long)(o.*r.f.b) : r.f.i ? (long long)(o.*r.f.i) : (long long)(o.*r.f.z);
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "rows")) {
    for (const Row& r : kRows) printf("row %s %s %d %d\n", or_dash(r.name), or_dash(r.env), (int)r.fx, (int)r.readable);
    return 0;
  }
  if (argc >= 2 && !strcmp(argv[1], "probe")) {
    for (const Row& r : kRows) {
      if (!r.name) continue;
      // the coupled key: the row whose member this row also writes
      const char* other = nullptr;
      for (const Row& c : kRows)
        if (r.also && c.name && c.f.z == r.also && !c.also) other = c.name;
      Options o;
      int rc, crc;
      long long v, cv;
      get(o, r.name, &rc, &v);
      printf("default %s %s %d %lld\n", r.name, or_dash(other), rc, v);
      for (int i = 2; i < argc; ++i) {
        const long long val = strtoll(argv[i], nullptr, 10);
        const int src = opt_check_and_store(o, r, val) < 0 ? GV_EINVAL : GV_OK;
        get(o, r.name, &rc, &v);
        get(o, other, &crc, &cv);
        printf("set %s %lld %d %d %lld %d %lld\n", r.name, val, src, rc, v, crc, cv);
      }
    }
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "env")) {
    for (const Row& r : kRows) {
      if (!r.env) continue;
      Options o;
      opt_from_env(o, [&](const char* name) -> const char* { return !strcmp(name, r.env) ? argv[2] : nullptr; });
      printf("env %s %lld\n", r.env, raw(o, r));
    }
    return 0;
  }
  fprintf(stderr, "usage: options_harness rows | probe V... | env S\n");
  return 2;
}
