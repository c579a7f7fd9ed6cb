// Host build of the op bodies of gv_debug_lane_op (csrc/secp_lane_ops.cuh,
// csrc/ed_lane_ops.cuh): every function of the one-lane 9 x 29 layers the
// device hook runs, from the same headers, with the fe29 overflow traps on
// (any wrapping u64 mad or u32 limb add aborts the process), for
// tests/test_lane_host.py and tests/test_lane_gpu.py (ctypes).  Build with
// -I <the csrc directory>; -DF29_NCH=2 -DF29X_NCH=2 gives the two-chain
// configuration of gv_lat.hip; -DLANE_NO_TRAPS leaves the traps out (the
// sharpness test's mutant builds, which must not be able to abort).
#ifndef LANE_NO_TRAPS
#define GV_F29_CHECK 1
#endif
#include <stddef.h>
#include "secp_lane_ops.cuh"
#include "ed_lane_ops.cuh"
#include <string.h>
#include <vector>

// n items in the hook's layout: in n x GV_LN_IN words, out n x GV_LN_OUT.
// A secp256k1 op is given by its one-chain code in either build.  -1 for an
// op the hook refuses.
extern "C" int lane_host_ops(int op, size_t n, const uint32_t* in, uint32_t* out) {
  const bool secp = op >= 0 && op < GV_LNOP_SECP_END, ed = op >= GV_LNOP_ED_MUL && op < GV_LNOP_ED_END;
  if (!secp && !ed) return -1;
  memset(out, 0, n * GV_LN_OUT * 4);
  std::vector<uint32_t> tab(ED_ATAB_WORDS);
  for (size_t i = 0; i < n; ++i) {
    if (secp) gv::lane_secp_op(op, in + i * GV_LN_IN, out + i * GV_LN_OUT);
    else gv::ed::lane_ed_op(op, in + i * GV_LN_IN, out + i * GV_LN_OUT, tab.data(), 1);
  }
  return 0;
}
extern "C" int lane_host_chains(void) { return F29_NCH * 10 + F29X_NCH; }
