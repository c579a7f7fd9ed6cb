// Host build of the comb-digit recoding k_ed_keyed runs (csrc/ed_scalar.cuh
// ed_comb_digit / ed_comb_windows) for tests/test_ed_comb_host.py (ctypes):
// the exact source of the gfx950 kernel, checked against Python integers.
#include "../../cosmos-sdk-rootchain_amd/csrc/ed_scalar.cuh"
using namespace gv::ed;

template <int RB>
static int recode(const uint32_t* h, int* digits) {
  int cin = 0;
  for (int w = 0; w < ed_comb_windows<RB>(); ++w) digits[w] = ed_comb_digit<RB>(h, w, cin);
  return cin == 0 ? ed_comb_windows<RB>() : -2;       // a carry out of the top window is never produced
}

extern "C" {
// digits[0..NW) of h (8 little-endian words, h < 2^253) at radix 2^rb;
// returns NW, or -1 for a radix the kernels do not have
int edc_recode(int rb, const uint32_t* h, int* digits) {
  switch (rb) {
    case 4: return recode<4>(h, digits);
    case 6: return recode<6>(h, digits);
    case 8: return recode<8>(h, digits);
    default: return -1;
  }
}
}
