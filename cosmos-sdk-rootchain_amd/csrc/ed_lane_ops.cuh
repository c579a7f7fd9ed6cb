// ed_lane_ops.cuh -- the ed25519 op body of gv_debug_lane_op: ONE item, one
// call of one function of the one-lane layers (ed_fe29.cuh, ed_group.cuh,
// ed_scalar.cuh) on raw limbs or canonical words.  Compiled into
// k_debug_elane (ed_verify.hip) and into the g++ host build with the
// GV_F29_CHECK traps (tools/fe29/lane_host.cpp): the device limbs can be
// compared with the trapped host run limb for limb.  Item layout and op
// codes: gv_lane.h.  o is zero on entry; tab / stride: this item's j(-A)
// table scratch (ED_ATAB_WORDS words, word k at tab[k * stride]).
#pragma once
#include "ed_group.cuh"
#include "gv_lane.h"

namespace gv {
namespace ed {

GV_DEV void eln_ld(fe29& r, const u32* p) {
#pragma unroll
  for (int i = 0; i < 9; ++i) r.n[i] = p[i];
}
GV_DEV void eln_st(u32* o, int slot, const fe29& a) {
#pragma unroll
  for (int i = 0; i < 9; ++i) o[16 * slot + i] = a.n[i];
}
GV_DEV void eln_ld_ext(ge_ext& p, const u32* it) {
  eln_ld(p.X, it);
  eln_ld(p.Y, it + 9);
  eln_ld(p.Z, it + 18);
  eln_ld(p.T, it + 27);
}
GV_DEV void eln_st_ext(u32* o, const ge_ext& p, bool t_out = true) {
  eln_st(o, 0, p.X);
  eln_st(o, 1, p.Y);
  eln_st(o, 2, p.Z);
  if (t_out) eln_st(o, 3, p.T);
}
template <int RB>
GV_DEV void eln_comb(u32* o, const u32 h[8]) {
  int cin = 0;
  for (int w = 0; w < ed_comb_windows<RB>(); ++w) o[w] = (u32)ed_comb_digit<RB>(h, w, cin);
}
#define ELN_A(v, j) fe29 v; eln_ld(v, it + 9 * (j))

GV_DEV void lane_ed_op(int op, const u32* it, u32* o, u32* tab, size_t stride) {
  const u32 flags = it[GV_LN_IN - 1];
  const bool neg = (flags & GV_LNF_NEG) != 0u;
  const bool wop = op == GV_LNOP_ED_FROM_WORDS || op == GV_LNOP_GE_FROMBYTES || op >= GV_LNOP_SC_REDUCE512;
  if (wop != ((flags & GV_LNF_WORDS) != 0u)) return;   // words where the op takes limbs, or the reverse: not run
  u32 flag = 0u, known = 1u;
  u32 w[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = wop ? it[i] : 0u;
  fe29 r;
  switch (op) {
    case GV_LNOP_ED_MUL: { ELN_A(a, 0); ELN_A(b, 1); e29_mul(r, a, b); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_SQR: { ELN_A(a, 0); e29_sqr(r, a); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_SUB1: { ELN_A(a, 0); ELN_A(b, 1); e29_sub<1>(r, a, b); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_NEG1: { ELN_A(a, 0); e29_neg<1>(r, a); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_SUB_NORM1: { ELN_A(a, 0); ELN_A(b, 1); e29_sub_norm<1>(r, a, b); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_SUB_NORM2: { ELN_A(a, 0); ELN_A(b, 1); e29_sub_norm<2>(r, a, b); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_SUB_NORM3: { ELN_A(a, 0); ELN_A(b, 1); e29_sub_norm<3>(r, a, b); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_ADD_NORM: { ELN_A(a, 0); ELN_A(b, 1); e29_add_norm(r, a, b); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_NORM: { ELN_A(a, 0); e29_norm(r, a); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_TO_WORDS: {
      ELN_A(a, 0);
      u32 t[8];
      e29_to_words(t, a);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = t[i];
      break;
    }
    case GV_LNOP_ED_FROM_WORDS: { e29_from_words(r, w); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_IS_ZERO: { ELN_A(a, 0); flag = e29_is_zero(a) ? 1u : 0u; break; }
    case GV_LNOP_ED_IS_NEGATIVE: { ELN_A(a, 0); flag = e29_is_negative(a); break; }
    case GV_LNOP_ED_INV: { ELN_A(a, 0); e29_inv(r, a); eln_st(o, 0, r); break; }
    case GV_LNOP_ED_POW22523: { ELN_A(a, 0); e29_pow22523(r, a); eln_st(o, 0, r); break; }
    case GV_LNOP_GE_DBL_T: {
      ge_ext p, q;
      eln_ld_ext(p, it);
      ge_dbl_t<true>(q, p);
      eln_st_ext(o, q);
      break;
    }
    case GV_LNOP_GE_DBL_NT: {
      ge_ext p, q;
      eln_ld_ext(p, it);
      ge_dbl_t<false>(q, p);
      eln_st_ext(o, q, false);
      break;
    }
    case GV_LNOP_GE_ADD_CACHED: {
      ge_ext p;
      eln_ld_ext(p, it);
      ge_cached c;
      eln_ld(c.ypx, it + 36); eln_ld(c.ymx, it + 45); eln_ld(c.z2, it + 54); eln_ld(c.t2d, it + 63);
      ge_add_cached(p, p, c, neg);
      eln_st_ext(o, p);
      break;
    }
    case GV_LNOP_GE_ADD_PRE: {
      ge_ext p;
      eln_ld_ext(p, it);
      ge_pre c;
      eln_ld(c.ypx, it + 36); eln_ld(c.ymx, it + 45); eln_ld(c.xy2d, it + 54);
      ge_add_pre(p, p, c, neg);
      eln_st_ext(o, p);
      break;
    }
    case GV_LNOP_GE_TO_CACHED: {
      ge_ext p;
      eln_ld_ext(p, it);
      ge_cached c;
      ge_to_cached(c, p);
      eln_st(o, 0, c.ypx); eln_st(o, 1, c.ymx); eln_st(o, 2, c.z2); eln_st(o, 3, c.t2d);
      break;
    }
    case GV_LNOP_GE_TO_PRE: {
      ge_ext p;
      eln_ld_ext(p, it);
      ge_pre c;
      ge_to_pre(c, p);
      eln_st(o, 0, c.ypx); eln_st(o, 1, c.ymx); eln_st(o, 2, c.xy2d);
      break;
    }
    case GV_LNOP_GE_NEG: {
      ge_ext p, q;
      eln_ld_ext(p, it);
      ge_neg(q, p);
      eln_st_ext(o, q);
      break;
    }
    case GV_LNOP_GE_FROMBYTES: {
      ge_ext p;
      flag = ge_frombytes(p, w) ? 1u : 0u;
      eln_st_ext(o, p);
      break;
    }
    case GV_LNOP_GE_TOBYTES: {
      ge_ext p;
      eln_ld_ext(p, it);
      u32 t[8];
      ge_tobytes(t, p);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = t[i];
      break;
    }
    case GV_LNOP_GE_ADD_TAB: {
      const int e = (int)((flags >> GV_LNF_ENTRY_SHIFT) & 15u);
      if (e >= ED_ATAB_ENTRIES) { known = 0u; break; }   // no such entry: nothing read or written
      ge_ext p, a;
      eln_ld_ext(p, it);
      eln_ld_ext(a, it + 36);
      atab_build(tab, stride, a);
      if (flags & GV_LNF_NOT) {
        ge_add_tab<false>(p, p, tab, stride, e, neg);
        eln_st_ext(o, p, false);
      } else {
        ge_add_tab<true>(p, p, tab, stride, e, neg);
        eln_st_ext(o, p);
      }
      break;
    }
    case GV_LNOP_SC_REDUCE512: {
      u32 t[8];
      sc_reduce512(t, w);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = t[i];
      break;
    }
    case GV_LNOP_SC_MINIMAL: flag = sc_minimal(w) ? 1u : 0u; break;
    case GV_LNOP_ED_RADIX16: {                        // ed_ladder_check's digits of h, digit i in word i
      const uint64_t carries = sc_radix16_carries(w);
      for (int i = 0; i < 64; ++i) {
        const int nib = (int)((w[i >> 3] >> (4 * (i & 7))) & 15u);
        const int cin = i > 0 ? (int)((carries >> (i - 1)) & 1u) : 0;
        const int cout = i < 63 ? (int)((carries >> i) & 1u) : 0;
        o[i] = (u32)(nib + cin - 16 * cout);
      }
      break;
    }
    case GV_LNOP_ED_COMB4: eln_comb<4>(o, w); break;
    case GV_LNOP_ED_COMB6: eln_comb<6>(o, w); break;
    case GV_LNOP_ED_COMB8: eln_comb<8>(o, w); break;
    default: known = 0u; break;
  }
  o[64 + GV_LNS_FLAG] = flag;
  o[64 + GV_LNS_KNOWN] = known;
}

}  // namespace ed
}  // namespace gv
