// secp_lane_ops.cuh -- the secp256k1 op body of gv_debug_lane_op: ONE item,
// one call of one function of the one-lane 9 x 29 layers (secp_fe29.cuh,
// secp_fe29x.cuh, secp_group29.cuh, secp_group29x.cuh) on raw limbs.  The same
// body is compiled three times: k_debug_lane (gv_kernels.hip, one mad chain
// per column), k_debug_lane_lat (gv_lat.hip, -DF29_NCH=2 -DF29X_NCH=2) and the
// g++ host build with the GV_F29_CHECK traps (tools/fe29/lane_host.cpp), so
// the device limbs can be compared with the trapped host run limb for limb.
// Item layout and op codes: gv_lane.h.  o is zero on entry.
#pragma once
#include "secp_group29x.cuh"
#include "gv_lane.h"

namespace gv {

GV_DEV void ln_ld(fe29& r, const u32* p) {
#pragma unroll
  for (int i = 0; i < 9; ++i) r.n[i] = p[i];
}
GV_DEV void ln_st(u32* o, int slot, const fe29& a) {
#pragma unroll
  for (int i = 0; i < 9; ++i) o[16 * slot + i] = a.n[i];
}
GV_DEV void ln_ld_gej(gej29& p, const u32* it) {
  ln_ld(p.x, it);
  ln_ld(p.y, it + 9);
  ln_ld(p.z, it + 18);
}
GV_DEV void ln_st_gej(u32* o, const gej29& p) {
  ln_st(o, 0, p.x);
  ln_st(o, 1, p.y);
  ln_st(o, 2, p.z);
}
#define LN_A(v, j) fe29 v; ln_ld(v, it + 9 * (j))

GV_DEV void lane_secp_op(int op, const u32* it, u32* o) {
  const u32 flags = it[GV_LN_IN - 1];
  const bool wop = op == GV_LNOP_FROM_WORDS;
  if (wop != ((flags & GV_LNF_WORDS) != 0u)) return;   // words where the op takes limbs, or the reverse: not run
  u32 flag = 0u, inf_out = 0u, known = 1u;
  fe29 r;
  switch (op) {
    case GV_LNOP_MUL: { LN_A(a, 0); LN_A(b, 1); f29_mul(r, a, b); ln_st(o, 0, r); break; }
    case GV_LNOP_SQR: { LN_A(a, 0); f29_sqr(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_MULTI_SS: {
      fe29 x[2], q[2];
      ln_ld(x[0], it); ln_ld(x[1], it + 9);
      f29_multi<true, true>(q, x, x);
      ln_st(o, 0, q[0]); ln_st(o, 1, q[1]);
      break;
    }
    case GV_LNOP_MULTI_MMM: {
      fe29 x[3], y[3], q[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) { ln_ld(x[s], it + 9 * s); ln_ld(y[s], it + 9 * (3 + s)); }
      f29_multi<false, false, false>(q, x, y);
#pragma unroll
      for (int s = 0; s < 3; ++s) ln_st(o, s, q[s]);
      break;
    }
    case GV_LNOP_MULTI_MM: {
      fe29 x[2], y[2], q[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) { ln_ld(x[s], it + 9 * s); ln_ld(y[s], it + 9 * (2 + s)); }
      f29_multi<false, false>(q, x, y);
      ln_st(o, 0, q[0]); ln_st(o, 1, q[1]);
      break;
    }
    case GV_LNOP_MULTI_SSM: {
      fe29 x[3], y[3], q[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) { ln_ld(x[s], it + 9 * s); y[s] = x[s]; }
      ln_ld(y[2], it + 27);
      f29_multi<true, true, false>(q, x, y);
#pragma unroll
      for (int s = 0; s < 3; ++s) ln_st(o, s, q[s]);
      break;
    }
    case GV_LNOP_SUB1: { LN_A(a, 0); LN_A(b, 1); f29_sub<1>(r, a, b); ln_st(o, 0, r); break; }
    case GV_LNOP_NEG1: { LN_A(a, 0); f29_neg<1>(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_SUB_NORM1: { LN_A(a, 0); LN_A(b, 1); f29_sub_norm<1>(r, a, b); ln_st(o, 0, r); break; }
    case GV_LNOP_SUB_NORM2: { LN_A(a, 0); LN_A(b, 1); f29_sub_norm<2>(r, a, b); ln_st(o, 0, r); break; }
    case GV_LNOP_SUB_NORM3: { LN_A(a, 0); LN_A(b, 1); f29_sub_norm<3>(r, a, b); ln_st(o, 0, r); break; }
    case GV_LNOP_SHL_NORM1: { LN_A(a, 0); f29_shl_norm<1>(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_SHL_NORM2: { LN_A(a, 0); f29_shl_norm<2>(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_SHL_NORM3: { LN_A(a, 0); f29_shl_norm<3>(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_MUL3_NORM: { LN_A(a, 0); f29_mul3_norm(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_NORM: { LN_A(a, 0); f29_norm(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_TO_WORDS: {
      LN_A(a, 0);
      u32 w[8];
      f29_to_words(w, a);
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = w[i];
      break;
    }
    case GV_LNOP_FROM_WORDS: {
      u32 w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) w[i] = it[i];
      f29_from_words(r, w);
      ln_st(o, 0, r);
      break;
    }
    case GV_LNOP_IS_ZERO: { LN_A(a, 0); flag = f29_is_zero(a) ? 1u : 0u; break; }
    case GV_LNOP_IS_ZERO_FAST: { LN_A(a, 0); flag = f29_is_zero_fast(a) ? 1u : 0u; break; }
    case GV_LNOP_EQUAL: { LN_A(a, 0); LN_A(b, 1); flag = f29_equal(a, b) ? 1u : 0u; break; }
    case GV_LNOP_INV: { LN_A(a, 0); f29_inv(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_SQRT: { LN_A(a, 0); f29_sqrt_candidate(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_X_MUL: { LN_A(a, 0); LN_A(b, 1); f29x_mul(r, a, b); ln_st(o, 0, r); break; }
    case GV_LNOP_X_MUL_P1: {
      LN_A(a, 0); LN_A(b, 1); LN_A(c, 2);
      f29x_mul(r, a, b, f29x_plus<1>{c.n});
      ln_st(o, 0, r);
      break;
    }
    case GV_LNOP_X_MUL_P8: {
      LN_A(a, 0); LN_A(b, 1); LN_A(c, 2);
      f29x_mul(r, a, b, f29x_plus<8>{c.n});
      ln_st(o, 0, r);
      break;
    }
    case GV_LNOP_X_MUL2: {
      LN_A(a, 0); LN_A(b, 1); LN_A(c, 2); LN_A(d, 3);
      f29x_mul2(r, a, b, c, d);
      ln_st(o, 0, r);
      break;
    }
    case GV_LNOP_X_SQR: { LN_A(a, 0); f29x_sqr(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_X_SQRD_P1: {
      LN_A(a, 0); LN_A(c, 1);
      fe29 d;
      f29x_shl1(d, a);
      f29x_sqr_d(r, a, d, f29x_plus<1>{c.n});
      ln_st(o, 0, r);
      break;
    }
    case GV_LNOP_X_SQRD_P8: {
      LN_A(a, 0); LN_A(c, 1);
      fe29 d;
      f29x_shl1(d, a);
      f29x_sqr_d(r, a, d, f29x_plus<8>{c.n});
      ln_st(o, 0, r);
      break;
    }
    case GV_LNOP_X_SQR3: { LN_A(a, 0); f29x_sqr3(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_X_SQRT: { LN_A(a, 0); f29x_sqrt_candidate(r, a); ln_st(o, 0, r); break; }
    case GV_LNOP_GEJ_DOUBLE: {
      gej29 p;
      ln_ld_gej(p, it);
      gej29_double(p, p);
      ln_st_gej(o, p);
      break;
    }
    case GV_LNOP_GEJ_ADD_GE: {
      gej29 p;
      ln_ld_gej(p, it);
      LN_A(x, 3); LN_A(y, 4);
      bool inf = false;
      gej29_add_ge(p, inf, x, y);
      ln_st_gej(o, p);
      inf_out = inf ? 1u : 0u;
      break;
    }
    case GV_LNOP_GEJ_ADD_GEJ: {
      gej29 p, q, s;
      ln_ld_gej(p, it);
      ln_ld_gej(q, it + 27);
      bool inf = false;
      gej29_add_gej(s, inf, p, (flags & GV_LNF_INF_A) != 0u, q, (flags & GV_LNF_INF_B) != 0u);
      ln_st_gej(o, s);
      inf_out = inf ? 1u : 0u;
      break;
    }
    case GV_LNOP_GEJX_DOUBLE: {
      gej29 p;
      ln_ld_gej(p, it);
      gej29x_double(p, p);
      ln_st_gej(o, p);
      break;
    }
    case GV_LNOP_GEJX_ADD_SCALED: {
      gej29 p;
      ln_ld_gej(p, it);
      LN_A(x, 3); LN_A(y, 4); LN_A(az, 5);
      bool inf = false;
      gej29x_add_scaled(p, inf, x, y, az);
      ln_st_gej(o, p);
      inf_out = inf ? 1u : 0u;
      break;
    }
    default: known = 0u; break;
  }
  o[64 + GV_LNS_FLAG] = flag;
  o[64 + GV_LNS_INF] = inf_out;
  o[64 + GV_LNS_KNOWN] = known;
}

}  // namespace gv
