// gv_lane.h -- item layout and op codes of gv_debug_lane_op, the test hook of
// the one-lane 9 x 29 layers (one field element per lane).  Plain C: read by
// gv_kernels.h, by the op bodies (secp_lane_ops.cuh, ed_lane_ops.cuh) and by
// their g++ host build (tools/fe29/lane_host.cpp).  Mirrored in gpuverify.py
// (LNOP).
//
// The layout is gv_debug_sl_op's.  in: GV_LN_IN words per item -- operand j's
// nine raw limbs at 9j..9j+8 (j < 8), flags in the last word; ops taking
// canonical words (up to 16) read them from word 0 on and need GV_LNF_WORDS.
// out: GV_LN_OUT words per item -- four 16-word result slots (nine limbs or
// eight words, the rest zero; the digit ops fill all 64 words), then sixteen
// status words (GV_LNS_*).
#pragma once

#define GV_LN_IN 80
#define GV_LN_OUT 80
#define GV_LNF_NEG 1u        // ge_add_cached / ge_add_pre / ge_add_tab: subtract
#define GV_LNF_NOT 2u        // ge_add_tab<false>: no T out
#define GV_LNF_INF_A 4u
#define GV_LNF_INF_B 8u
#define GV_LNF_WORDS 16u
#define GV_LNF_ENTRY_SHIFT 8  // ge_add_tab: table entry 0..8 in bits 8..11
#define GV_LNS_FLAG 0        // boolean result (is_zero, equal, decode ok, sc_minimal)
#define GV_LNS_INF 1         // infinity out
#define GV_LNS_KNOWN 3       // the kernel knows the op and ran it

// secp256k1 ops: code c runs in k_debug_lane (gv_kernels.hip, one mad chain
// per column), c + GV_LNOP_LAT in k_debug_lane_lat (gv_lat.hip, two chains).
#define GV_LNOP_LAT 64
enum {
  GV_LNOP_MUL = 0, GV_LNOP_SQR,
  GV_LNOP_MULTI_SS,          // f29_multi<true, true>:          a0^2, a1^2
  GV_LNOP_MULTI_MMM,         // f29_multi<false, false, false>: a0 a3, a1 a4, a2 a5
  GV_LNOP_MULTI_MM,          // f29_multi<false, false>:        a0 a2, a1 a3
  GV_LNOP_MULTI_SSM,         // f29_multi<true, true, false>:   a0^2, a1^2, a2 a3
  GV_LNOP_SUB1, GV_LNOP_NEG1, GV_LNOP_SUB_NORM1, GV_LNOP_SUB_NORM2, GV_LNOP_SUB_NORM3,
  GV_LNOP_SHL_NORM1, GV_LNOP_SHL_NORM2, GV_LNOP_SHL_NORM3, GV_LNOP_MUL3_NORM, GV_LNOP_NORM,
  GV_LNOP_TO_WORDS, GV_LNOP_FROM_WORDS, GV_LNOP_IS_ZERO, GV_LNOP_IS_ZERO_FAST, GV_LNOP_EQUAL,
  GV_LNOP_INV, GV_LNOP_SQRT,
  GV_LNOP_X_MUL, GV_LNOP_X_MUL_P1, GV_LNOP_X_MUL_P8,      // a0 a1 (+ 1 a2, + 8 a2)
  GV_LNOP_X_MUL2,                                         // a0 a1 + a2 a3
  GV_LNOP_X_SQR, GV_LNOP_X_SQRD_P1, GV_LNOP_X_SQRD_P8,    // a0^2 (f29x_sqr_d with d = 2 a0: + 1 a1, + 8 a1)
  GV_LNOP_X_SQR3, GV_LNOP_X_SQRT,
  GV_LNOP_GEJ_DOUBLE,        // (a0, a1, a2)
  GV_LNOP_GEJ_ADD_GE,        // (a0, a1, a2) += (a3, a4)
  GV_LNOP_GEJ_ADD_GEJ,       // (a0, a1, a2) + (a3, a4, a5), GV_LNF_INF_A / _B
  GV_LNOP_GEJX_DOUBLE,
  GV_LNOP_GEJX_ADD_SCALED,   // (a0, a1, a2) += (a3, a4) scaled by a5
  GV_LNOP_SECP_END,
  // ed25519: k_debug_elane in ed_verify.hip
  GV_LNOP_ED_MUL = 128, GV_LNOP_ED_SQR, GV_LNOP_ED_SUB1, GV_LNOP_ED_NEG1, GV_LNOP_ED_SUB_NORM1,
  GV_LNOP_ED_SUB_NORM2, GV_LNOP_ED_SUB_NORM3, GV_LNOP_ED_ADD_NORM, GV_LNOP_ED_NORM, GV_LNOP_ED_TO_WORDS,
  GV_LNOP_ED_FROM_WORDS, GV_LNOP_ED_IS_ZERO, GV_LNOP_ED_IS_NEGATIVE, GV_LNOP_ED_INV, GV_LNOP_ED_POW22523,
  GV_LNOP_GE_DBL_T,          // ge_dbl_t<true> (a0, a1, a2; T is not read)
  GV_LNOP_GE_DBL_NT,         // ge_dbl_t<false>: slot 3 stays zero
  GV_LNOP_GE_ADD_CACHED,     // (a0..a3) + cached (a4..a7), GV_LNF_NEG
  GV_LNOP_GE_ADD_PRE,        // (a0..a3) + precomputed (a4, a5, a6), GV_LNF_NEG
  GV_LNOP_GE_TO_CACHED, GV_LNOP_GE_TO_PRE, GV_LNOP_GE_NEG,
  GV_LNOP_GE_FROMBYTES,      // words in; X, Y, Z, T out and the ok flag
  GV_LNOP_GE_TOBYTES,        // (a0, a1, a2) -> eight words
  GV_LNOP_GE_ADD_TAB,        // atab_build(a4..a7), then (a0..a3) +- entry e: GV_LNF_NEG, _NOT, entry bits
  GV_LNOP_SC_REDUCE512,      // 16 words in, 8 out
  GV_LNOP_SC_MINIMAL,        // 8 words in, flag
  GV_LNOP_ED_RADIX16,        // 8 words in (h < 2^253): the ladder's 64 signed digits
  GV_LNOP_ED_COMB4, GV_LNOP_ED_COMB6, GV_LNOP_ED_COMB8,   // ed_comb_digit<RB>: all windows' digits
  GV_LNOP_ED_END
};
