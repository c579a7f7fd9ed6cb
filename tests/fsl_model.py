"""Exact integer model of the limb-sliced field layers (csrc/secp_fsl.cuh,
csrc/ed_fsl.cuh) and of the group operations built on them (gjsl_* / gj4_* in
csrc/gv_lat.hip, gesl_* / ge4_* and the two decodes in csrc/ed_fsl.cuh and
csrc/ed_lat.hip) -- test infrastructure, no GPU.

A sliced value is a list of sixteen lane values (one 16-lane DPP row): limb i
of the 9 x 29 form in lane i.  fsl_cols, fsl_reduce and fsl_norm are
transcribed instruction by instruction: the row moves read 0 outside the row,
the per-lane constants are those of fsl_consts / efsl_consts, every (u32)
truncation and the 24-bit factors of __umul24 are where the device code has
them.  Every hardware width is asserted on the way (Width is raised when one
is crossed), so running an operation at the limb magnitudes a call site
declares proves that call site's bound:
  column sums and the column-16 product   < 2^64
  the F accumulator                       < 2^61 ((u32)(t >> 29) drops nothing)
  limb 8's accumulator                    < 2^53 (its carry is a __umul24 factor)
  every 32-bit limb sum                   < 2^32, no 32-bit difference below 0
The row-parallel rounds (gj4_*, ge4_*) are modelled as their four per-row
products; rows_all only moves values.

Curve.fault names ONE deliberate transcription error (FAULTS); the sharpness
tests show that the shared operand set tells each of them from the model.
"""
import random

from oracle import ed25519_ref as E

M29 = (1 << 29) - 1
NB = (1 << 29) + (1 << 17)          # N-form: every limb < NB
U32 = 1 << 32
LANES = 16

FAULTS = ("fold_const", "no_r3", "no_carry8", "k8_lane0", "no_col16", "h_shr1")


class Width(AssertionError):
    """a value left the width the hardware gives it"""


def _w(cond, what, *info):
    if not cond:
        raise Width((what,) + info)


class Curve:
    def __init__(self, name, p, k9, k8, k16, k17, k18, kc, bias, big8):
        self.name, self.p, self.fault = name, p, None
        lo = [1 if l <= 8 else 0 for l in range(LANES)]
        self.m29 = [M29 * x for x in lo]
        self.mw = [0xFFFFFFFF * x for x in lo]
        self.m29lo = [M29 if l < 8 else (0xFFFFFFFF if l == 8 else 0) for l in range(LANES)]
        full = lambda d: [d.get(l, 0) for l in range(LANES)]
        self.k9, self.k8, self.k16, self.k17, self.k18, self.kc = (full(d) for d in (k9, k8, k16, k17, k18, kc))
        self.bias, self.big8 = full(bias), full(big8)

    def with_fault(self, fault):
        """this curve with one deliberate error in the reduction (FAULTS)"""
        c = Curve.__new__(Curve)
        c.__dict__ = {k: (list(v) if isinstance(v, list) else v) for k, v in self.__dict__.items()}
        c.fault = fault
        if fault == "fold_const":
            c.k9[3] += 1
        if fault == "k8_lane0":
            c.k8[0] = 256
        assert fault in FAULTS
        return c


def _secp():
    lo9 = {l: 31264 for l in range(9)}
    bias = {l: 0x3ffffffe for l in range(9)}
    bias[0], bias[1] = 0x3fff0bc0, 0x3ffffdfe
    big8 = {l: 0x1fffffff0 for l in range(9)}
    big8[0], big8[1] = 0x1fff85e00, 0x1ffffeff0
    return Curve("secp256k1", 2**256 - 2**32 - 977, lo9, {l: 256 for l in range(1, 9)}, {7: 31264, 8: 256},
                 {0: 8003584, 1: 65536, 8: 31264}, {0: 440566784, 1: 16007169, 2: 65536}, {0: 31264, 1: 256},
                 bias, big8)


def _ed():
    bias = {l: 0x3ffffffe for l in range(9)}
    bias[0] = 0x3ffff680
    return Curve("ed25519", 2**255 - 19, {l: 1216 for l in range(9)}, {}, {7: 1216}, {8: 1216}, {0: 1478656},
                 {0: 1216}, bias, {l: b << 3 for l, b in bias.items()})


SECP = _secp()
ED = _ed()
N_SECP = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
ED_D = -121665 * pow(121666, ED.p - 2, ED.p) % ED.p
ED_SQRTM1 = pow(2, (ED.p - 1) // 4, ED.p)


# ------------------------------------------------------------------ lanes
def sl(limbs):
    """nine limbs -> a row (lanes 9..15 zero)"""
    assert len(limbs) == 9
    return list(limbs) + [0] * 7


def canon(v):
    """canonical limbs of an integer < 2^261"""
    assert 0 <= v < 1 << 261
    return sl([(v >> (29 * i)) & M29 for i in range(9)])


def val(x):
    return sum(v << (29 * i) for i, v in enumerate(x[:9]))


def shr(v, i):
    return [v[l - i] if l - i >= 0 else 0 for l in range(LANES)]


def shl(v, i):
    return [v[l + i] if l + i < LANES else 0 for l in range(LANES)]


def bc(v, i):
    return [v[i]] * LANES


def _u32(v, what):
    for x in v:
        _w(0 <= x < U32, what, x)
    return v


def vadd(*xs):
    return _u32([sum(t) for t in zip(*xs)], "32-bit sum")


def vsub(a, b):
    """a - b lane-wise, a the (already checked) minuend sum"""
    return _u32([x - y for x, y in zip(a, b)], "32-bit difference")


def vmulc(a, c):
    return _u32([x * c for x in a], "32-bit multiple")


def is_nform(x):
    return all(v < NB for v in x[:9]) and not any(x[9:])


# ------------------------------------------------------------- primitives
def fsl_cols(a, b, a2=None, b2=None, k=SECP):
    _u32(a, "operand")
    _u32(b, "operand")
    v = [sum(a[i] * b[l - i] for i in range(min(l, 8) + 1)) for l in range(LANES)]
    u = a[8] * b[8]
    if a2 is not None:
        _u32(a2, "operand")
        _u32(b2, "operand")
        v = [x + sum(a2[i] * b2[l - i] for i in range(min(l, 8) + 1)) for l, x in enumerate(v)]
        u += a2[8] * b2[8]
    for x in v:
        _w(x < 1 << 64, "column sum", x)
    _w(u < 1 << 64, "column 16", u)
    if k.fault == "no_col16":
        u = 0
    return v, [u] * LANES


def fsl_reduce(v, u, extra, k):
    # R1
    lo = [x & M29 for x in v]
    m = [(x >> 29) & M29 for x in v]
    h = [(x >> 58) & 0xFFFFFFFF for x in v]
    w = vadd(lo, shr(m, 1), shr(h, 1 if k.fault == "h_shr1" else 2))
    w16 = vadd([x & M29 for x in u], bc(m, 15), bc(h, 14))
    w17 = vadd([(x >> 29) & M29 for x in u], bc(h, 15))
    w18 = [(x >> 58) & 0xFFFFFFFF for x in u]
    # F
    for e in extra:
        _w(0 <= e < 1 << 64, "extra", e)
    w9, w8 = shl(w, 9), shl(w, 8)
    t = []
    for l in range(LANES):
        x = (w[l] & k.mw[l]) + extra[l] + w9[l] * k.k9[l] + w8[l] * k.k8[l] + w16[l] * k.k16[l] \
            + w17[l] * k.k17[l] + w18[l] * k.k18[l]
        _w(x < 1 << 61, "F accumulator", l, x)
        t.append(x)
    _w(t[8] < 1 << 53, "F accumulator of limb 8", t[8])
    # R2
    m2 = [(x >> 29) & 0xFFFFFFFF for x in t]
    x = vadd([(a & 0xFFFFFFFF) & b for a, b in zip(t, k.m29)], shr(m2, 1))
    return _fold_r3(x, k)


def _fold_r3(x, k):
    """the tail fsl_reduce and fsl_norm share: limb 8's carry (lane 9) into
    limbs 0 and 1 by __umul24, then one more carry step over limbs 0..7"""
    f = x[9]
    _w(f < 1 << 24, "__umul24 factor", f)
    if k.fault == "no_carry8":
        f = 0
    fold = [((f & 0xFFFFFF) * (c & 0xFFFFFF)) & 0xFFFFFFFF for c in k.kc]
    x = [a & b for a, b in zip(vadd(x, fold), k.mw)]
    if k.fault == "no_r3":
        return x
    c = [(a & ~b & 0xFFFFFFFF) >> 29 for a, b in zip(x, k.m29lo)]
    return vadd([a & b for a, b in zip(x, k.m29lo)], shr(c, 1))


ZERO = [0] * LANES


def fsl_mul(a, b, k):
    v, u = fsl_cols(a, b, k=k)
    return fsl_reduce(v, u, ZERO, k)


def fsl_sqr(a, k):
    return fsl_mul(a, a, k)


def fsl_mul_plus(a, b, extra, k):
    v, u = fsl_cols(a, b, k=k)
    return fsl_reduce(v, u, extra, k)


def fsl_mul2(a, b, c, d, k):
    v, u = fsl_cols(a, b, c, d, k=k)
    return fsl_reduce(v, u, ZERO, k)


def fsl_norm(x, k):
    _u32(x, "operand")
    c = [a >> 29 for a in x]
    x = vadd([a & b for a, b in zip(x, k.m29)], shr(c, 1))
    return _fold_r3(x, k)


def fsl_sub(a, b, k):
    return fsl_norm(vsub(vadd(a, k.bias), b), k)


def fsl_neg(b, k):
    return fsl_norm(vsub(k.bias, b), k)


def extra_big8_minus8(c, k):
    """k.big8 - ((u64)c << 3)"""
    return [x - (y << 3) for x, y in zip(k.big8, c)]


def extra_bias_minus(c, k):
    """(u64)(k.bias - c): a 32-bit difference, widened"""
    return vsub(k.bias, c)


def fsl_is_zero(a, k=SECP):
    """secp_fsl.cuh: the low-limb filter, then the canonical test"""
    _u32(a, "operand")
    z = a[0] & M29
    cand = z == 0 or z >= M29 + 1 - 977 * 256
    return cand and val(a) % k.p == 0


def efsl_is_zero(a, k=ED):
    _u32(a, "operand")
    return val(a) % k.p == 0


def to_words_value(a, k):
    """fsl_to_words / efsl_to_words: the canonical value (its 8 words)"""
    _u32(a, "operand")
    return val(a) % k.p


def fsl_from_words(value, k):
    """8 little-endian words -> limbs: secp keeps all 256 bits (limb 8 has
    24), ed25519 drops bit 255"""
    assert 0 <= value < 1 << 256
    if k.name == "ed25519":
        value &= (1 << 255) - 1
    return canon(value)


def fsl_sqr_n(a, n, k):
    for _ in range(n):
        a = fsl_sqr(a, k)
    return a


def fsl_sqrt_candidate(a, k=SECP):
    x2 = fsl_mul(fsl_sqr(a, k), a, k)
    x3 = fsl_mul(fsl_sqr(x2, k), a, k)
    x6 = fsl_mul(fsl_sqr_n(x3, 3, k), x3, k)
    x9 = fsl_mul(fsl_sqr_n(x6, 3, k), x3, k)
    x11 = fsl_mul(fsl_sqr_n(x9, 2, k), x2, k)
    x22 = fsl_mul(fsl_sqr_n(x11, 11, k), x11, k)
    x44 = fsl_mul(fsl_sqr_n(x22, 22, k), x22, k)
    x88 = fsl_mul(fsl_sqr_n(x44, 44, k), x44, k)
    x176 = fsl_mul(fsl_sqr_n(x88, 88, k), x88, k)
    x220 = fsl_mul(fsl_sqr_n(x176, 44, k), x44, k)
    x223 = fsl_mul(fsl_sqr_n(x220, 3, k), x3, k)
    t = fsl_mul(fsl_sqr_n(x223, 23, k), x22, k)
    t = fsl_mul(fsl_sqr_n(t, 6, k), x2, k)
    return fsl_sqr_n(t, 2, k)


def efsl_pow22523(z, k=ED):
    t0 = fsl_sqr(z, k)
    t1 = fsl_sqr_n(t0, 2, k)
    t1 = fsl_mul(z, t1, k)
    z11 = fsl_mul(t0, t1, k)
    t0 = fsl_sqr(z11, k)
    t0 = fsl_mul(t1, t0, k)
    t1 = fsl_sqr_n(t0, 5, k)
    t0 = fsl_mul(t1, t0, k)
    t1 = fsl_sqr_n(t0, 10, k)
    t1 = fsl_mul(t1, t0, k)
    t2 = fsl_sqr_n(t1, 20, k)
    t1 = fsl_mul(t2, t1, k)
    t1 = fsl_sqr_n(t1, 10, k)
    t0 = fsl_mul(t1, t0, k)
    t1 = fsl_sqr_n(t0, 50, k)
    t1 = fsl_mul(t1, t0, k)
    t2 = fsl_sqr_n(t1, 100, k)
    t1 = fsl_mul(t2, t1, k)
    t1 = fsl_sqr_n(t1, 50, k)
    t0 = fsl_mul(t1, t0, k)
    t0 = fsl_sqr_n(t0, 2, k)
    return fsl_mul(t0, z, k)


# ------------------------------------------------- secp256k1 group (one row)
def gjsl_double(a, k=SECP):
    x, y, z = a
    B = fsl_sqr(y, k)
    z3 = fsl_mul(y, vmulc(z, 2), k)
    E = fsl_mul(x, vmulc(x, 3), k)
    D = fsl_mul(x, B, k)
    C = fsl_mul(B, B, k)
    x3 = fsl_mul_plus(E, E, extra_big8_minus8(D, k), k)
    t = vsub(vadd(vmulc(D, 4), k.bias), x3)
    y3 = fsl_mul_plus(E, t, extra_big8_minus8(C, k), k)
    return (x3, y3, z3)


def _extra_x3(h3, v, k):
    """k.big8 - (u64)h3 - ((u64)v << 1)"""
    return [b - p - (q << 1) for b, p, q in zip(k.big8, h3, v)]


def gjsl_add_scaled(a, x, y, az, k=SECP):
    """-> (point, inf)"""
    ax, ay, azz = a
    z2 = fsl_sqr(az, k)
    h = fsl_mul_plus(x, z2, extra_bias_minus(ax, k), k)
    z3 = fsl_mul(z2, az, k)
    rr = fsl_mul_plus(y, z3, extra_bias_minus(ay, k), k)
    if fsl_is_zero(h, k):
        if fsl_is_zero(rr, k):
            return gjsl_double(a, k), False
        return a, True
    h2 = fsl_sqr(h, k)
    h3 = fsl_mul(h2, h, k)
    v = fsl_mul(ax, h2, k)
    nz = fsl_mul(azz, h, k)
    nx = fsl_mul_plus(rr, rr, _extra_x3(h3, v, k), k)
    t = vsub(vadd(v, k.bias), nx)
    ny = vsub(k.bias, ay)
    return (nx, fsl_mul2(rr, t, ny, h3, k), nz), False


def gjsl_add_gej(a, ainf, b, binf, k=SECP):
    if ainf or binf:
        return (b if ainf else a), (ainf and binf)
    z1z1, z2z2 = fsl_sqr(a[2], k), fsl_sqr(b[2], k)
    u1, u2 = fsl_mul(a[0], z2z2, k), fsl_mul(b[0], z1z1, k)
    s1 = fsl_mul(a[1], fsl_mul(b[2], z2z2, k), k)
    s2 = fsl_mul(b[1], fsl_mul(a[2], z1z1, k), k)
    h, rr = fsl_sub(u2, u1, k), fsl_sub(s2, s1, k)
    if fsl_is_zero(h, k):
        if fsl_is_zero(rr, k):
            return gjsl_double(a, k), False
        return a, True
    h2 = fsl_sqr(h, k)
    h3 = fsl_mul(h2, h, k)
    v = fsl_mul(u1, h2, k)
    oz = fsl_mul(fsl_mul(a[2], b[2], k), h, k)
    ox = fsl_mul_plus(rr, rr, _extra_x3(h3, v, k), k)
    t = vsub(vadd(v, k.bias), ox)
    return (ox, fsl_mul2(rr, t, vsub(k.bias, s1), h3, k), oz), False


# ------------------------------------------ secp256k1 group (row-parallel)
def gj4_double(A, k=SECP):
    x, y, z = A
    B, Z3, E = fsl_mul(y, y, k), fsl_mul(y, vmulc(z, 2), k), fsl_mul(x, vmulc(x, 3), k)
    D, C, E2 = fsl_mul(x, B, k), fsl_mul(B, B, k), fsl_mul(E, E, k)
    t = vsub(vadd(vmulc(fsl_norm(vmulc(D, 3), k), 4), k.bias), E2)
    x3 = fsl_mul_plus(E, E, extra_big8_minus8(D, k), k)
    y3 = fsl_mul_plus(E, t, extra_big8_minus8(C, k), k)
    return (x3, y3, Z3)


def _bias3(k):
    return vmulc(k.bias, 3)


def gj4_add(A, x, y, k=SECP):
    ax, ay, az = A
    z2 = fsl_sqr(az, k)
    h = fsl_mul_plus(x, z2, extra_bias_minus(ax, k), k)
    z3 = fsl_mul_plus(z2, az, ZERO, k)
    rr = fsl_mul_plus(y, z3, extra_bias_minus(ay, k), k)
    h2, zn, y1h = fsl_mul(h, h, k), fsl_mul(az, h, k), fsl_mul(ay, h, k)
    if fsl_is_zero(h, k):
        if fsl_is_zero(rr, k):
            return gj4_double(A, k), False
        return A, True
    h3, v, r2, y1h3 = fsl_mul(h2, h, k), fsl_mul(ax, h2, k), fsl_mul(rr, rr, k), fsl_mul(y1h, h2, k)
    x3 = fsl_norm(vsub(vsub(vadd(r2, _bias3(k)), h3), vmulc(v, 2)), k)
    y3 = fsl_mul_plus(rr, vsub(vadd(v, k.bias), x3), extra_bias_minus(y1h3, k), k)
    return (x3, y3, zn), False


def gj4_add_gej(A, inf, O, oinf, k=SECP):
    if inf or oinf:
        return (O if inf else A), (inf and oinf)
    z11, z22, z12 = fsl_mul(A[2], A[2], k), fsl_mul(O[2], O[2], k), fsl_mul(A[2], O[2], k)
    u1, u2, z23, z13 = fsl_mul(A[0], z22, k), fsl_mul(O[0], z11, k), fsl_mul(O[2], z22, k), fsl_mul(A[2], z11, k)
    h = fsl_sub(u2, u1, k)
    s1, s2, zn, h2 = fsl_mul(A[1], z23, k), fsl_mul(O[1], z13, k), fsl_mul(z12, h, k), fsl_mul(h, h, k)
    rr = fsl_sub(s2, s1, k)
    if fsl_is_zero(h, k):
        if fsl_is_zero(rr, k):
            return gj4_double(A, k), False
        return A, True
    r2, h3, v = fsl_mul(rr, rr, k), fsl_mul(h2, h, k), fsl_mul(u1, h2, k)
    x3 = fsl_norm(vsub(vsub(vadd(r2, _bias3(k)), h3), vmulc(v, 2)), k)
    y3 = fsl_mul2(rr, vsub(vadd(v, k.bias), x3), vsub(k.bias, s1), h3, k)
    return (x3, y3, zn), False


def gj4_add_affine(A, inf, x, y, k=SECP):
    if inf:
        return (x, fsl_norm(y, k), sl([1] + [0] * 8)), False
    return gj4_add(A, x, y, k)


# ------------------------------------------------------- edwards25519 group
def ed_small(v):
    return sl([v] + [0] * 8)


def _cached_tail(a, b, c, d, neg, k):
    x1 = fsl_norm(vsub(vadd(a, k.bias), b), k)
    y1 = vadd(a, b)
    dpc = vadd(d, c)
    dmc = fsl_norm(vsub(vadd(d, k.bias), c), k)
    z1, t1 = (dmc, dpc) if neg else (dpc, dmc)
    return (fsl_mul(x1, t1, k), fsl_mul(y1, z1, k), fsl_mul(z1, t1, k), fsl_mul(x1, y1, k))


def gesl_add_cached(P, ypx, ymx, z2, t2d, neg, k=ED):
    X, Y, Z, T = P
    qa, qb = (ymx, ypx) if neg else (ypx, ymx)
    a = fsl_mul(vadd(Y, X), qa, k)
    b = fsl_mul(vsub(vadd(Y, k.bias), X), qb, k)
    c = fsl_mul(t2d, T, k)
    d = fsl_mul(Z, z2, k)
    return _cached_tail(a, b, c, d, neg, k)


def gesl_add_pre(P, ypx, ymx, xy2d, neg, k=ED):
    X, Y, Z, T = P
    qa, qb = (ymx, ypx) if neg else (ypx, ymx)
    a = fsl_mul(vadd(Y, X), qa, k)
    b = fsl_mul(vsub(vadd(Y, k.bias), X), qb, k)
    c = fsl_mul(xy2d, T, k)
    return _cached_tail(a, b, c, vmulc(Z, 2), neg, k)


def gesl_add(P, Q, k=ED):
    ypx = vadd(Q[1], Q[0])
    ymx = fsl_norm(vsub(vadd(Q[1], k.bias), Q[0]), k)
    t2d = fsl_mul(Q[3], canon(2 * ED_D % k.p), k)
    return gesl_add_cached(P, ypx, ymx, vmulc(Q[2], 2), t2d, False, k)


def ge4_double(P, k=ED):
    X, Y, Z, _ = P
    a, bb, cz, sq = fsl_sqr(X, k), fsl_sqr(Y, k), fsl_sqr(Z, k), fsl_sqr(vadd(X, Y), k)
    b2 = vmulc(k.bias, 2)
    e = vsub(vsub(vadd(sq, b2), a), bb)
    g = vsub(vadd(bb, k.bias), a)
    h = fsl_norm(vsub(vsub(b2, a), bb), k)
    f = fsl_norm(vsub(vsub(vadd(bb, _bias3(k)), a), vmulc(cz, 2)), k)
    return (fsl_mul(e, f, k), fsl_mul(g, h, k), fsl_mul(g, f, k), fsl_mul(e, h, k))     # X, Y, Z, T


def ge4_add_cached(P, ypx, ymx, z2, t2d, pre, neg, k=ED):
    X, Y, Z, T = P
    qa, qb = (ymx, ypx) if neg else (ypx, ymx)
    a = fsl_mul(vadd(Y, X), qa, k)
    b = fsl_mul(vsub(vadd(Y, k.bias), X), qb, k)
    c = fsl_mul(t2d, T, k)
    d4 = fsl_mul(Z, z2, k)                                  # row 3's product runs for a precomputed q too
    return _cached_tail(a, b, c, vmulc(Z, 2) if pre else d4, neg, k)


def ge4_add(P, Q, k=ED):
    ypx = vadd(Q[1], Q[0])
    ymx = fsl_norm(vsub(vadd(Q[1], k.bias), Q[0]), k)
    t2d = fsl_mul(Q[3], canon(2 * ED_D % k.p), k)
    return ge4_add_cached(P, ypx, ymx, vmulc(Q[2], 2), t2d, False, False, k)


def efsl_decode(enc, strict, k=ED):
    """efsl_decode_strict / efsl_decode_lenient of a 256-bit encoding (int):
    -> (ok, x, y), x and y sliced"""
    sign = enc >> 255
    yv = enc & ((1 << 255) - 1)
    y = canon(yv)
    one = ed_small(1)
    yy = fsl_sqr(y, k)
    u = fsl_norm(vsub(vadd(yy, k.bias), one), k)
    v = fsl_norm(vadd(fsl_mul(yy, canon(ED_D), k), one), k)
    v3 = fsl_mul(fsl_sqr(v, k), v, k)
    t = fsl_mul(fsl_sqr(v3, k), v, k)
    t = efsl_pow22523(fsl_mul(t, u, k), k)
    x = fsl_mul(fsl_mul(t, v3, k), u, k)
    vxx = fsl_mul(fsl_sqr(x, k), v, k)
    root = efsl_is_zero(vsub(vadd(vxx, k.bias), u), k)
    neg_root = efsl_is_zero(vadd(vxx, u), k)
    if not root:
        x = fsl_mul(x, canon(ED_SQRTM1), k)
    xv = to_words_value(x, k)
    if (xv & 1) != sign:
        x = fsl_norm(vsub(k.bias, x), k)
    ok = root or neg_root
    if strict:
        ok = ok and yv < k.p and not (xv == 0 and sign)
    return ok, x, y


# ------------------------------------------------------------ operand sets
SECP_EDGE = [0, 1, 2, 977, 2**32, 2**32 + 977, SECP.p - 1, SECP.p, SECP.p + 1, 2**256 - 1, 2**256 - 2**32 - 978,
             2**255, 2**224 - 1, N_SECP, N_SECP - 1,
             0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE, (1 << 128) - 1]


def kp_limbs(kmul, p, bound, rng):
    """k p in redundant form: the canonical limbs (limb 8 takes every bit from
    2^232 up), then carries pushed back down at random while every limb stays
    below the bound; None when k p has no such representation"""
    v = kmul * p
    limbs = [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]
    for i in range(8, 0, -1):
        room = (bound - 1 - limbs[i - 1]) >> 29
        t = rng.randint(0, min(limbs[i], room)) if room > 0 else 0
        if limbs[i] >= bound:                              # must come down to fit at all
            t = max(t, min(room, limbs[i] - (bound - 1)))
        limbs[i] -= t
        limbs[i - 1] += t << 29
    if any(x >= bound for x in limbs):
        return None
    assert sum(x << (29 * i) for i, x in enumerate(limbs)) == v
    return limbs


def edge_limbs(bound, k, rng, kmax=33):
    """the edge representations of one operand whose limbs are below bound"""
    top = bound - 1
    out = [[top] * 9]
    for _ in range(3):
        v = [top] * 9
        v[rng.randrange(9)] = rng.randrange(bound)
        out.append(v)
    out += [[0] * 8 + [top], [top] + [0] * 8]
    out += [[top if i % 2 else 0 for i in range(9)], [0 if i % 2 else top for i in range(9)]]
    out += [[0] * 9, [1] + [0] * 8]
    for m in range(kmax + 1):
        for _ in range(2):
            r = kp_limbs(m, k.p, bound, rng)
            if r is not None:
                out.append(r)
    for e in SECP_EDGE:
        if e < 1 << 261 and all(x < bound for x in canon(e)[:9]):
            out.append(canon(e)[:9])
    return out


def operands(k, bounds, nrand, seed, kmax=33):
    """The operand tuples shared by the model tests and the device tests: one
    limb vector per entry of bounds (limbs in [0, bound)).  Every edge
    representation of every operand against the others' all-max form and three
    more of their edges, then nrand random tuples."""
    rng = random.Random(seed)
    edges = [edge_limbs(b, k, rng, kmax) for b in bounds]
    rnd = lambda b: [rng.randrange(b) for _ in range(9)]
    out = []
    for n, en in enumerate(edges):                          # every edge of operand n ...
        for i, e in enumerate(en):
            for step in (0, 1, 3, 7):                          # ... against four edges of every other operand
                t = [edges[m][0 if step == 0 else (step * i + m + 1) % len(edges[m])] for m in range(len(bounds))]
                t[n] = e
                out.append(tuple(t))
    out += [tuple(rnd(b) for b in bounds) for _ in range(nrand)]
    return out


def mul_operands(k):
    """the operand pairs of the product tests (model sharpness and device)"""
    return operands(k, [NB, NB], 2000, 11)


# ---------------------------------------- points, encodings, worst cases
def jac(pt, z):
    """affine secp256k1 point -> Jacobian with this Z, canonical limbs"""
    x, y = pt
    p = SECP.p
    return (canon(x * z * z % p), canon(y * z * z * z % p), canon(z))


def aff(P, inf=False):
    """Jacobian (sliced) -> affine, None for infinity"""
    if inf:
        return None
    x, y, z = (val(v) % SECP.p for v in P)
    zi = pow(z, SECP.p - 2, SECP.p)
    return (x * zi * zi % SECP.p, y * zi * zi * zi % SECP.p)


def ext(pt, z):
    """affine edwards25519 point -> extended coordinates with this Z"""
    x, y = pt
    p = ED.p
    return (canon(x * z % p), canon(y * z % p), canon(z), canon(x * y % p * z % p))


def ed_aff(P):
    """extended (sliced) -> affine; T Z == X Y is part of the check"""
    X, Y, Z, T = (val(v) % ED.p for v in P)
    zi = pow(Z, ED.p - 2, ED.p)
    assert T * Z % ED.p == X * Y % ED.p
    return (X * zi % ED.p, Y * zi % ED.p)


def cached(Q):
    """extended -> cached form (Y+X, Y-X, 2Z, 2dT)"""
    X, Y, Z, T = (val(v) % ED.p for v in Q)
    return (canon((Y + X) % ED.p), canon((Y - X) % ED.p), canon(2 * Z % ED.p), canon(2 * ED_D * T % ED.p))


def ed_points(rng):
    """the eight small-order points, the identity, B and three random multiples"""
    pts = list(E.small_order_points()) + [E.IDENT, E.B]
    pts += [E.point_mul(rng.randrange(1, E.L), E.B) for _ in range(3)]
    return pts


def decode_encodings():
    """the encodings of test_ed_host.py::test_frombytes_matches_oracle"""
    rng = random.Random(6)
    P = ED.p
    encs = [E.encode_point(p) for p in E.small_order_points()]
    encs += [((y + P) | (s << 255)).to_bytes(32, "little") for y in range(19) for s in (0, 1)]
    encs += [(1 | (1 << 255)).to_bytes(32, "little"), ((P - 1) | (1 << 255)).to_bytes(32, "little")]
    encs += [rng.randbytes(32) for _ in range(60)]
    encs += [E.keypair(rng.randbytes(32))[2] for _ in range(20)]
    return encs


def worst(bound_of_lane, rng, nrand=200):
    """all limbs at their bound - 1, one limb lowered (every position), random"""
    top = [bound_of_lane(l) - 1 for l in range(9)]
    out = [top]
    for i in range(9):
        v = list(top)
        v[i] = rng.randrange(top[i] + 1)
        out.append(v)
        v = list(top)
        v[i] = 0
        out.append(v)
    out += [[rng.randrange(t + 1) for t in top] for _ in range(nrand)]
    return [sl(v) for v in out]


def mag(n, k=None, bias=False):
    """per-lane bound of n N-form values (+ BIAS)"""
    return lambda l: n * (NB - 1) + (k.bias[l] if bias else 0) + 1
