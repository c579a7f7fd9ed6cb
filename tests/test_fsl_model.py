"""The integer model of the limb-sliced layers (tests/fsl_model.py) on the CPU:
  correctness  its results are the true values mod p, on both curves;
  contracts    every primitive at each limb magnitude a call site declares, and
               every composite with all inputs at worst-case N-form limbs,
               stays inside every hardware width and returns N-form;
  sharpness    single-fault mutants of the reduction each change a result on
               the operand set the device tests (test_sliced_gpu.py) share.
"""
import random
import zlib

import pytest

import fsl_model as F
from fsl_model import ED, NB, SECP, sl, val
from oracle import ed25519_ref as E
from oracle import secp_ref as R

CURVES = [SECP, ED]
IDS = ["secp256k1", "ed25519"]
TOP = NB - 1
Y2 = int(2 ** 30.1)                 # an affine y or its negation BIAS - y (secp_fsl.cuh: "y < 2^30.1")
B316 = int(2 ** 31.6)               # gj4_double: 12 D - E^2 "< 2^31.6"


# ----------------------------------------------------------- correctness
@pytest.mark.parametrize("k", CURVES, ids=IDS)
def test_products_and_sums_are_the_values_mod_p(k):
    p = k.p
    for a, b, c, d in F.operands(k, [NB, NB, NB, NB], 300, 1):
        A, B, C, D = sl(a), sl(b), sl(c), sl(d)
        va, vb, vc, vd = val(A), val(B), val(C), val(D)
        for got, want in (
            (F.fsl_mul(A, B, k), va * vb),
            (F.fsl_sqr(A, k), va * va),
            (F.fsl_mul_plus(A, B, F.extra_big8_minus8(C, k), k), va * vb - 8 * vc),
            (F.fsl_mul_plus(A, B, F.extra_bias_minus(C, k), k), va * vb - vc),
            (F.fsl_mul2(A, B, C, D, k), va * vb + vc * vd),
            (F.fsl_sub(A, B, k), va - vb),
            (F.fsl_neg(A, k), -va),
            (F.fsl_norm(F.vadd(A, B, C, D), k), va + vb + vc + vd),
        ):
            assert val(got) % p == want % p and F.is_nform(got)


@pytest.mark.parametrize("k", CURVES, ids=IDS)
def test_norm_and_is_zero_on_limbs_below_2_32(k):
    is_zero = F.fsl_is_zero if k is SECP else F.efsl_is_zero
    ops = F.operands(k, [1 << 32], 500, 2, kmax=256)
    zeros = 0
    for (a,) in ops:
        A = sl(a)
        r = F.fsl_norm(A, k)
        assert val(r) % k.p == val(A) % k.p and F.is_nform(r)
        assert is_zero(A, k) == (val(A) % k.p == 0)
        zeros += val(A) % k.p == 0
    assert zeros >= 257                                      # every k p, k = 0..256, is in the set


def test_power_chains():
    rng = random.Random(3)
    for x in [0, 1, 2, SECP.p - 1] + [rng.randrange(SECP.p) for _ in range(12)]:
        assert val(F.fsl_sqrt_candidate(F.canon(x), SECP)) % SECP.p == pow(x, (SECP.p + 1) // 4, SECP.p)
    for x in [0, 1, 2, ED.p - 1] + [rng.randrange(ED.p) for _ in range(12)]:
        assert val(F.efsl_pow22523(F.canon(x), ED)) % ED.p == pow(x, (ED.p - 5) // 8, ED.p)


def test_secp_group_ops_are_the_group_law():
    rng = random.Random(4)
    ks = [1, 2, 3, R.N - 1, R.LAMBDA, rng.randrange(1, R.N), rng.randrange(1, R.N)]
    pts = [R.point_mul(s, R.G) for s in ks]
    for P in pts:
        z1 = rng.randrange(1, SECP.p)
        A = F.jac(P, z1)
        assert F.aff(F.gjsl_double(A)) == F.aff(F.gj4_double(A)) == R.point_add(P, P)
        for Q in pts + [R.point_neg(P)]:
            want = R.point_add(P, Q)
            z2 = rng.randrange(1, SECP.p)
            Bj = F.jac(Q, z2)
            for fn in (F.gjsl_add_gej, F.gj4_add_gej):
                r, inf = fn(A, False, Bj, False)
                assert F.aff(r, inf) == want
                assert F.aff(*fn(A, True, Bj, False)) == Q and F.aff(*fn(A, False, Bj, True)) == P
                assert fn(A, True, Bj, True)[1]
            # Q scaled onto A's curve: (x az^2, y az^3) is what the kernels add
            qx, qy = F.canon(Q[0]), F.canon(Q[1])
            r, inf = F.gjsl_add_scaled(A, qx, qy, A[2])
            assert F.aff(r, inf) == want
            r, inf = F.gj4_add(A, qx, qy)
            assert F.aff(r, inf) == want
            r, inf = F.gj4_add_affine(A, False, qx, F.vsub(SECP.bias, qy))     # the negated entry, raw
            assert F.aff(r, inf) == R.point_add(P, R.point_neg(Q))
            assert F.aff(*F.gj4_add_affine(A, True, qx, qy)) == Q


def test_ed_group_ops_are_the_group_law():
    rng = random.Random(5)
    pts = F.ed_points(rng)
    for P in pts:
        Pe = F.ext(P, rng.randrange(1, ED.p))
        assert F.ed_aff(F.ge4_double(Pe)) == E.point_add(P, P)
        for Q in pts + [E.point_neg(P), P]:
            Qe = F.ext(Q, rng.randrange(1, ED.p))
            want = {False: E.point_add(P, Q), True: E.point_add(P, E.point_neg(Q))}
            assert F.ed_aff(F.gesl_add(Pe, Qe)) == F.ed_aff(F.ge4_add(Pe, Qe)) == want[False]
            c = F.cached(Qe)
            x, y = Q
            pre = (F.canon((y + x) % ED.p), F.canon((y - x) % ED.p), F.canon(2 * F.ED_D * x * y % ED.p))
            for neg in (False, True):
                assert F.ed_aff(F.gesl_add_cached(Pe, *c, neg)) == want[neg]
                assert F.ed_aff(F.ge4_add_cached(Pe, *c, False, neg)) == want[neg]
                assert F.ed_aff(F.gesl_add_pre(Pe, *pre, neg)) == want[neg]
                assert F.ed_aff(F.ge4_add_cached(Pe, pre[0], pre[1], F.ZERO, pre[2], True, neg)) == want[neg]


def test_decodes_match_the_oracle():
    for enc in F.decode_encodings():
        e = int.from_bytes(enc, "little")
        want = E.decode_point(enc)
        ok, x, y = F.efsl_decode(e, False)
        assert ok == (want is not None), enc.hex()
        if want is not None:
            assert (val(x) % ED.p, val(y) % ED.p) == (want[0], want[1] % ED.p), enc.hex()
        sok, sx, sy = F.efsl_decode(e, True)
        yv, sign = e & ((1 << 255) - 1), e >> 255
        strict_ok = want is not None and yv < ED.p and not (want[0] == 0 and sign)
        assert sok == strict_ok, enc.hex()
        if sok:
            assert (val(sx) % ED.p, val(sy)) == (want[0], want[1]) and E.encode_point(want) == enc


# ------------------------------------------------------------- contracts
def pairs(wa, wb):
    n = max(len(wa), len(wb))
    return [(wa[0], wb[0])] + [(wa[i % len(wa)], wb[0]) for i in range(n)] + [(wa[0], wb[i % len(wb)]) for i in range(n)] \
        + [(wa[i % len(wa)], wb[(7 * i + 3) % len(wb)]) for i in range(n)]


@pytest.mark.parametrize("k", CURVES, ids=IDS)
@pytest.mark.parametrize("name", ["NxN", "Nx2N", "Nx3N", "2Nx2N", "2Nx3N", "(N+BIAS)x2N", "Nx(4N+BIAS)", "Nx2^31.6"])
def test_product_contracts(k, name):
    rng = random.Random(zlib.crc32(name.encode()))
    bounds = {
        "NxN": (F.mag(1), F.mag(1)), "Nx2N": (F.mag(1), F.mag(2)), "Nx3N": (F.mag(1), F.mag(3)), "2Nx2N": (F.mag(2), F.mag(2)),
        "2Nx3N": (F.mag(2), F.mag(3)), "(N+BIAS)x2N": (F.mag(1, k, True), F.mag(2)), "Nx(4N+BIAS)": (F.mag(1), F.mag(4, k, True)),
        "Nx2^31.6": (F.mag(1), lambda l: B316),
    }[name]
    wa, wb = F.worst(bounds[0], rng), F.worst(bounds[1], rng)
    wc = F.worst(F.mag(1), rng)
    for i, (a, b) in enumerate(pairs(wa, wb)):
        c = wc[i % len(wc)]
        for r in (F.fsl_mul(a, b, k), F.fsl_mul(b, a, k),
                  F.fsl_mul_plus(a, b, F.extra_big8_minus8(c, k), k),
                  F.fsl_mul_plus(a, b, F.extra_bias_minus(c, k), k)):
            assert F.is_nform(r)
        assert val(F.fsl_mul(a, b, k)) % k.p == val(a) * val(b) % k.p


@pytest.mark.parametrize("k", CURVES, ids=IDS)
def test_mul2_contract(k):
    """fsl_mul2 at N x (N + BIAS) + BIAS x N (gjsl_add_scaled: R (V - X3) - Y1 H^3)"""
    rng = random.Random(22)
    wa, wb = F.worst(F.mag(1), rng), F.worst(F.mag(1, k, True), rng)
    wc, wd = F.worst(F.mag(0, k, True), rng), F.worst(F.mag(1), rng)
    for i, (a, b) in enumerate(pairs(wa, wb)):
        c, d = wc[(3 * i) % len(wc)], wd[(5 * i) % len(wd)]
        r = F.fsl_mul2(a, b, c, d, k)
        assert F.is_nform(r) and val(r) % k.p == (val(a) * val(b) + val(c) * val(d)) % k.p


@pytest.mark.parametrize("k", CURVES, ids=IDS)
def test_the_width_assertions_fire_past_the_bound(k):
    a = sl([3 * TOP] * 9)
    with pytest.raises(F.Width):
        F.fsl_mul(a, a, k)                                   # 3N x 3N: nine products of 2^61.2
    with pytest.raises(F.Width):
        F.fsl_norm(sl([1 << 32] + [0] * 8), k)
    with pytest.raises(F.Width):
        F.fsl_sub(sl([0] * 9), sl([1 << 31] * 9), k)         # b above BIAS: the difference wraps


def test_power_chains_from_worst_case_inputs():
    """every square and product of the two chains from an all-max N-form element"""
    top = sl([TOP] * 9)
    r = F.fsl_sqrt_candidate(top, SECP)
    assert F.is_nform(r) and val(r) % SECP.p == pow(val(top), (SECP.p + 1) // 4, SECP.p)
    r = F.efsl_pow22523(top, ED)
    assert F.is_nform(r) and val(r) % ED.p == pow(val(top), (ED.p - 5) // 8, ED.p)


def nform_worst(rng, n):
    return F.worst(F.mag(1), rng, n)


def test_secp_composites_at_worst_case_inputs():
    rng = random.Random(31)
    w = nform_worst(rng, 40)
    wy = F.worst(lambda l: Y2, rng, 40)
    n = len(w)
    for i in range(n):
        g = lambda s: w[0] if i == 0 else w[(s * i + s) % n]
        A, B = (g(1), g(2), g(3)), (g(4), g(5), g(6))
        x, y, az = g(7), wy[0] if i == 0 else wy[(3 * i) % len(wy)], g(8)
        outs = [F.gjsl_double(A), F.gj4_double(A), F.gjsl_add_scaled(A, x, y, az)[0], F.gjsl_add_gej(A, False, B, False)[0],
                F.gj4_add(A, x, y)[0], F.gj4_add_gej(A, False, B, False)[0], F.gj4_add_affine(A, False, x, y)[0],
                F.gj4_add_affine(A, True, x, y)[0]]
        for P in outs:
            assert all(F.is_nform(v) for v in P)
        # the two schedules compute the same point (projectively the same Jacobian triple)
        for P, Q in ((outs[0], outs[1]), (outs[3], outs[5])):
            assert [val(v) % SECP.p for v in P] == [val(v) % SECP.p for v in Q]


def test_ed_composites_at_worst_case_inputs():
    rng = random.Random(32)
    w = nform_worst(rng, 40)
    w2 = F.worst(F.mag(2), rng, 40)
    n = len(w)
    for i in range(n):
        g = lambda s: w[0] if i == 0 else w[(s * i + s) % n]
        g2 = lambda s: w2[0] if i == 0 else w2[(s * i + s) % len(w2)]
        P, Q = (g(1), g(2), g(3), g(4)), (g(5), g(6), g(7), g(8))
        for neg in (False, True):
            outs = [F.gesl_add_cached(P, g2(1), g2(2), g2(3), g(9), neg), F.gesl_add_pre(P, g2(1), g2(2), g(9), neg),
                    F.ge4_add_cached(P, g2(1), g2(2), g2(3), g(9), False, neg),
                    F.ge4_add_cached(P, g2(1), g2(2), F.ZERO, g(9), True, neg)]
            assert [[val(v) % ED.p for v in o] for o in outs[:2]] == [[val(v) % ED.p for v in o] for o in outs[2:]]
            for o in outs:
                assert all(F.is_nform(v) for v in o)
        for o in (F.gesl_add(P, Q), F.ge4_add(P, Q), F.ge4_double(P)):
            assert all(F.is_nform(v) for v in o)


# ------------------------------------------------------------- sharpness
@pytest.mark.parametrize("k", CURVES, ids=IDS)
@pytest.mark.parametrize("fault", F.FAULTS)
def test_operand_set_tells_each_mutant_from_the_model(k, fault):
    """A device that had this single fault would fail test_sliced_gpu.py's
    bit-for-bit comparison on at least one operand pair of the shared set."""
    bad = k.with_fault(fault)
    for a, b in F.mul_operands(k):
        A, B = sl(a), sl(b)
        try:
            if F.fsl_mul(A, B, bad) != F.fsl_mul(A, B, k):
                return
        except F.Width:
            pass                                             # the fault left a width: not counted as told apart
    pytest.fail("no operand pair tells this mutant from the model")
