"""The limb-sliced field and group layers on the device (gv_debug_sl_op:
k_debug_sl in csrc/gv_lat.hip, k_debug_esl in csrc/ed_lat.hip), one operation
per 64-lane wave with the operands replicated in its four rows, at the
operand bounds their call sites declare.

Every comparison is exact.  The device limbs must equal those of the integer
model (tests/fsl_model.py, which asserts every hardware width) bit for bit in
all sixteen lanes, the values must be the true ones mod p (pow, the oracles'
group laws), outputs must be N-form with lanes 9..15 zero, and the four rows
must agree.  The operand set is fsl_model.operands -- the set whose sharpness
tests/test_fsl_model.py proves against single-fault mutants.
"""
import random

import numpy as np
import pytest

import fsl_model as F
import gpuverify as gvm
from fsl_model import ED, NB, SECP, aff, cached, decode_encodings, ed_aff, ed_points, ext, jac, mag, sl, val, worst
from oracle import ed25519_ref as E
from oracle import secp_ref as R

pytestmark = pytest.mark.gpu
CURVES = [SECP, ED]
IDS = ["secp256k1", "ed25519"]


@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    yield v
    v.close()


def pre(k, name):
    """the op of this name with curve k's constants"""
    if k is SECP:
        return name
    return {"sub": "ed_sub"}.get(name, "ed_" + name)


def pack(items, flags=0, words=False):
    """items: tuples of 9-limb operands (or, words=True, one integer of up to
    512 bits) -> the n x SL_IN input of gv_debug_sl_op"""
    w = np.zeros((len(items), gvm.SL_IN), np.uint32)
    for i, it in enumerate(items):
        if words:
            w[i, :16] = [(it >> (32 * j)) & 0xFFFFFFFF for j in range(16)]
        else:
            for j, limbs in enumerate(it):
                w[i, 9 * j:9 * j + 9] = limbs[:9]
    fl = np.asarray(flags, np.uint32) | np.uint32(gvm.SLF_WORDS if words else 0)
    w[:, gvm.SL_IN - 1] = fl
    return w


def run(ver, op, items, flags=0, words=False):
    out = ver.debug_sl_op(op, pack(items, flags, words))
    assert (out[:, 64 + gvm.SLS_KNOWN] == 1).all(), op
    assert (out[:, 64 + gvm.SLS_ROWS] == 1).all(), (op, "the four rows disagree", np.nonzero(out[:, 66] != 1)[0][:5])
    return out


def slot(out, i, s):
    return [int(x) for x in out[i, 16 * s:16 * s + 16]]


def check_nform(row, what):
    assert all(x < NB for x in row[:9]) and not any(row[9:]), what


def rows(it):
    return [sl(list(x)[:9]) for x in it]


def test_unknown_ops_and_mismatched_flags_are_refused(ver):
    one = [([1] + [0] * 8,) * 2]
    for code in (-1, gvm.SLOP["modinv"] + 1, 63, gvm.SLOP["ed_digits"] + 1):
        with pytest.raises(gvm.GpuVerifyError):
            ver.debug_sl_op(code, pack(one))
    for op in ("mul", "ed_mul"):                             # limb ops do not take words, word ops need the bit
        assert ver.debug_sl_op(op, pack(one, gvm.SLF_WORDS))[0, 64 + gvm.SLS_KNOWN] == 0
        assert slot(run(ver, op, one), 0, 0) == sl([1] + [0] * 8)
    for op in ("from_words", "modinv", "ed_from_words", "ed_digits"):
        assert ver.debug_sl_op(op, pack(one))[0, 64 + gvm.SLS_KNOWN] == 0


# --------------------------------------------------------------- primitives
def prim_cases(k):
    b = min(k.bias[:9])
    return {
        "mul": ([NB, NB], lambda a, b_: F.fsl_mul(a, b_, k), lambda a, b_: a * b_),
        "sqr": ([NB], lambda a: F.fsl_sqr(a, k), lambda a: a * a),
        "norm": ([1 << 32], lambda a: F.fsl_norm(a, k), lambda a: a),
        "sub": ([(1 << 32) - max(k.bias), b + 1], lambda a, b_: F.fsl_sub(a, b_, k), lambda a, b_: a - b_),
    }


SECP_ONLY = {
    "mul_plus8": ([NB, NB, NB], lambda a, b, c: F.fsl_mul_plus(a, b, F.extra_big8_minus8(c, SECP), SECP),
                  lambda a, b, c: a * b - 8 * c),
    "mul_plusb": ([NB, NB, NB], lambda a, b, c: F.fsl_mul_plus(a, b, F.extra_bias_minus(c, SECP), SECP),
                  lambda a, b, c: a * b - c),
    # N x (N + BIAS) + BIAS x N, as gjsl_add_scaled calls it
    "mul2": ([NB, NB + min(SECP.bias[:9]), min(SECP.bias[:9]) + 1, NB], lambda a, b, c, d: F.fsl_mul2(a, b, c, d, SECP),
             lambda a, b, c, d: a * b + c * d),
    "neg": ([min(SECP.bias[:9]) + 1], lambda a: F.fsl_neg(a, SECP), lambda a: -a),
}


def prim_params():
    out = []
    for k, kid in zip(CURVES, IDS):
        for name in ("mul", "sqr", "norm", "sub"):
            out.append(pytest.param(k, name, id=f"{kid}-{name}"))
    out += [pytest.param(SECP, name, id=f"secp256k1-{name}") for name in SECP_ONLY]
    return out


@pytest.mark.parametrize("k,name", prim_params())
def test_primitive_matches_the_model_bit_for_bit(ver, k, name):
    bounds, model, true = (prim_cases(k)[name] if name in prim_cases(k) else SECP_ONLY[name])
    kmax = 256 if name == "norm" else 33
    items = F.mul_operands(k) if name == "mul" else F.operands(k, bounds, 2000, 40 + len(name), kmax)
    out = run(ver, pre(k, name), items)
    for i, it in enumerate(items):
        got = slot(out, i, 0)
        ops = rows(it)
        assert got == model(*ops), (name, it)
        assert val(got) % k.p == true(*[val(o) for o in ops]) % k.p, (name, it)
        check_nform(got, (name, it))


@pytest.mark.parametrize("k", CURVES, ids=IDS)
def test_is_zero_exactly_on_the_multiples_of_p(ver, k):
    items = F.operands(k, [1 << 32], 2000, 50, kmax=256)
    items += F.operands(k, [NB], 200, 51)
    out = run(ver, pre(k, "is_zero"), items)
    zeros = 0
    for i, (a,) in enumerate(items):
        want = val(sl(a)) % k.p == 0
        zeros += want
        assert bool(out[i, 64 + gvm.SLS_FLAG]) == want, a
    assert zeros >= 257 + 30


@pytest.mark.parametrize("k", CURVES, ids=IDS)
def test_words_in_and_out(ver, k):
    rng = random.Random(60)
    vals = F.SECP_EDGE + [ED.p - 1, ED.p, ED.p + 1, 2**255 - 1, 2**255 + 5] + [rng.randrange(2**256) for _ in range(2000)]
    for op in (["from_words", "load_words"] if k is SECP else ["from_words"]):
        out = run(ver, pre(k, op), vals, words=True)
        for i, v in enumerate(vals):
            assert slot(out, i, 0) == F.fsl_from_words(v, k), (op, hex(v))
    items = F.operands(k, [7 * NB], 2000, 61)
    out = run(ver, pre(k, "to_words"), items)
    for i, (a,) in enumerate(items):
        got = slot(out, i, 0)
        assert sum(x << (32 * j) for j, x in enumerate(got[:8])) == val(sl(a)) % k.p and not any(got[8:]), a


def test_rows_all_moves_four_distinct_rows(ver):
    rng = random.Random(70)
    items = [tuple([rng.randrange(1 << 32) for _ in range(9)] for _ in range(4)) for _ in range(200)]
    out = run(ver, "rows_all", items)
    for i, it in enumerate(items):
        for s in range(4):
            assert slot(out, i, s) == sl(it[s])


def test_modinv_sl(ver):
    rng = random.Random(80)
    N = R.N
    xs = [1, 2, N - 1, N - 2, (N - 1) // 2, 2**255, 2**128 + 1] + [rng.randrange(1, N) for _ in range(4000)]
    out = run(ver, "modinv", xs + [0], words=True)
    for i, x in enumerate(xs):
        got = slot(out, i, 0)
        assert sum(v << (32 * j) for j, v in enumerate(got[:8])) == pow(x, -1, N), hex(x)
    assert not any(slot(out, len(xs), 0))


def test_power_chains(ver):
    rng = random.Random(90)
    for k, op, e in ((SECP, "sqrt", (SECP.p + 1) // 4), (ED, "ed_pow22523", (ED.p - 5) // 8)):
        edge = [v for (v,) in F.operands(k, [NB], 0, 91)]
        xs = edge + [F.canon(rng.randrange(k.p))[:9] for _ in range(500)]
        out = run(ver, op, [(x,) for x in xs])
        model = F.fsl_sqrt_candidate if k is SECP else F.efsl_pow22523
        for i, x in enumerate(xs):
            got = slot(out, i, 0)
            assert val(got) % k.p == pow(val(sl(x)), e, k.p), (op, x)
            check_nform(got, (op, x))
            if i % 25 == 0:
                assert got == model(sl(x), k), (op, x)


# --------------------------------------------------------- secp256k1 group
def secp_points():
    rng = random.Random(100)
    ks = [1, 2, 3, R.N - 1, R.LAMBDA] + [rng.randrange(1, R.N) for _ in range(5)]
    return rng, [R.point_mul(s, R.G) for s in ks]


def worst_rows(n, seed, bound=None):
    rng = random.Random(seed)
    w = worst(bound or mag(1), rng, 20)
    return [[w[0] if i == 0 else w[(s * i + s) % len(w)] for s in range(1, n + 1)] for i in range(len(w))]


def point_out(out, i, n=3):
    return tuple(slot(out, i, s) for s in range(n))


def test_secp_doubling(ver):
    rng, pts = secp_points()
    items = [jac(P, rng.randrange(1, SECP.p)) for P in pts for _ in range(3)]
    want = [R.point_add(P, P) for P in pts for _ in range(3)]
    extra = [tuple(r) for r in worst_rows(3, 101)]
    o1, o4 = run(ver, "gjsl_double", items + extra), run(ver, "gj4_double", items + extra)
    for i, A in enumerate(items + extra):
        g1, g4 = point_out(o1, i), point_out(o4, i)
        assert g1 == F.gjsl_double(A) and g4 == F.gj4_double(A)
        assert [val(v) % SECP.p for v in g1] == [val(v) % SECP.p for v in g4]
        for v in g1 + g4:
            check_nform(v, A)
        if i < len(items):
            assert aff(g1) == aff(g4) == want[i]


def test_secp_additions_and_their_exceptional_cases(ver):
    rng, pts = secp_points()
    cases = []                                               # (A jacobian, P, Q)
    for P in pts:
        for Q in pts[:6] + [P, R.point_neg(P)]:              # general, Q = P (doubling), Q = -P (infinity)
            cases.append((jac(P, rng.randrange(1, SECP.p)), P, Q))
    # Jacobian + Jacobian, with every combination of infinite inputs
    items, flags, want = [], [], []
    for A, P, Q in cases:
        Bj = jac(Q, rng.randrange(1, SECP.p))
        for fl, w in ((0, R.point_add(P, Q)), (gvm.SLF_INF_A, Q), (gvm.SLF_INF_B, P), (gvm.SLF_INF_A | gvm.SLF_INF_B, None)):
            items.append(A + Bj)
            flags.append(fl)
            want.append(w)
    nw = len(items)
    items += [tuple(r) for r in worst_rows(6, 102)]
    flags += [0] * (len(items) - nw)
    o1, o4 = run(ver, "gjsl_add_gej", items, flags), run(ver, "gj4_add_gej", items, flags)
    for i, it in enumerate(items):
        A, Bj = tuple(rows(it[:3])), tuple(rows(it[3:]))
        ai, bi = bool(flags[i] & gvm.SLF_INF_A), bool(flags[i] & gvm.SLF_INF_B)
        m1, m4 = F.gjsl_add_gej(A, ai, Bj, bi), F.gj4_add_gej(A, ai, Bj, bi)
        for o, m in ((o1, m1), (o4, m4)):
            inf = bool(o[i, 64 + gvm.SLS_INF])
            assert inf == m[1]
            if not inf:
                assert point_out(o, i) == m[0]
            if i < nw:
                assert aff(point_out(o, i), inf) == want[i]
        if not m1[1]:
            assert [val(v) % SECP.p for v in point_out(o1, i)] == [val(v) % SECP.p for v in point_out(o4, i)]
    # Jacobian + affine on the accumulator's curve (az = a.z, as the kernels call it; the gj4 rounds
    # always scale by a.z, so operand 5 is gjsl_add_scaled's alone)
    items, want = [], []
    for A, P, Q in cases:
        for neg in (False, True):
            qy = F.canon(Q[1])[:9]
            y = [b - v for b, v in zip(SECP.bias[:9], qy)] if neg else qy     # the negated entry stays raw
            items.append(A + (F.canon(Q[0])[:9], y, A[2][:9]))
            want.append(R.point_add(P, R.point_neg(Q) if neg else Q))
    nw = len(items)
    items += [tuple(r) for r in worst_rows(6, 103)]
    os_ = {op: run(ver, op, items) for op in ("gjsl_add_scaled", "gj4_add", "gj4_add_affine")}
    for i, it in enumerate(items):
        r = rows(it)
        A = tuple(r[:3])
        models = {"gjsl_add_scaled": F.gjsl_add_scaled(A, r[3], r[4], r[5]), "gj4_add": F.gj4_add(A, r[3], r[4]),
                  "gj4_add_affine": F.gj4_add_affine(A, False, r[3], r[4])}
        for op, m in models.items():
            o = os_[op]
            inf = bool(o[i, 64 + gvm.SLS_INF])
            assert inf == m[1], (op, i)
            if not inf:
                assert point_out(o, i) == m[0], (op, i)
                for v in point_out(o, i):
                    check_nform(v, (op, i))
            if i < nw:
                assert aff(point_out(o, i), inf) == want[i], (op, i)
        if i < nw and not models["gjsl_add_scaled"][1]:      # az = a.z: the same point in the same coordinates
            ref = [val(v) % SECP.p for v in point_out(os_["gjsl_add_scaled"], i)]
            for op in ("gj4_add", "gj4_add_affine"):
                assert [val(v) % SECP.p for v in point_out(os_[op], i)] == ref, (op, i)
    # onto infinity: the affine point itself
    items = [(A[0][:9], A[1][:9], A[2][:9], F.canon(Q[0])[:9], F.canon(Q[1])[:9]) for A, _, Q in cases[:12]]
    o = run(ver, "gj4_add_affine", items, gvm.SLF_INF_A)
    for i, (_, _, Q) in enumerate(cases[:12]):
        assert not o[i, 64 + gvm.SLS_INF] and aff(point_out(o, i)) == Q


# ------------------------------------------------------------ edwards25519
def test_ed_group_ops(ver):
    rng = random.Random(110)
    pts = ed_points(rng)
    pairs = [(P, Q) for P in pts for Q in pts[:4] + [E.IDENT, E.B, P, E.point_neg(P)]]
    PQ = [(ext(P, rng.randrange(1, ED.p)), ext(Q, rng.randrange(1, ED.p))) for P, Q in pairs]
    lim = lambda t: tuple(v[:9] for v in t)
    # doubling
    items = [lim(Pe) for Pe, _ in PQ] + [tuple(r) for r in worst_rows(4, 111)]
    o = run(ver, "ge4_double", items)
    for i, it in enumerate(items):
        got = point_out(o, i, 4)
        assert got == F.ge4_double(tuple(rows(it)))
        if i < len(PQ):
            assert ed_aff(got) == E.point_add(pairs[i][0], pairs[i][0])
    # extended + extended
    items = [lim(Pe) + lim(Qe) for Pe, Qe in PQ] + [tuple(r) for r in worst_rows(8, 112)]
    o1, o4 = run(ver, "gesl_add", items), run(ver, "ge4_add", items)
    for i, it in enumerate(items):
        r = rows(it)
        g1, g4 = point_out(o1, i, 4), point_out(o4, i, 4)
        assert g1 == F.gesl_add(tuple(r[:4]), tuple(r[4:])) and g4 == F.ge4_add(tuple(r[:4]), tuple(r[4:]))
        assert [val(v) % ED.p for v in g1] == [val(v) % ED.p for v in g4]
        if i < len(PQ):
            assert ed_aff(g1) == E.point_add(*pairs[i])
    # cached and precomputed second operands, every pre / neg combination
    worst8 = []
    for r in worst_rows(8, 113):                             # ypx, ymx, z2 at 2N
        worst8.append(tuple(r[:4]) + tuple([2 * v for v in x] for x in r[4:7]) + (r[7],))
    for neg in (False, True):
        fl = gvm.SLF_NEG if neg else 0
        citems = [lim(Pe) + lim(cached(Qe)) for Pe, Qe in PQ] + worst8
        og, o4 = run(ver, "gesl_add_cached", citems, fl), run(ver, "ge4_add_cached", citems, fl)
        pitems = []
        for (Pe, _), (_, Q) in zip(PQ, pairs):
            x, y = Q
            pitems.append(lim(Pe) + lim((F.canon((y + x) % ED.p), F.canon((y - x) % ED.p), F.canon(2 * F.ED_D * x * y % ED.p))))
        pitems += [t[:6] + (t[7],) for t in worst8]
        op_ = run(ver, "gesl_add_pre", pitems, fl)
        # ge4_add_cached with pre: operand 6 (2 Z2) is null, operand 7 the 2dxy entry
        p4items = [t[:6] + ([0] * 9, t[6]) for t in pitems]
        op4 = run(ver, "ge4_add_cached", p4items, fl | gvm.SLF_PRE)
        for i in range(len(citems)):
            r = rows(citems[i])
            P = tuple(r[:4])
            gc, g4 = point_out(og, i, 4), point_out(o4, i, 4)
            assert gc == F.gesl_add_cached(P, r[4], r[5], r[6], r[7], neg)
            assert g4 == F.ge4_add_cached(P, r[4], r[5], r[6], r[7], False, neg)
            rp = rows(pitems[i])
            gp, gp4 = point_out(op_, i, 4), point_out(op4, i, 4)
            assert gp == F.gesl_add_pre(P, rp[4], rp[5], rp[6], neg)
            assert gp4 == F.ge4_add_cached(P, rp[4], rp[5], F.ZERO, rp[6], True, neg)
            assert [val(v) % ED.p for v in gc] == [val(v) % ED.p for v in g4]
            assert [val(v) % ED.p for v in gp] == [val(v) % ED.p for v in gp4]
            for g in (gc, g4, gp, gp4):
                for v in g:
                    check_nform(v, (i, neg))
            if i < len(PQ):
                P_, Q_ = pairs[i]
                want = E.point_add(P_, E.point_neg(Q_) if neg else Q_)
                assert ed_aff(gc) == ed_aff(g4) == ed_aff(gp) == ed_aff(gp4) == want


def test_ed_decodes(ver):
    encs = decode_encodings()
    vals = [int.from_bytes(e, "little") for e in encs]
    ol, os_ = run(ver, "ed_decode_lenient", vals, words=True), run(ver, "ed_decode_strict", vals, words=True)
    for i, (enc, e) in enumerate(zip(encs, vals)):
        want = E.decode_point(enc)
        ok = bool(ol[i, 64 + gvm.SLS_FLAG])
        assert ok == (want is not None), enc.hex()
        if i % 3 == 0:                                       # the model runs two 250-squaring chains per encoding
            assert (ok, slot(ol, i, 0), slot(ol, i, 1)) == F.efsl_decode(e, False), enc.hex()
        if ok:
            assert (val(slot(ol, i, 0)) % ED.p, val(slot(ol, i, 1)) % ED.p) == (want[0], want[1] % ED.p), enc.hex()
        yv, sign = e & ((1 << 255) - 1), e >> 255
        sok = bool(os_[i, 64 + gvm.SLS_FLAG])
        assert sok == (want is not None and yv < ED.p and not (want[0] == 0 and sign)), enc.hex()
        if i % 3 == 0:
            assert (sok, slot(os_, i, 0), slot(os_, i, 1)) == F.efsl_decode(e, True), enc.hex()
        if sok:
            assert (val(slot(os_, i, 0)) % ED.p, val(slot(os_, i, 1))) == want, enc.hex()


def test_ed_hash_digits(ver):
    rng = random.Random(120)
    L = E.L
    nib = lambda d, n=128: sum(d << (4 * i) for i in range(n))
    # below L the nibbles survive the reduction: 63 nibbles of 8 carry through every position, 63 of 7 through none
    low = [nib(8, 63), nib(7, 63), nib(8, 62), nib(8, 63) - 1, nib(7, 63) + 1, nib(8, 32), nib(8, 32) << 124]
    xs = [0, L - 1, L, 2**512 - 1, nib(8), nib(7)] + low + [m * L + v for v in low for m in (1, 2**200 + 12345, 2**259)]
    xs += [rng.randrange(2**512) for _ in range(300)]
    assert all(x < 2**512 for x in xs)
    out = ver.debug_sl_op("ed_digits", pack(xs, words=True))
    assert (out[:, 64 + gvm.SLS_KNOWN] == 1).all()
    for i, x in enumerate(xs):
        d = [int(v) for v in out[i, :64].astype(np.int32)]
        assert all(-8 <= v < 8 for v in d), hex(x)
        assert sum(v << (4 * j) for j, v in enumerate(d)) == x % L, hex(x)
