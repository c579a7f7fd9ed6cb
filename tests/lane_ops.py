"""Operand sets and exact references of the one-lane 9 x 29 layers' unit tests
(gv_debug_lane_op on the device, tools/fe29/lane_host.cpp on the host) --
test infrastructure, no GPU.

cases() gives, per op of gpuverify.LNOP, one Case: the items in the hook's
layout and a check of the n x LN_OUT result against Python integers and the
oracles' group laws (oracle/secp_ref.py, oracle/ed25519_ref.py): the value
mod p, the output magnitude the function's comment states, every flag.  The
same Case serves the host build (tests/test_lane_host.py, which also proves
the set sharp against single-fault mutants of the headers) and the device
(tests/test_lane_gpu.py).

Every operand stays inside the bound its function declares: mul
mag(a) mag(b) <= 6, sqr <= 2, sqr3 <= 1, linear results / norm / to_words
inputs <= 7, points X, Y magnitude 1 and Z <= 2, gej29x_add_scaled x 1,
y <= 2, az <= 2, fused extras at 2 (an f29_neg<1> output) and 4 (K_3 - ...).
Magnitude m: every limb <= m B, B = 2^29 + 2^18.
"""
import os
import random
import re

import numpy as np

import fsl_model as F
import gpuverify as gvm
from oracle import ed25519_ref as E
from oracle import secp_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "cosmos-sdk-rootchain_amd", "csrc")
B = (1 << 29) + (1 << 18)
M29 = (1 << 29) - 1
ST = 64                                   # first status word


class Curve:
    def __init__(self, name, p, consts, edge_add):
        self.name, self.p = name, p
        self.pl = [(p >> (29 * i)) & M29 for i in range(9)]
        rows = re.findall(r"\{((?:0x[0-9A-Fa-f]+u,? ?){9})\}", open(os.path.join(CSRC, consts)).read())
        self.kneg = [[int(x.rstrip("u"), 16) for x in r.replace(",", " ").split()] for r in rows]   # kneg[m - 1]
        assert len(self.kneg) == 7 and all(val(r) % p == 0 for r in self.kneg)
        self.edge_add = edge_add          # the neighbours of k p that the canonical-form tests add


def val(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs[:9]))


SECP = Curve("secp256k1", R.P, "secp_fe29_consts.inc", (1, -1, 1 << 29, 977))
ED = Curve("ed25519", E.P, "ed_fe29_consts.inc", (1, -1, 1 << 29, 18, 19))


def canon(v):
    assert 0 <= v < 1 << 261
    return [(v >> (29 * i)) & M29 for i in range(9)]


def is_mag(limbs, m):
    return all(0 <= x <= m * B for x in limbs[:9])


STYLES = ["rand"] * 40 + ["max", "zero", "p", "hi", "hi"]
EDGE_STYLES = ["max", "zero", "p", "hi"]


def rand_mag(rng, m, style, k):
    """the rand_mag styles of tests/test_fe29_host.py, for either curve"""
    cap = m * B
    if style == "max":
        return [cap] * 9
    if style == "zero" or m == 0:
        return [0] * 9
    if style == "p":
        return [x * m for x in k.pl]
    if style == "hi":
        return [rng.randint(cap - 2**20, cap) for _ in range(9)]
    return [rng.randint(0, cap) for _ in range(9)]


def edge_values():
    """both curves' p +- 1 and the 2^255 / 2^256 edges, canonical limbs (magnitude 1)"""
    vs = [1, 2]
    for p in (R.P, E.P):
        vs += [p - 1, p, p + 1, 2 * p - 1, 2 * p + 1]
    vs += [2**255 - 1, 2**255, 2**255 + 1, 2**256 - 1, 2**256, 2**256 + 1, 2**256 + 2**32 + 977, 2**261 - 1]
    return [canon(v) for v in vs]


def field_items(k, mags_list, n, seed):
    """(mags, operands) items: per magnitude tuple every edge style of every
    operand against the others at their cap (all limbs at m B: the column sums
    are maximal and the last carry chi of a reduction is non-zero), the edge
    values in every magnitude-1 position, then random styles."""
    rng = random.Random(seed)
    per = max(n // len(mags_list), 40)
    out = []
    for mags in mags_list:
        for s in EDGE_STYLES:
            out.append((mags, tuple(rand_mag(rng, m, s, k) for m in mags)))
        for j in range(len(mags)):
            for s in EDGE_STYLES:
                out.append((mags, tuple(rand_mag(rng, m, s if i == j else "max", k) for i, m in enumerate(mags))))
            if mags[j] >= 1:
                for e in edge_values():
                    ops = [rand_mag(rng, m, rng.choice(["max", "hi", "rand"]), k) for m in mags]
                    ops[j] = e
                    out.append((mags, tuple(ops)))
        for _ in range(per):
            out.append((mags, tuple(rand_mag(rng, m, rng.choice(STYLES), k) for m in mags)))
    return out


def col8(a, b):
    """column 8 of the schoolbook product: at 2^61 and above, its carry passes 2^32 and chi != 0"""
    return sum(a[i] * b[8 - i] for i in range(9))


def kp_items(k, kmax, seed, reps=3):
    """Every multiple m p, m = 0..kmax, that fits magnitude 7: its plain
    base-2^29 form and reps forms with units of limb i + 1 pushed down into
    limb i up to the cap, each with its neighbours (k.edge_add)."""
    rng = random.Random(seed)
    cap = 7 * B
    out = []
    for m in range(kmax + 1):
        v = m * k.p
        forms = [[(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]]
        for _ in range(reps):
            f = F.kp_limbs(m, k.p, cap + 1, rng)
            if f is not None:
                forms.append(f)
        for f in forms:
            assert val(f) == v and is_mag(f, 7), m
            out.append(f)
            for d in k.edge_add:
                g = list(f)
                if d == 1 << 29:
                    g[1] += 1
                else:
                    g[0] += d
                if is_mag(g, 7):
                    out.append(g)
    return out


# ------------------------------------------------------------------ packing
def pack(items, flags=0, words=False):
    """items: tuples of 9-limb operands (or, words=True, integers of up to 512
    bits) -> the n x LN_IN input of the hook"""
    w = np.zeros((len(items), gvm.LN_IN), np.uint32)
    for i, it in enumerate(items):
        if words:
            w[i, :16] = [(it >> (32 * j)) & 0xFFFFFFFF for j in range(16)]
        else:
            for j, limbs in enumerate(it):
                w[i, 9 * j:9 * j + 9] = limbs[:9]
    w[:, gvm.LN_IN - 1] = np.asarray(flags, np.uint32) | np.uint32(gvm.LNF_WORDS if words else 0)
    return w


def slot(out, i, s):
    return [int(x) for x in out[i, 16 * s:16 * s + 9]]


def words_of(out, i, n=8):
    return sum(int(x) << (32 * j) for j, x in enumerate(out[i, :n]))


class Case:
    """one op's items and the check of its n x LN_OUT result (AssertionError
    names the first wrong item); undefined(out): rows whose result slots the
    function leaves unspecified (an infinite sum's coordinates)"""

    def __init__(self, op, inp, check, undefined=None):
        self.op, self.inp, self._check, self._undef = op, inp, check, undefined

    def check(self, out):
        assert out.shape == (len(self.inp), gvm.LN_OUT)
        assert (out[:, ST + gvm.LNS_KNOWN] == 1).all(), (self.op, "not run")
        assert not out[:, ST + 2].any() and not out[:, ST + 4:].any(), (self.op, "stray status words")
        self._check(out)

    def undefined(self, out):
        return self._undef(out) if self._undef else np.zeros(len(self.inp), bool)


def _padding_zero(out, i, nslots, what):
    for s in range(4):
        lo = 16 * s + (9 if s < nslots else 0)
        assert not out[i, lo:16 * s + 16].any(), (what, i, "slot padding")


def value_case(k, op, items, fn, outmag, nslots=1):
    """fn(*operand values) -> the expected values (one per result slot); outmag(mags) the stated magnitude"""
    def check(out):
        for i, (mags, ops) in enumerate(items):
            want = fn(*[val(o) for o in ops])
            want = want if isinstance(want, tuple) else (want,)
            assert len(want) == nslots
            for s, w in enumerate(want):
                got = slot(out, i, s)
                assert val(got) % k.p == w % k.p, (op, i, mags, s)
                assert is_mag(got, outmag(mags)), (op, i, mags, [hex(x) for x in got])
            _padding_zero(out, i, nslots, op)
            assert out[i, ST + gvm.LNS_FLAG] == 0 and out[i, ST + gvm.LNS_INF] == 0
    return Case(op, pack([ops for _, ops in items]), check)


def flag_case(op, items, pred):
    def check(out):
        for i, ops in enumerate(items):
            assert int(out[i, ST + gvm.LNS_FLAG]) == int(pred(*[val(o) for o in ops])), (op, i, ops)
        assert not out[:, :ST].any()
    return Case(op, pack(items), check)


def words_case(k, op, items):
    def check(out):
        for i, (a,) in enumerate(items):
            assert words_of(out, i) == val(a) % k.p and not out[i, 8:ST].any(), (op, i, a)
    return Case(op, pack(items), check)


MUL_MAGS = [(1, 1), (2, 2), (1, 6), (6, 1), (2, 3), (3, 2), (1, 3)]
ONE = lambda mags: 1


def field_cases(k, pre, n=2000):
    """the ops both curves have (pre: the op names' prefix)"""
    c = {}
    seed = 1000 if k is SECP else 2000
    c[pre + "mul"] = value_case(k, pre + "mul", field_items(k, MUL_MAGS, n, seed + 1), lambda a, b: a * b, ONE)
    c[pre + "sqr"] = value_case(k, pre + "sqr", field_items(k, [(1,), (2,)], n, seed + 2), lambda a: a * a, ONE)
    c[pre + "sub1"] = value_case(k, pre + "sub1", field_items(k, [(m, 1) for m in range(6)], n, seed + 3),
                                 lambda a, b: a - b, lambda mags: mags[0] + 2)
    c[pre + "neg1"] = value_case(k, pre + "neg1", field_items(k, [(1,)], n // 2, seed + 4), lambda a: -a, lambda m: 2)
    for mb in (1, 2, 3):
        c[f"{pre}sub_norm{mb}"] = value_case(k, f"{pre}sub_norm{mb}",
                                             field_items(k, [(m, mb) for m in range(7 - mb)], n, seed + 4 + mb),
                                             lambda a, b: a - b, ONE)
    c[pre + "norm"] = value_case(k, pre + "norm", field_items(k, [(m,) for m in range(1, 8)], n, seed + 8),
                                 lambda a: a, ONE)
    kp = [(f,) for f in kp_items(k, 224 if k is SECP else 448, seed + 9)]
    anym = [ops for _, ops in field_items(k, [(m,) for m in range(1, 8)], n // 2, seed + 10)]
    c[pre + "to_words"] = words_case(k, pre + "to_words", kp + anym)
    c[pre + "is_zero"] = flag_case(pre + "is_zero", kp + anym, lambda a: a % k.p == 0)
    rng = random.Random(seed + 11)
    vals = [0, 1, k.p - 1, k.p, k.p + 1, k.p + 5, 2**255 - 1, 2**255, 2**255 + 19, 2**256 - 1, 2**256 - 2**32 - 977]
    vals += [rng.getrandbits(256) for _ in range(500)]

    def check_from(out):
        for i, v in enumerate(vals):
            got = slot(out, i, 0)
            assert val(got) == (v if k is SECP else v & (2**255 - 1)) and all(x <= M29 for x in got), hex(v)
            _padding_zero(out, i, 1, pre + "from_words")
    c[pre + "from_words"] = Case(pre + "from_words", pack(vals, words=True), check_from)
    chain = field_items(k, [(1,), (2,)], 120, seed + 12)
    c[pre + "inv"] = value_case(k, pre + "inv", chain, lambda a: pow(a, k.p - 2, k.p), ONE)
    return c, kp, anym, chain


# ------------------------------------------------------------ secp256k1
def limbs_of(rng, v, m, k=SECP):
    """v + j p limb-wise for a random j < m: magnitude <= m (tests/test_fe29x_host.py)"""
    j = rng.randrange(0, m)
    return [((v >> (29 * i)) & M29) + j * k.pl[i] for i in range(9)]


def negated(v, k=SECP):
    """-v as f29_neg<1> / e29_neg<1> leaves it: K_1 - the canonical limbs, magnitude 2"""
    return [kn - x for kn, x in zip(k.kneg[0], canon(v % k.p))]


def secp_points(rng):
    ks = [1, 2, 3, R.N - 1, R.LAMBDA] + [rng.randrange(1, R.N) for _ in range(5)]
    return [R.point_mul(s, R.G) for s in ks]


def jac(rng, pt, mz=2):
    z = rng.randrange(1, R.P)
    x, y = pt
    return (limbs_of(rng, x * z * z % R.P, 1), limbs_of(rng, y * z ** 3 % R.P, 1), limbs_of(rng, z, mz))


def aff(out, i):
    x, y, z = (val(slot(out, i, s)) % R.P for s in range(3))
    if z == 0:
        return "Z = 0"
    zi = pow(z, R.P - 2, R.P)
    return (x * zi * zi % R.P, y * zi ** 3 % R.P)


def point_case(op, items, flags, want, zmag, same_on_inf):
    """want[i]: the affine sum, None for infinity.  An infinite result leaves
    the input point in place where same_on_inf (the in-place additions)."""
    def check(out):
        for i, w in enumerate(want):
            inf = bool(out[i, ST + gvm.LNS_INF])
            assert inf == (w is None), (op, i, "infinity")
            assert out[i, ST + gvm.LNS_FLAG] == 0
            if inf:
                if same_on_inf:
                    assert [slot(out, i, s) for s in range(3)] == [list(v) for v in items[i][:3]], (op, i)
                continue
            assert aff(out, i) == w, (op, i)
            assert is_mag(slot(out, i, 0), 1) and is_mag(slot(out, i, 1), 1) and is_mag(slot(out, i, 2), zmag), (op, i)
            _padding_zero(out, i, 3, op)
    undefined = None if same_on_inf else (lambda out: out[:, ST + gvm.LNS_INF] != 0)
    return Case(op, pack(items, flags), check, undefined)


def secp_pairs(rng):
    """(P, Q) with the general case, Q = P (doubling) and Q = -P (infinity) in
    neighbouring lanes: the exceptional lanes diverge inside a wave whose other
    lanes run the regular formula, and the doubling runs after that region"""
    pts = secp_points(rng)
    out = []
    for i, P in enumerate(pts):
        for j in range(6):
            out += [(P, pts[(i + j + 1) % len(pts)]), (P, P) if j % 2 else (P, R.point_neg(P))]
    return out


def secp_cases():
    c, kp, anym, chain = field_cases(SECP, "")
    k = SECP
    n = 2000
    c["multi_ss"] = value_case(k, "multi_ss", field_items(k, [(1, 1), (2, 2), (1, 2)], n, 101),
                               lambda a, b: (a * a, b * b), ONE, 2)
    c["multi_mmm"] = value_case(k, "multi_mmm",
                                field_items(k, [(1, 1, 2, 1, 1, 1), (1, 1, 1, 6, 1, 3), (2, 3, 1, 3, 2, 6), (2, 2, 2, 2, 2, 2)], n, 102),
                                lambda a, b, c_, d, e, f: (a * d, b * e, c_ * f), ONE, 3)
    c["multi_mm"] = value_case(k, "multi_mm", field_items(k, [(1, 1, 3, 1), (2, 2, 3, 3), (1, 6, 6, 1), (1, 1, 1, 1)], n, 103),
                               lambda a, b, c_, d: (a * c_, b * d), ONE, 2)
    c["multi_ssm"] = value_case(k, "multi_ssm", field_items(k, [(1, 1, 1, 2), (2, 2, 2, 3), (1, 2, 6, 1)], n, 104),
                                lambda a, b, c_, d: (a * a, b * b, c_ * d), ONE, 3)
    for s in (1, 2, 3):
        c[f"shl_norm{s}"] = value_case(k, f"shl_norm{s}", field_items(k, [(1,)], n // 2, 104 + s),
                                       lambda a, s=s: a << s, ONE)
    c["mul3_norm"] = value_case(k, "mul3_norm", field_items(k, [(1,), (2,)], n, 108), lambda a: 3 * a, ONE)
    c["is_zero_fast"] = flag_case("is_zero_fast", kp + anym, lambda a: a % k.p == 0)
    rng = random.Random(109)
    eq = []
    for m in range(0, 128, 2):                                # a + m p (magnitude 3 + 4) against a, and against a +- 1
        a = rand_mag(rng, 3, "rand", k)
        f = F.kp_limbs(m, k.p, 4 * B + 1, rng)
        g = [x + y for x, y in zip(a, f)]
        eq += [(g, a), (g, [a[0] ^ 1] + a[1:]), (a, g)]
    eq += [ops for _, ops in field_items(k, [(7, 7), (1, 7)], 200, 110)]
    c["equal"] = flag_case("equal", eq, lambda a, b: (a - b) % k.p == 0)
    c["sqrt"] = value_case(k, "sqrt", chain, lambda a: pow(a, (k.p + 1) // 4, k.p), ONE)
    c["x_sqrt"] = value_case(k, "x_sqrt", chain, lambda a: pow(a, (k.p + 1) // 4, k.p), ONE)
    c["x_mul"] = value_case(k, "x_mul", field_items(k, MUL_MAGS, n, 111), lambda a, b: a * b, ONE)
    ext = [(ma, mb, me) for ma, mb in MUL_MAGS for me in (2, 4)]
    c["x_mul_p1"] = value_case(k, "x_mul_p1", field_items(k, ext, n, 112), lambda a, b, e: a * b + e, ONE)
    c["x_mul_p8"] = value_case(k, "x_mul_p8", field_items(k, ext, n, 113), lambda a, b, e: a * b + 8 * e, ONE)
    c["x_mul2"] = value_case(k, "x_mul2",
                             field_items(k, [(1, 3, 2, 1), (1, 1, 1, 1), (2, 1, 1, 4), (1, 5, 1, 1), (3, 1, 1, 3)], n, 114),
                             lambda a, b, c_, d: a * b + c_ * d, ONE)
    c["x_sqr"] = value_case(k, "x_sqr", field_items(k, [(1,), (2,)], n, 115), lambda a: a * a, ONE)
    sext = [(m, me) for m in (1, 2) for me in (2, 4)]
    c["x_sqrd_p1"] = value_case(k, "x_sqrd_p1", field_items(k, sext, n, 116), lambda a, e: a * a + e, ONE)
    c["x_sqrd_p8"] = value_case(k, "x_sqrd_p8", field_items(k, sext, n, 117), lambda a, e: a * a + 8 * e, ONE)
    c["x_sqr3"] = value_case(k, "x_sqr3", field_items(k, [(1,)], n, 118), lambda a: 3 * a * a, ONE)

    # ---- group
    rng = random.Random(120)
    pts = secp_points(rng)
    ditems = [jac(rng, P) for P in pts for _ in range(6)]
    dwant = [R.point_add(P, P) for P in pts for _ in range(6)]
    c["gej_double"] = point_case("gej_double", ditems, 0, dwant, 2, False)
    c["gejx_double"] = point_case("gejx_double", ditems, 0, dwant, 1, False)
    pairs = secp_pairs(rng)
    items, want = [], []
    for n_, (P, Q) in enumerate(pairs):                       # Jacobian + affine, plain and negated entries
        for neg in (False, True):
            y = negated(-Q[1]) if neg and n_ % 2 else limbs_of(rng, Q[1], 2)
            items.append(jac(rng, P) + (limbs_of(rng, Q[0], 2), y))
            want.append(R.point_add(P, Q))
    c["gej_add_ge"] = point_case("gej_add_ge", items, 0, want, 2, True)   # Q = P: gej29_double's Z
    items, want = [], []
    for n_, (P, Q) in enumerate(pairs):                       # the entry on the curve scaled by s: az = Z1 s
        for var in range(3):
            A = jac(rng, P)
            z1 = val(A[2]) % R.P
            s = 1 if var == 0 else rng.randrange(1, R.P)      # var 0: az = a.z itself
            si = pow(s, R.P - 2, R.P)
            ex, ey = Q[0] * si * si % R.P, Q[1] * si ** 3 % R.P
            y = negated(-ey) if var == 2 else limbs_of(rng, ey, 2 if n_ % 2 else 1)
            az = list(A[2]) if var == 0 else limbs_of(rng, z1 * s % R.P, 2)
            items.append(A + (limbs_of(rng, ex, 1), y, az))
            want.append(R.point_add(P, Q))
    c["gejx_add_scaled"] = point_case("gejx_add_scaled", items, 0, want, 1, True)
    items, flags, want = [], [], []
    for P, Q in pairs:                                        # Jacobian + Jacobian, every combination of infinite inputs
        for fl, w in ((0, R.point_add(P, Q)), (gvm.LNF_INF_A, Q), (0, R.point_add(P, Q)), (gvm.LNF_INF_B, P),
                      (gvm.LNF_INF_A | gvm.LNF_INF_B, None)):
            items.append(jac(rng, P) + jac(rng, Q))
            flags.append(fl)
            want.append(w)
    c["gej_add_gej"] = point_case("gej_add_gej", items, flags, want, 2, False)
    return c


# -------------------------------------------------------------- ed25519
def ext(rng, pt, mz=2, k=ED):
    """affine -> extended: X, Y, T magnitude 1, Z <= mz"""
    z = rng.randrange(1, k.p)
    x, y = pt
    return (canon(x * z % k.p), canon(y * z % k.p), limbs_of(rng, z, mz, k), canon(x * y % k.p * z % k.p))


def ed_aff(out, i, t=True):
    X, Y, Z, T = (val(slot(out, i, s)) % E.P for s in range(4))
    if Z == 0:
        return "Z = 0"
    zi = pow(Z, E.P - 2, E.P)
    if t:
        assert T * Z % E.P == X * Y % E.P, (i, "T Z != X Y")
    else:
        assert not out[i, 48:64].any(), (i, "T written")
    return (X * zi % E.P, Y * zi % E.P)


def ed_point_case(op, items, flags, want, t=True):
    def check(out):
        for i, w in enumerate(want):
            assert ed_aff(out, i, t) == w, (op, i)
            for s in range(4 if t else 3):
                assert is_mag(slot(out, i, s), 1), (op, i, s)
            _padding_zero(out, i, 4 if t else 3, op)
    return Case(op, pack(items, flags), check)


def ed_pairs(rng):
    pts = F.ed_points(rng)
    pts += [p for p in (E.decode_point(e) for e in F.decode_encodings()[-30:]) if p is not None][:6]
    return [(P, Q) for P in pts for Q in pts[:4] + [E.IDENT, E.B, P, E.point_neg(P)]]


def hash_scalars():
    """the vector list of tests/test_sliced_gpu.py::test_ed_hash_digits"""
    rng = random.Random(120)
    L = E.L
    nib = lambda d, n=128: sum(d << (4 * i) for i in range(n))
    low = [nib(8, 63), nib(7, 63), nib(8, 62), nib(8, 63) - 1, nib(7, 63) + 1, nib(8, 32), nib(8, 32) << 124]
    xs = [0, L - 1, L, 2**512 - 1, nib(8), nib(7)] + low + [m * L + v for v in low for m in (1, 2**200 + 12345, 2**259)]
    xs += [rng.randrange(2**512) for _ in range(300)]
    assert all(x < 2**512 for x in xs)
    return xs


def comb_scalars(rb):
    """the cases of tests/test_ed_comb_host.py, its full-ripple vectors of every radix included"""
    import test_ed_comb_host as C
    hs = C.cases(rb)
    for r in (4, 6, 8):
        nw, ne = C.NW[r], 1 << (r - 1)
        hs.append(ne + sum((ne - 1) << (r * w) for w in range(1, nw - 1)))
    return hs


def ed_cases():
    k = ED
    c, kp, anym, chain = field_cases(ED, "ed_")
    n = 2000
    c["ed_add_norm"] = value_case(k, "ed_add_norm", field_items(k, [(ma, mb) for ma in range(1, 7) for mb in (1, 7 - ma)], n, 201),
                                  lambda a, b: a + b, ONE)
    c["ed_is_negative"] = flag_case("ed_is_negative", kp[::5] + anym, lambda a: (a % k.p) & 1)
    c["ed_pow22523"] = value_case(k, "ed_pow22523", chain, lambda a: pow(a, (k.p - 5) // 8, k.p), ONE)

    rng = random.Random(210)
    pairs = ed_pairs(rng)
    PQ = [(ext(rng, P), ext(rng, Q, 1)) for P, Q in pairs]
    dbl = [E.point_add(P, P) for P, _ in pairs]
    c["ge_dbl_t"] = ed_point_case("ge_dbl_t", [Pe for Pe, _ in PQ], 0, dbl)
    c["ge_dbl_nt"] = ed_point_case("ge_dbl_nt", [Pe for Pe, _ in PQ], 0, dbl, t=False)
    d2 = 2 * E.D % k.p
    citems, pitems, flags, want = [], [], [], []
    for i, ((P, Q), (Pe, Qe)) in enumerate(zip(pairs, PQ)):
        for neg in (0, 1):
            P1 = ext(rng, P, 1)                               # ge_add_cached: p magnitude 1
            X, Y, Z, T = (val(v) % k.p for v in Qe)
            citems.append(P1 + (canon((Y + X) % k.p), canon((Y - X) % k.p), canon(2 * Z % k.p), canon(d2 * T % k.p)))
            x, y = Q
            pitems.append(P1 + (canon((y + x) % k.p), canon((y - x) % k.p), canon(d2 * x * y % k.p)))
            flags.append(gvm.LNF_NEG if neg else 0)
            want.append(E.point_add(P, E.point_neg(Q) if neg else Q))
    c["ge_add_cached"] = ed_point_case("ge_add_cached", citems, flags, want)
    c["ge_add_pre"] = ed_point_case("ge_add_pre", pitems, flags, want)

    exts = [ext(rng, P, 1) for P, _ in pairs[::3]]
    affs = [P for P, _ in pairs[::3]]

    def check_cached(out):
        for i, (x, y) in enumerate(affs):
            ypx, ymx, z2, t2d = (val(slot(out, i, s)) % k.p for s in range(4))
            zi = pow(z2 * pow(2, k.p - 2, k.p) % k.p, k.p - 2, k.p)
            assert (ypx * zi % k.p, ymx * zi % k.p, t2d * zi % k.p) == ((y + x) % k.p, (y - x) % k.p, d2 * x * y % k.p), i
            assert all(is_mag(slot(out, i, s), 1) for s in range(4))
    c["ge_to_cached"] = Case("ge_to_cached", pack(exts), check_cached)

    def check_pre(out):
        for i, (x, y) in enumerate(affs):
            got = tuple(val(slot(out, i, s)) % k.p for s in range(3))
            assert got == ((y + x) % k.p, (y - x) % k.p, d2 * x * y % k.p), i
            assert all(is_mag(slot(out, i, s), 1) for s in range(3)) and not out[i, 48:ST].any()
    c["ge_to_pre"] = Case("ge_to_pre", pack(exts), check_pre)
    c["ge_neg"] = ed_point_case("ge_neg", exts, 0, [E.point_neg(P) for P in affs])

    encs = F.decode_encodings()
    evals = [int.from_bytes(e, "little") for e in encs]

    def check_frombytes(out):
        for i, enc in enumerate(encs):
            w = E.decode_point(enc)
            assert bool(out[i, ST + gvm.LNS_FLAG]) == (w is not None), enc.hex()
            if w is not None:
                assert ed_aff(out, i) == w, enc.hex()
                assert val(slot(out, i, 2)) == 1 and all(is_mag(slot(out, i, s), 1) for s in range(4))
    c["ge_frombytes"] = Case("ge_frombytes", pack(evals, words=True), check_frombytes)

    tb = [ext(rng, P) for P, _ in pairs[::2]]

    def check_tobytes(out):
        for i, (P, _) in enumerate(pairs[::2]):
            assert words_of(out, i).to_bytes(32, "little") == E.encode_point(P) and not out[i, 8:ST].any(), i
    c["ge_tobytes"] = Case("ge_tobytes", pack(tb), check_tobytes)

    items, flags, want, tflag = [], [], [], []
    for i, (P, A) in enumerate(pairs):                        # acc P, table of A: every entry, both signs, both T_OUT
        for e in range(9):
            neg, nt = (i + e) & 1, (i + e) >> 1 & 1
            if e in (0, 8) or i % 3 == 0:
                items.append(ext(rng, P, 1) + ext(rng, A, 1))
                flags.append((e << gvm.LNF_ENTRY_SHIFT) | (gvm.LNF_NEG if neg else 0) | (gvm.LNF_NOT if nt else 0))
                eA = E.point_mul(e, A)
                want.append(E.point_add(P, E.point_neg(eA) if neg else eA))
                tflag.append(not nt)

    def check_tab(out):
        for i, w in enumerate(want):
            assert ed_aff(out, i, tflag[i]) == w, ("ge_add_tab", i, hex(flags[i]))
            assert all(is_mag(slot(out, i, s), 1) for s in range(4))
    c["ge_add_tab"] = Case("ge_add_tab", pack(items, flags), check_tab)

    xs = hash_scalars()

    def check_reduce(out):
        for i, x in enumerate(xs):
            assert words_of(out, i) == x % E.L and not out[i, 8:ST].any(), hex(x)
    c["sc_reduce512"] = Case("sc_reduce512", pack(xs, words=True), check_reduce)
    ss = [0, 1, E.L - 1, E.L, E.L + 1, 2**252, 2**252 - 1, 2**253, 2**256 - 1, E.L + 2**128, E.L - 2**128]
    ss += [random.Random(211).randrange(2**256) >> (3 * (j % 2)) for j in range(200)]

    def check_min(out):
        for i, s in enumerate(ss):
            assert bool(out[i, ST + gvm.LNS_FLAG]) == (s < E.L), hex(s)
    c["sc_minimal"] = Case("sc_minimal", pack(ss, words=True), check_min)
    hs = [x % E.L for x in xs]

    def check_radix16(out):
        for i, h in enumerate(hs):
            d = [int(v) for v in out[i, :64].astype(np.int32)]
            assert all(-8 <= v < 8 for v in d[:63]) and 0 <= d[63] <= 2, hex(h)
            assert sum(v << (4 * j) for j, v in enumerate(d)) == h, hex(h)
    c["ed_radix16"] = Case("ed_radix16", pack(hs, words=True), check_radix16)
    for rb in (4, 6, 8):
        cs = comb_scalars(rb)

        def check_comb(out, rb=rb, cs=cs):
            nw, ne = (253 + rb - 1) // rb, 1 << (rb - 1)
            for i, h in enumerate(cs):
                d = [int(v) for v in out[i, :64].astype(np.int32)]
                assert not any(d[nw:]) and sum(v << (rb * w) for w, v in enumerate(d[:nw])) == h, (rb, hex(h))
                assert all(-ne <= v < ne for v in d[:nw - 1]) and 0 <= d[nw - 1] <= {4: 1, 6: 1, 8: 17}[rb], (rb, hex(h))
        c[f"ed_comb{rb}"] = Case(f"ed_comb{rb}", pack(cs, words=True), check_comb)
    return c


_CASES = {}


def cases():
    """op name -> Case, for every op of gpuverify.LNOP (built once, never changed)"""
    if not _CASES:
        _CASES.update(secp_cases())
        _CASES.update(ed_cases())
        assert set(_CASES) == set(gvm.LNOP), set(gvm.LNOP) ^ set(_CASES)
        for c in _CASES.values():
            c.inp.setflags(write=False)
    return _CASES


# --------------------------------------------------------------- host build
def host_lib(chains, csrc=CSRC, traps=True, out_dir=None):
    """tools/fe29/lane_host.cpp built by g++ against the headers in csrc, in
    the one-chain or the two-chain configuration; CalledProcessError if it
    does not compile, FileNotFoundError without a compiler"""
    import ctypes
    import subprocess
    import tempfile
    d = out_dir or tempfile.mkdtemp()
    so = os.path.join(d, f"lane_host_{chains}.so")
    cmd = ["g++", "-O2", "-std=c++17", "-I", csrc, f"-DF29_NCH={chains}", f"-DF29X_NCH={chains}", "-shared", "-fPIC",
           "-o", so, os.path.join(REPO, "tools", "fe29", "lane_host.cpp")]
    if not traps:
        cmd.insert(1, "-DLANE_NO_TRAPS")
    subprocess.run(cmd, check=True, capture_output=True)
    L = ctypes.CDLL(so)
    L.lane_host_ops.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.lane_host_ops.restype = ctypes.c_int
    assert L.lane_host_chains() == chains * 11
    return L


def host_run(L, op, inp):
    inp = np.ascontiguousarray(inp, np.uint32)
    out = np.full((inp.shape[0], gvm.LN_OUT), 0xA5A5A5A5, np.uint32)
    rc = L.lane_host_ops(gvm.LNOP[op] if isinstance(op, str) else op, inp.shape[0], inp.ctypes.data, out.ctypes.data)
    assert rc == 0, (op, rc)
    return out
