"""GPU tests of the secp256k1 key tables, entry by entry (gv_keys_entry and
gv_group_entry, include/gpuverify.h): every entry the resident arena and the
grouped sets hold must be the affine point j * 2^(QW w0(k)) * Q of its key,
computed here by oracle/secp_ref.py's ParsePubKey and plain affine arithmetic.
Comparison is equality of the 64 bytes; nothing here has a tolerance.

The layouts (csrc/gv_kernels.h): QWIN signed QW-bit windows per 128-bit half
in NG groups, P = ceil(QWIN / NG) windows in the first R = QWIN - (P - 1) NG
groups and P - 1 in the rest, group k starting at window w0(k) = k P -
max(0, k - R); a group's table holds the multiples 1..NT = 2^(QW-1) of
2^(QW w0(k)) Q.

Which keys get which entries checked: in the resident arena every entry of
every group of every slot, for all 14 slots and all six layouts (the CPU side
of the largest, 11-bit x 12 groups, is 123k affine additions, about 2 s).  In
the grouped sets (300 to 1,500 rows) every row gets j = 1 and j = NT of every
group, and the rows of the edge keys and the two rows on each side of every
append boundary get every entry."""
import functools
import time

import numpy as np
import pytest

import bench
import gpuverify as gvm
from oracle import oracle as O
from oracle import secp_ref as R

pytestmark = pytest.mark.gpu

P, N_ORD = R.P, R.N
U32 = np.uint32
QWIN = {5: 26, 6: 22, 11: 12, 9: 15}                     # windows per 128-bit half


def w0(qw, ng, k):
    p = -(-QWIN[qw] // ng)
    r = QWIN[qw] - (p - 1) * ng
    return k * p - max(0, k - r)


def group_bits(qw, ng):
    return [qw * w0(qw, ng, k) for k in range(ng)]


def test_group_starts():
    assert group_bits(5, 4) == [0, 35, 70, 100]                    # k4
    assert group_bits(6, 4) == [0, 36, 72, 102]                    # k6
    assert group_bits(6, 11) == [12 * k for k in range(11)]        # kn: two windows per group
    assert group_bits(11, 12) == [11 * k for k in range(12)] and group_bits(11, 6) == [22 * k for k in range(6)]
    assert group_bits(9, 15) == [9 * k for k in range(15)]
    assert group_bits(9, 8) == [18 * k for k in range(7)] + [126]  # the last group holds one window
    for qw, ng in ((5, 4), (5, 6), (5, 7), (5, 9), (6, 4), (6, 11), (11, 12), (11, 6), (9, 15), (9, 8)):
        p = -(-QWIN[qw] // ng)
        r = QWIN[qw] - (p - 1) * ng
        ends = [w0(qw, ng, k) + (p if k < r else p - 1) for k in range(ng)]
        assert ends[:-1] == [w0(qw, ng, k) for k in range(1, ng)] and ends[-1] == QWIN[qw]   # the groups tile the windows


# ---------------------------------------------------------------- reference
def aff_add(a, b):
    """a + b for finite affine points with a != +-b."""
    lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def aff_dbl(a):
    lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    x = (lam * lam - 2 * a[0]) % P
    return x, (lam * (a[0] - x) - a[1]) % P


def xy64(pt):
    return pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def test_fast_add_matches_secp_ref():
    """aff_add / aff_dbl against secp_ref.point_add on 300 points: the multiples of a random point and of -G."""
    for base in (R.point_mul(0x1234567 << 200 | 99, R.G), R.point_neg(R.G)):
        cur = base
        for j in range(2, 152):
            nxt = aff_dbl(cur) if j == 2 else aff_add(cur, base)
            assert nxt == R.point_add(cur, base) and R.is_on_curve(*nxt), j
            cur = nxt
        assert cur == R.point_mul(151, base)


@functools.lru_cache(maxsize=None)
def doublings(pub):
    """[2^i Q for i = 0..136] for the key bytes pub, or None when ParsePubKey rejects them."""
    q = R.parse_pubkey(pub)
    if q is None:
        return None
    out = [q]
    for _ in range(136):
        out.append(aff_dbl(out[-1]))
    return out


_COLUMNS = {}


def column(pub, bit, nt):
    """(nt, 64) bytes: j * 2^bit * Q for j = 1..nt, by nt affine additions of the group base."""
    col = _COLUMNS.setdefault((pub, bit), [])
    base = doublings(pub)[bit]
    while len(col) < nt:
        col.append(base if not col else aff_dbl(base) if len(col) == 1 else aff_add(col[-1], base))
    return np.frombuffer(b"".join(xy64(p) for p in col[:nt]), np.uint8).reshape(nt, 64)


def table(pub, qw, ng):
    """(ng * nt, 64): every entry of every group of the key's tables, group-major; zeros for a rejected key."""
    nt = 1 << (qw - 1)
    if doublings(pub) is None:
        return np.zeros((ng * nt, 64), np.uint8)
    return np.concatenate([column(pub, b, nt) for b in group_bits(qw, ng)])


def ends(pub, qw, ng):
    """(ng * 2, 64): entries j = 1 and j = NT of every group (doublings only: NT is a power of two)."""
    d = doublings(pub)
    if d is None:
        return np.zeros((ng * 2, 64), np.uint8)
    return np.frombuffer(b"".join(xy64(d[b]) + xy64(d[b + qw - 1]) for b in group_bits(qw, ng)), np.uint8).reshape(-1, 64)


def triples_all(slots, qw, ng):
    """Every (slot, group, j) of the slots, slot-major then group-major: the order of table()."""
    nt = 1 << (qw - 1)
    s = np.repeat(np.asarray(slots, U32), ng * nt)
    g = np.tile(np.repeat(np.arange(ng, dtype=U32), nt), len(slots))
    j = np.tile(np.arange(1, nt + 1, dtype=U32), len(slots) * ng)
    return s, g, j


def triples_ends(slots, qw, ng):
    nt = 1 << (qw - 1)
    s = np.repeat(np.asarray(slots, U32), ng * 2)
    g = np.tile(np.repeat(np.arange(ng, dtype=U32), 2), len(slots))
    j = np.tile(np.array([1, nt], U32), len(slots) * ng)
    return s, g, j


def assert_entries(got, want, trip, what):
    """Byte equality, naming the first wrong entries by slot / row, group and entry."""
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        s, g, j = trip
        named = ", ".join(f"(slot {s[i]} group {g[i]} entry {j[i]})" for i in bad[:8])
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} entries wrong, first {named}")


# ------------------------------------------------------------------ the keys
def priv32(d):
    return np.frombuffer(d.to_bytes(32, "big"), np.uint8)


def x_with_point(start, step):
    x = start
    while pow((x * x * x + 7) % P, (P - 1) // 2, P) != 1:
        x += step
    return x


def x_without_point(start):
    x = start
    while pow((x * x * x + 7) % P, (P - 1) // 2, P) != P - 1:
        x += 1
    return x


class Keys:
    """14 slots: 10 valid keys and 4 ParsePubKey rejects, a rejected key first and last."""

    def __init__(self):
        rng = np.random.default_rng(0xE7)
        r1, r2, r3 = (int.from_bytes(rng.bytes(32), "big") % (N_ORD - 1) + 1 for _ in range(3))
        # private keys where they are known (None: a point found by its x)
        self.priv = {"G": 1, "2G": 2, "-G": N_ORD - 1, "lambdaG": R.LAMBDA, "r1": r1, "-r1": N_ORD - r1, "r2": r2, "r3": r3}
        pub = {k: R.pubkey(d) for k, d in self.priv.items()}
        assert pub["G"][1:] == pub["-G"][1:] and pub["r1"][1:] == pub["-r1"][1:]      # both parities of one x
        assert pub["G"][0] != pub["-G"][0] and pub["r1"][0] != pub["-r1"][0]
        lo, hi = x_with_point(1, 1), x_with_point(P - 1, -1)
        assert lo < 2**32 and P - hi < 2**32
        pub["x_small"] = b"\x02" + lo.to_bytes(32, "big")
        pub["x_large"] = b"\x03" + hi.to_bytes(32, "big")
        gx = R.GX.to_bytes(32, "big")
        pub["rej_04"] = b"\x04" + gx
        pub["rej_x_ge_p"] = b"\x02" + (P + 6).to_bytes(32, "big")
        pub["rej_no_root"] = b"\x03" + x_without_point(int.from_bytes(rng.bytes(32), "big") % P).to_bytes(32, "big")
        pub["rej_00"] = b"\x00" + gx
        self.order = ["rej_04", "G", "2G", "-G", "rej_x_ge_p", "lambdaG", "x_small", "x_large", "rej_no_root", "r1",
                      "-r1", "r2", "r3", "rej_00"]
        assert sorted(self.order) == sorted(pub)
        self.pub = pub
        self.list = [pub[k] for k in self.order]
        self.ok = np.array([R.parse_pubkey(p) is not None for p in self.list], np.uint8)
        assert self.ok.sum() == 10 and not self.ok[0] and not self.ok[-1]
        assert R.parse_pubkey(pub["lambdaG"]) == (R.BETA * R.GX % P, R.GY)
        self.arr = np.frombuffer(b"".join(self.list), np.uint8).reshape(-1, 33).copy()


KEYS = Keys()
NK = len(KEYS.list)
LAYOUTS = {                                   # name: (tabs, QW, NG, keys_wide, keys_wide_qw)
    "k4": (0, 5, 4, 2, 0), "kn": (1, 6, 11, 2, 0), "w11x12": (2, 11, 12, 2, 0), "w11x6": (2, 11, 6, 1, 0),
    "w9x15": (2, 9, 15, 2, 9), "w9x8": (2, 9, 8, 1, 9),
}


def open_arena(keys_wide=2, keys_wide_qw=0, devices=(0,)):
    v = gvm.Verifier(list(devices))
    v.set_option("keys_wide_qw", keys_wide_qw)
    v.set_option("keys_wide", keys_wide)
    return v


def expected_arena(pubs, qw, ng):
    return np.concatenate([table(p, qw, ng) for p in pubs])


def check_arena(v, pubs, layout, dev_slot=0, slots=None, what=""):
    """Every entry of every group of the slots (default: all, holding pubs in order) in one read."""
    tabs, qw, ng = LAYOUTS[layout][:3]
    if tabs == 2:
        assert (v.get_option("kw_arena_qw"), v.get_option("kw_arena_ng")) == (qw, ng)
    slots = np.arange(len(pubs), dtype=U32) if slots is None else np.asarray(slots, U32)
    trip = triples_all(slots, qw, ng)
    xy, ok = v.keys_entry(tabs, *trip, dev_slot=dev_slot)
    want_ok = np.array([doublings(p) is not None for p in pubs], np.uint8)
    assert np.array_equal(ok, np.repeat(want_ok, ng << (qw - 1))), f"{what}{layout}: ParsePubKey verdicts"
    assert_entries(xy, expected_arena(pubs, qw, ng), trip, f"{what}{layout} dev_slot {dev_slot}")
    return len(xy)


def einval(fn, *a, **kw):
    with pytest.raises(gvm.GpuVerifyError) as e:
        fn(*a, **kw)
    assert e.value.code == gvm.GV_EINVAL


# ------------------------------------------- 1. resident arena, every layout
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_arena_every_entry(layout):
    tabs, qw, ng, kw, kwq = LAYOUTS[layout]
    nt = 1 << (qw - 1)
    t0 = time.perf_counter()
    expected_arena(KEYS.list, qw, ng)
    t1 = time.perf_counter()
    with open_arena(kw, kwq) as v:
        assert np.array_equal(v.keys_load(KEYS.arr), np.arange(NK))
        n = check_arena(v, KEYS.list, layout)
        assert n == NK * ng * nt
        print(f"{layout}: {n} entries compared, reference {t1 - t0:.2f} s, GPU side {time.perf_counter() - t1:.2f} s")
        one = lambda s, g, j: v.keys_entry(tabs, np.array([s], U32), np.array([g], U32), np.array([j], U32))
        xy, ok = one(1, ng - 1, nt)                                   # the last entry of the last group (slot 1: G)
        assert ok[0] == 1 and xy[0].tobytes() == xy64(doublings(KEYS.pub["G"])[group_bits(qw, ng)[-1] + qw - 1])
        for s, g, j in ((1, ng, 1), (1, 0, 0), (1, 0, nt + 1), (1, 0xFFFFFFFF, 1), (1, 0, 0xFFFFFFFF)):
            einval(one, s, g, j)
        # one bad triple among good ones refuses the call
        einval(v.keys_entry, tabs, np.array([1, 2, 3], U32), np.array([0, ng, 0], U32), np.array([1, 1, 1], U32))
        einval(v.keys_entry, 3, *(np.ones(1, U32),) * 3)
        einval(v.keys_entry, -1, *(np.ones(1, U32),) * 3)
        einval(v.keys_entry, tabs, *(np.ones(1, U32),) * 3, dev_slot=1)
        past = np.array([NK, NK + 7, 4096, 0xFFFFFFFF, 1], U32)      # at or past keys_count: zeros; then a loaded slot
        xy, ok = v.keys_entry(tabs, past, np.zeros(5, U32), np.full(5, nt, U32))
        assert not xy[:4].any() and not ok[:4].any() and ok[4] == 1 and xy[4].any()
        assert v.keys_count == NK


def test_table_sets_a_context_does_not_have():
    with gvm.Verifier([0]) as v:
        v.set_option("keys_wide", 0)
        v.set_option("keys_k6", 0)
        one = (np.ones(1, U32), np.zeros(1, U32), np.ones(1, U32))
        xy, ok = v.keys_entry(0, *one)                                # an empty arena: zeros, not an error
        assert not xy.any() and not ok.any()
        v.keys_load(KEYS.arr)
        check_arena(v, KEYS.list, "k4")
        einval(v.keys_entry, 1, *one)
        einval(v.keys_entry, 2, *one)
        assert v.get_option("kw_arena_qw") == 0
        einval(v.group_entry, 0, *one)                                # no grouped call ran on any set
        einval(v.group_entry, 2, *one)
        einval(v.group_entry, 4, *one)
        einval(v.group_entry, -1, *one)


# ------------------------------------------- 2. chunked and appended loads
def test_load_in_two_calls():
    with open_arena() as v:
        assert np.array_equal(v.keys_load(KEYS.arr[:5]), np.arange(5))
        assert np.array_equal(v.keys_load(KEYS.arr[5:]), np.arange(5, NK))        # the append form: base 5
        for layout in ("k4", "kn", "w11x12"):
            check_arena(v, KEYS.list, layout, what="two loads, ")


def test_load_across_an_arena_growth():
    """4,090 filler keys, then the key set over slots 4,090..4,103: the arenas (4,096 slots at first) grow once and
    their rows move.  The narrow two-window layout keeps the move at 0.5 GiB."""
    rng = np.random.default_rng(0xE8)
    priv = rng.integers(0, 256, size=(4090, 32), dtype=np.uint8)
    priv[:, 0] &= 0x7F
    priv[:, 31] |= 1
    filler = O.pubkey_batch(priv, threads=16)
    with open_arena(1, 9) as v:
        v.keys_load(filler)
        mem = v.get_option("hbm_optional_bytes")
        slots = v.keys_load(KEYS.arr)
        assert np.array_equal(slots, np.arange(4090, 4090 + NK))
        assert v.get_option("hbm_optional_bytes") - mem > 4096 * 128 * 1024       # both arenas doubled
        for layout in ("k4", "kn", "w9x8"):
            check_arena(v, KEYS.list, layout, slots=slots, what="grown, ")
        # ... and the rows that moved: the filler keys on both sides of the old capacity's end and at slot 0
        near = [0, 1, 4088, 4089]
        for layout in ("k4", "kn", "w9x8"):
            check_arena(v, [bytes(filler[i]) for i in near], layout, slots=near, what="moved, ")


# ------------------------------------------------------ 3. gv_keys_replace
@pytest.mark.parametrize("devices", [(0,), (0, 0)], ids=["one_device", "two_devices"])
def test_replace_rewrites_every_entry(devices):
    rng = np.random.default_rng(0xE9)
    new_valid = [R.pubkey(int.from_bytes(rng.bytes(32), "big") % (N_ORD - 1) + 1) for _ in range(2)]
    # slot 1 (G) takes a rejected key, slot 0 (rejected) a valid one, slot 7 (x_large) another; given unsorted
    rep = {7: new_valid[1], 0: new_valid[0], 1: b"\x05" + R.GX.to_bytes(32, "big")}
    final = list(KEYS.list)
    for s, p in rep.items():
        final[s] = p
    with open_arena(devices=devices) as v:
        v.keys_load(KEYS.arr)
        for dev in range(len(devices)):
            check_arena(v, KEYS.list, "w11x12", dev_slot=dev, what="before, ")
        v.keys_replace(np.array(list(rep), U32), np.frombuffer(b"".join(rep.values()), np.uint8).reshape(-1, 33))
        # every slot: the three replaced ones hold the new keys' tables, the eleven others (the neighbours 2, 6
        # and 8 among them) what they held
        for dev in range(len(devices)):
            for layout in ("k4", "kn", "w11x12"):
                check_arena(v, final, layout, dev_slot=dev, what="replaced, ")
        assert v.keys_count == NK and v.get_option("keys_replaced") == 3




# --------------------------------------------------------- 4. grouped sets
N = 16_384
P_BYTES = P.to_bytes(32, "big")
KEY_BYTES = set(KEYS.list)


def has_row(pub):
    """k_dedupe gives a key a row when its prefix is 02 / 03 and x < p (a key without a root included)."""
    return pub[0] in (2, 3) and pub[1:] < P_BYTES


EDGE_ROWS = {p for p in KEYS.list if has_row(p)}                      # 11: the valid keys and the x without a root


def keyset(pub):
    """The distinct keys of a batch that get a row."""
    return {r for r in {bytes(k) for k in np.unique(pub, axis=0)} if has_row(r)}


def edge_items(pub):
    return np.array([bytes(k) in KEY_BYTES for k in pub])


def sample_oracle(pub, sig, dig, exp, seed, must=None):
    idx = np.random.default_rng(seed).choice(len(exp), 1000, replace=False)
    if must is not None:
        idx = np.union1d(np.nonzero(must)[0], idx)
    assert np.array_equal(O.verify_digests(np.ascontiguousarray(pub[idx]), np.ascontiguousarray(sig[idx]),
                                           np.ascontiguousarray(dig[idx]), threads=16), exp[idx])


@functools.lru_cache(maxsize=None)
def fresh_batch(seed, nkeys):
    """16,384 valid items over nkeys keys of the workload generator (never changed by a test)."""
    pub, sig, dig, exp = bench.make_digest_workload(N, seed, nkeys, 0.0, 16)
    sample_oracle(pub, sig, dig, exp, seed)
    assert len(keyset(pub)) == nkeys
    return pub, sig, dig, exp


@pytest.fixture(scope="module")
def batch_x():
    """16,384 items over 280 keys, a fiftieth adversarial (keys of a random x among them, with rows of their own,
    some without a root), and, eight items each at random positions, the 14 of KEYS (11 of them get a row),
    signed where the private key is known; verdicts by construction, the oracle agreeing on every edge-key
    item and a sample."""
    pub, sig, dig, exp = bench.make_digest_workload(N, 0xB1, 280, 0.02, 16)
    pos = np.random.default_rng(31).choice(N, 8 * NK, replace=False).reshape(NK, 8)
    for name, where in zip(KEYS.order, pos):
        pub[where] = np.frombuffer(KEYS.pub[name], np.uint8)
        d = KEYS.priv.get(name)
        if d is None:
            exp[where] = 0                                            # nobody signed for it: the item's signature fails
        else:
            sig[where] = O.sign_batch(np.tile(priv32(d), (8, 1)), np.ascontiguousarray(dig[where]), threads=1)
            exp[where] = 1
    assert edge_items(pub).sum() == 8 * NK
    sample_oracle(pub, sig, dig, exp, 32, edge_items(pub))
    assert 0.5 < exp.mean() < 1 and EDGE_ROWS <= keyset(pub) and 291 <= len(keyset(pub)) <= 360
    return pub, sig, dig, exp


@pytest.fixture(scope="module")
def batch_y(batch_x):
    """batch_x with 640 items replaced by items of 40 keys it does not hold."""
    pub, sig, dig, exp = (a.copy() for a in batch_x)
    new = bench.make_digest_workload(640, 0xB2, 40, 0.0, 16)
    pos = np.random.default_rng(33).choice(np.nonzero(~edge_items(pub))[0], 640, replace=False)
    pub[pos], sig[pos], dig[pos], exp[pos] = new
    sample_oracle(pub, sig, dig, exp, 34)
    assert len(keyset(pub) - keyset(batch_x[0])) == 40 and EDGE_ROWS <= keyset(pub)
    return pub, sig, dig, exp


class DevCalls:
    """Device-resident calls on device 0 of a context opened for this object: the context stream alternates the
    two scratch sets from set 0, so call number c runs on set c % 2."""

    def __init__(self, ver):
        self.ver, self.calls, self.held = ver, 0, {}
        self.words = (N + 63) // 64
        self.bits = ver.dev_alloc(self.words * 8)

    def put(self, name, batch):
        pub, sig, dig, exp = batch
        d = [self.ver.dev_alloc(a.nbytes) for a in (pub, sig, dig)]
        for p, a in zip(d, (pub, sig, dig)):
            self.ver.dev_upload(p, np.ascontiguousarray(a))
        self.held[name] = (d, exp)

    def call(self, name, read=None):
        """One call: (set it ran on, keys built, keys reused); verdicts against construction.  read(set) runs
        between the call's launch and the first wait for it."""
        v = self.ver
        d, exp = self.held[name]
        h0, b0 = v.get_option("group_reuse_hit"), v.get_option("group_reuse_built")
        v.dev_verify_digests(0, N, d[0], d[1], d[2], self.bits)
        s = self.calls % 2
        self.calls += 1
        out = (s, v.get_option("group_reuse_built") - b0, v.get_option("group_reuse_hit") - h0)
        if read:
            read(s)
        v.dev_sync()
        got = np.zeros(self.words, np.uint64)
        v.dev_download(got, self.bits)
        assert np.array_equal(bench.unpack_bits(got, N), exp), f"verdicts of call {self.calls - 1} ({name})"
        return out

    def pair(self, name, read=None):
        return [self.call(name, read), self.call(name, read)]


def cold(n):
    return [(0, n, 0), (1, n, 0)]


def warm(n, built=0):
    return [(0, built, n - built), (1, built, n - built)]


def check_set(v, s, qw, ng, keys, full=(), what=""):
    """Set s holds exactly `keys`, one row each, in the layout (qw, ng): j = 1 and j = NT of every group of every
    row, every entry of the edge keys' rows and of the rows `full`.  Returns {key: row}."""
    nt = 1 << (qw - 1)
    count = len(keys)
    rows = np.arange(count + 8, dtype=U32)                            # ... and eight rows past the count
    assert v.get_option("group_layout") == ng
    one = lambda r, g, j: v.group_entry(s, np.array([r], U32), np.array([g], U32), np.array([j], U32))
    one(0, ng - 1, nt)                                                # the layout's last entry reads
    for g, j in ((ng, 1), (0, 0), (0, nt + 1)):                       # ... and nothing past it
        einval(one, 0, g, j)
    trip = triples_ends(rows, qw, ng)
    key, xy, ok = v.group_entry(s, *trip)
    per = key.reshape(len(rows), ng * 2, 33)
    assert (per == per[:, :1]).all()                                  # one key per row, whatever the entry
    held = [bytes(k) for k in per[:count, 0]]
    assert not per[count:].any() and not xy[count * ng * 2:].any() and not ok[count * ng * 2:].any(), \
        f"{what}set {s}: rows past the key count"
    assert len(set(held)) == count, f"{what}set {s}: a key in two rows"
    assert set(held) == set(keys), f"{what}set {s}: the rows' keys are not the batch's"
    want = np.concatenate([ends(k, qw, ng) for k in held] + [np.zeros((8 * ng * 2, 64), np.uint8)])
    want_ok = np.array([doublings(k) is not None for k in held] + [False] * 8, np.uint8)
    assert np.array_equal(ok, np.repeat(want_ok, ng * 2)), f"{what}set {s}: ParsePubKey verdicts"
    assert_entries(xy, want, trip, f"{what}set {s} layout {qw}x{ng}, j = 1 and NT")
    row_of = {k: r for r, k in enumerate(held)}
    whole = sorted({row_of[k] for k in EDGE_ROWS & set(held)} | {r for r in full if 0 <= r < count})
    if whole:
        trip = triples_all(whole, qw, ng)
        key, xy, ok = v.group_entry(s, *trip)
        assert [bytes(k) for k in key[::ng * nt]] == [held[r] for r in whole]
        assert_entries(xy, np.concatenate([table(held[r], qw, ng) for r in whole]), trip,
                       f"{what}set {s} layout {qw}x{ng}, whole rows")
    return row_of


def open_grouped(promote=0):
    v = gvm.Verifier([0])
    assert v.get_option("group_reuse") == 1 and v.get_option("kg") == 0
    v.set_option("group_promote_min", 0)
    v.set_option("group_promote", promote)
    return v


@pytest.mark.parametrize("ng", [6, 7, 9])
def test_grouped_cold_append_promote_demote(batch_x, batch_y, ng):
    """Per set: a cold call (k4's layout), a warm call that appends 40 keys at the row count, a warm call, the
    promoting rebuild in the ng-group layout, and a batch of 1,500 new keys that sends the set back to k4's
    layout inside the promoted layout's arena.  The cold read runs between the call and the wait for it."""
    kx, ky = keyset(batch_x[0]), keyset(batch_y[0])
    U = len(kx)
    with open_grouped(ng) as v:
        d = DevCalls(v)
        d.put("x", batch_x)
        d.put("y", batch_y)
        rows_x = {}
        assert d.pair("x", read=lambda s: rows_x.update({s: check_set(v, s, 5, 4, kx, what="cold, ")})) == cold(U)
        assert d.pair("y") == warm(len(ky), 40)
        for s in (0, 1):                                              # the rows of x stay, y's 40 follow at row U
            rows = check_set(v, s, 5, 4, kx | ky, full=range(U - 2, U + 2), what="appended, ")
            assert all(rows[k] == r for k, r in rows_x[s].items())
            assert sorted(rows[k] for k in ky - kx) == list(range(U, U + 40))
        assert d.pair("y") == warm(len(ky))
        assert d.pair("y") == cold(len(ky))                           # the promoting rebuild: y's keys from row 0
        assert v.get_option("group_promoted") == 2
        for s in (0, 1):
            check_set(v, s, 5, ng, ky, full=(0, 1, len(ky) - 2, len(ky) - 1), what="promoted, ")
        f = fresh_batch(0xB3, 1500)
        d.put("f", f)
        assert d.pair("f") == cold(1500)
        assert v.get_option("group_demoted") == 2
        for s in (0, 1):                                              # four groups per key in an arena of ng
            check_set(v, s, 5, 4, keyset(f[0]), full=(0, 1, 1498, 1499), what="demoted, ")


@pytest.mark.parametrize("opt, val, qw, route", [("kg", 4, 5, "kg"), ("k6", 1, 6, "k6")])
def test_grouped_explicit_layout(batch_x, opt, val, qw, route):
    kx = keyset(batch_x[0])
    with open_grouped() as v:
        v.set_option(opt, val)
        d = DevCalls(v)
        d.put("x", batch_x)
        assert d.pair("x") == cold(len(kx))
        assert v.route_stats()[route] == 2
        check_set(v, 0, qw, 4, kx, full=(0, 1, len(kx) - 1), what=f"{opt} cold, ")
        assert d.pair("x") == warm(len(kx))
        check_set(v, 1, qw, 4, kx, what=f"{opt} warm, ")


def test_grouped_overflow_flush(batch_x):
    """About 300 + 2,000 rows in use, then a batch of 1,100 other keys: 3,400 rows do not fit the arena's 3,328,
    the set is flushed and the batch's keys are built from row 0."""
    kx = keyset(batch_x[0])
    assert len(kx) + 2000 <= 3328 < len(kx) + 2000 + 1100
    w1, w2 = fresh_batch(0xB4, 2000), fresh_batch(0xB5, 1100)
    assert not keyset(w1[0]) & keyset(w2[0])
    with open_grouped() as v:
        d = DevCalls(v)
        for name, b in (("x", batch_x), ("w1", w1), ("w2", w2)):
            d.put(name, b)
        assert d.pair("x") == cold(len(kx))
        assert v.get_option("group_reuse_rows") == 3328
        assert d.pair("w1") == cold(2000)                             # appended: nothing of x in it
        assert v.get_option("group_reuse_reset") == 0
        check_set(v, 1, 5, 4, kx | keyset(w1[0]), full=range(len(kx) - 2, len(kx) + 2), what="before the flush, ")
        assert d.pair("w2") == cold(1100)
        assert v.get_option("group_reuse_reset") == 2
        for s in (0, 1):
            check_set(v, s, 5, 4, keyset(w2[0]), full=(0, 1, 1098, 1099), what="flushed, ")


def test_host_slice_set(batch_x):
    """A host-buffer call past the pipeline bound groups its slice's keys once on a set of its own (set 2)."""
    pub, sig, dig, exp = batch_x
    with gvm.Verifier([0]) as v:
        v.set_option("pipe_chunk", 4096)                              # 16,384 items in more than one chunk
        v.set_option("slice_plain_first", 0)                          # ... all of them behind the grouping
        b0 = v.group_stats()[0]
        assert np.array_equal(v.verify_batch_digests(pub, sig, dig), exp)
        assert v.group_stats()[0] - b0 == 1
        check_set(v, 2, 5, 4, keyset(pub), what="host slice, ")
        one = (np.zeros(1, U32), np.zeros(1, U32), np.ones(1, U32))
        for s in (0, 1, 3):                                           # no other set has run
            einval(v.group_entry, s, *one)
        assert np.array_equal(v.verify_batch_digests(pub, sig, dig), exp)
        check_set(v, 2, 5, 4, keyset(pub), what="host slice, warm, ")


# ----------------------------------------------------------- 5. read-only
def test_readback_changes_nothing(batch_x):
    kx = keyset(batch_x[0])
    U = len(kx)
    counters = ("group_reuse_launches", "group_reuse_built", "group_reuse_hit", "group_reuse_reset", "group_promoted",
                "group_demoted", "group_layout", "group_reuse_rows", "hbm_optional_bytes", "keys_index_launches",
                "keys_replaced", "kw_arena_qw", "kw_arena_ng")
    with open_grouped(9) as v:
        v.keys_load(KEYS.arr)
        state = lambda: ([v.get_option(k) for k in counters], v.group_stats(), v.route_stats(), v.keys_count,
                         v.keys_generation())
        d = DevCalls(v)
        d.put("x", batch_x)
        assert d.pair("x") == cold(U) and d.pair("x") == warm(U)
        before = state()
        for s in (0, 1):
            check_set(v, s, 5, 4, kx, full=range(U - 2, U))
        n = sum(check_arena(v, KEYS.list, layout) for layout in ("k4", "kn", "w11x12"))
        assert n == NK * (64 + 352 + 12288)
        e = np.zeros(0, U32)
        v.keys_entry(0, e, e, e)
        v.group_entry(0, e, e, e)
        assert state() == before
        assert d.pair("x") == warm(U)                                 # still warm: nothing built, the same verdicts
        assert v.get_option("group_promoted") == 0
        assert d.pair("x") == cold(U)                                 # ... and the promotion after two warm calls stands
        assert v.get_option("group_promoted") == 2
        check_set(v, 0, 5, 9, kx)
