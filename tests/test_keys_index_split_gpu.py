"""GPU tests of "keys_index_split" (include/gpuverify.h): a pub33 device batch
the pubkey index routes, a few of whose keys are NOT resident, still runs on
the arena -- the non-resident items are compacted into a sub-batch (k_kidx_split),
verified by their key bytes on the pub33 routes and their accept bits merged in
(k_bits_merge).

The method: load every key of a world EXCEPT a chosen subset, so exactly the
items of those keys miss.  The expected verdicts are the C oracle's, which do
not depend on residency; every split call is also compared, bit for bit, with
the same call under "keys_index_split" 0 (today's fall-through).  The digest
world, the helpers and the host model are those of test_keys_index_gpu.py."""
import numpy as np
import pytest

import gpuverify as gvm
from golden_io import load_digest_vectors, load_msg_vectors
from kidx_model import NONE, SEED, Model, homed_keys, load_model
from oracle import oracle as O
from test_keys_index_gpu import (ARENA_ROUTES, SIZES, DevBufs, Digests, dev_digests, dev_msgs, first_seen,
                                 fresh_privs, signed_items, start, unpack)

pytestmark = pytest.mark.gpu

SUB_ROUTES = {"pub33", "item_f", "lat"}
REJECTED = ("bad_prefix", "x_ge_p", "x_nonresidue")
BIG = 1 << 20                                          # a bound no test batch reaches


# ---------------------------------------------------------------- helpers
def counters(ver, slot=0):
    c = {k: ver.get_option("keys_index_" + k) for k in ("hit", "miss", "launches", "split_calls", "split_items")}
    c["routes"] = ver.route_stats(slot)
    return c


def moved(ver, fn, slot=0):
    """fn's result, the index counters it moved, the routes it took."""
    c0 = counters(ver, slot)
    out = fn()
    c1 = counters(ver, slot)
    routes = {k: c1["routes"][k] - c0["routes"][k] for k in c1["routes"] if c1["routes"][k] != c0["routes"][k]}
    return out, {k: c1[k] - c0[k] for k in c0 if k != "routes"}, routes


def assert_split(delta, routes, m, sub=SUB_ROUTES):
    assert delta == {"hit": 1, "miss": 0, "launches": 3, "split_calls": 1, "split_items": m}, (delta, m)
    assert sum(routes.values()) == 2, routes
    assert sum(v for k, v in routes.items() if k in ARENA_ROUTES) == 1, routes
    assert sum(v for k, v in routes.items() if k in sub) == 1, routes


def assert_fell_through(delta, routes, expect_routes):
    assert delta == {"hit": 0, "miss": 1, "launches": 1, "split_calls": 0, "split_items": 0}, delta
    assert routes == expect_routes and not set(routes) & ARENA_ROUTES, (routes, expect_routes)


def both_ways(ver, call, want, m, sub=SUB_ROUTES):
    """call() with the split on (a bound past m) and with "keys_index_split" 0:
    the oracle's verdicts both times, the same bits, a split and a fall-through."""
    ver.set_option("keys_index_split", BIG)
    got, delta, routes = moved(ver, call)
    assert_split(delta, routes, m, sub)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])
    ver.set_option("keys_index_split", 0)
    off, delta, plain = moved(ver, call)
    assert delta == {"hit": 0, "miss": 1, "launches": 1, "split_calls": 0, "split_items": 0}, delta   # no split, no merge
    assert not set(plain) & ARENA_ROUTES, plain
    assert np.array_equal(off, got)
    return plain


# ---------------------------------------------------------------- the world
class World(Digests):
    """The digest world with a fixed subset of its keys marked to stay out of
    the arena: 16 of the random keys (80 items, a quarter with a corrupted
    signature), a golden key of each ParsePubKey rejection class and two valid
    golden keys."""

    def __init__(self):
        super().__init__()
        gpub, _, _, _, cats = load_digest_vectors()
        cat_keys = {}
        for p, c in zip(gpub, cats):
            cat_keys.setdefault(c, []).append(p.tobytes())
        golden = {k.tobytes() for k in gpub}
        rand = [k.tobytes() for k in self.keys if k.tobytes() not in golden]
        assert len(rand) == 60
        out = set(rand[:16])
        self.out_rejected = {c: cat_keys[c][0] for c in REJECTED}
        out |= set(self.out_rejected.values())
        out |= set(sorted(set(cat_keys["valid"]))[:2])
        self.out = out
        self.is_out = np.array([k.tobytes() in out for k in self.pub])
        self.resident_keys = np.array([k for k in self.keys if k.tobytes() not in out], np.uint8)
        self.miss_items = np.nonzero(self.is_out)[0]
        self.hit_items = np.nonzero(~self.is_out)[0]
        assert len(self.miss_items) >= 90 and len(self.hit_items) >= 600
        # what the sub-batch has to answer: accepted and refused signatures of valid keys, every rejection class
        w = self.want[self.miss_items]
        assert w.sum() >= 50 and (w == 0).sum() >= 20
        for c, k in self.out_rejected.items():
            assert any(p.tobytes() == k for p in self.pub[self.miss_items]), c

    def batch(self, n, miss_at, rot=0):
        """n items of the world, the ones at the positions miss_at from the
        non-resident keys and all others resident: (pub, sig, dig, want)."""
        miss_at = sorted(set(int(p) for p in miss_at if 0 <= p < n))
        assert len(miss_at) <= len(self.miss_items)
        pick = np.zeros(n, np.int64)
        is_m = np.zeros(n, bool)
        is_m[miss_at] = True
        pick[is_m] = np.roll(self.miss_items, -rot)[:len(miss_at)]
        pick[~is_m] = np.resize(np.roll(self.hit_items, -rot), n - len(miss_at))   # (cyclic past the last one)
        return (np.ascontiguousarray(self.pub[pick]), np.ascontiguousarray(self.sig[pick]),
                np.ascontiguousarray(self.dig[pick]), self.want[pick])


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    v.set_option("lat_max", 0)
    assert v.get_option("keys_index_split") == 0       # the default
    v.arena_tag = None
    yield v
    v.close()


def arena(ver, tag, keys, keys_wide=0, seed=None):
    """Exactly `keys` resident, with the index (reloaded only when another test's arena is in place)."""
    if ver.arena_tag != tag:
        ver.arena_tag = None
        start(ver, keys_wide=keys_wide, seed=seed)
        ver.keys_load(keys)
        ver.arena_tag = tag
    ver.set_option("keys_index", 1)
    assert ver.get_option("keys_index_live") == 1 and ver.get_option("keys_index_left_out") == 0


# ---------------------------------------------------------------- option
def test_option_range_and_default(ver):
    assert ver.get_option("keys_index_split") == 0
    for val in (1, 4096, 0xFFFFFF00, 0):
        ver.set_option("keys_index_split", val)
        assert ver.get_option("keys_index_split") == val
    for val in (-1, 0xFFFFFF01):
        with pytest.raises(gvm.GpuVerifyError) as e:
            ver.set_option("keys_index_split", val)
        assert e.value.code == gvm.GV_EINVAL
    assert ver.get_option("keys_index_split") == 0
    for key in ("keys_index_split_calls", "keys_index_split_items"):
        assert ver.get_option(key) >= 0
        with pytest.raises(gvm.GpuVerifyError):
            ver.set_option(key, 0)


# ---------------------------------------------------------------- positions
def position_cases(n):
    cases = {"ends and word edge": [0, 63, 64, n - 1]}
    if n > 40:
        cases["two in one word"] = [3, 40]
    if n > 130:
        cases["word edges"] = [63, 64, 127, 128, n - 2]
    if n >= 128:
        cases["a whole wave"] = list(range(64, 128))
        cases["a whole wave and neighbours"] = list(range(63, 129)) + [n - 1]
    return cases


@pytest.mark.parametrize("n", SIZES + [None])
def test_positions(ver, world, n):
    """Misses at the batch's ends, on both sides of a bitmap word's edge, two in
    one word, one whole wave of 64: sizes around the wave and block edges."""
    arena(ver, "world", world.resident_keys)
    n = n or len(world.pub)
    try:
        for rot, (name, at) in enumerate(position_cases(n).items()):
            pub, sig, dig, want = world.batch(n, at, rot=7 * rot)
            m = len({p for p in at if 0 <= p < n})
            assert m >= 1, name
            both_ways(ver, lambda: dev_digests(ver, pub, sig, dig), want, m)
    finally:
        ver.set_option("keys_index_split", 0)


def test_whole_world_every_key_kind(ver, world):
    """The world in its own order, every item of the non-resident keys split
    off: valid keys with accepted and with corrupted signatures, a key of each
    ParsePubKey rejection class, on a caller stream too."""
    arena(ver, "world", world.resident_keys)
    m = len(world.miss_items)
    st = ver.stream_create()
    try:
        for stream in (None, st):
            both_ways(ver, lambda: dev_digests(ver, world.pub, world.sig, world.dig, stream=stream), world.want, m)
    finally:
        ver.stream_destroy(st)
        ver.set_option("keys_index_split", 0)


def test_one_key_repeated_over_many_items(ver, world):
    arena(ver, "world", world.resident_keys)
    key = world.pub[world.miss_items[world.want[world.miss_items] == 1][0]]
    same = np.nonzero((world.pub == key).all(axis=1))[0]
    assert len(same) >= 5 and 0 < world.want[same].sum()
    reps = np.tile(same, 60)[:300]                     # 300 items of ONE non-resident key, spread
    pick = np.concatenate([world.hit_items[:400], reps])
    pick = pick[np.random.default_rng(0x5B1).permutation(len(pick))]
    pub, sig, dig = (np.ascontiguousarray(a[pick]) for a in (world.pub, world.sig, world.dig))
    try:
        both_ways(ver, lambda: dev_digests(ver, pub, sig, dig), world.want[pick], 300)
    finally:
        ver.set_option("keys_index_split", 0)


# ---------------------------------------------------------------- the bound
def test_the_bound(ver, world):
    """M equal to the option splits; one above it falls through whole, on the
    routes of the option-0 call; option 0 launches the lookup alone."""
    arena(ver, "world", world.resident_keys)
    pub, sig, dig, want = world.batch(300, [0, 5, 64, 65, 130, 200, 299])
    call = lambda: dev_digests(ver, pub, sig, dig)
    try:
        plain = both_ways(ver, call, want, 7)
        ver.set_option("keys_index_split", 7)
        got, delta, routes = moved(ver, call)
        assert_split(delta, routes, 7)
        assert np.array_equal(got, want)
        ver.set_option("keys_index_split", 6)
        got, delta, routes = moved(ver, call)
        assert_fell_through(delta, routes, plain)
        assert np.array_equal(got, want)
        # no miss: the keyed route as without the option (one lookup, no split, no merge)
        pub, sig, dig, want = world.batch(300, [])
        got, delta, routes = moved(ver, lambda: dev_digests(ver, pub, sig, dig))
        assert delta == {"hit": 1, "miss": 0, "launches": 1, "split_calls": 0, "split_items": 0}
        assert set(routes) <= ARENA_ROUTES and sum(routes.values()) == 1
        assert np.array_equal(got, want)
    finally:
        ver.set_option("keys_index_split", 0)


# ---------------------------------------------------------------- both sub-batch routes
@pytest.mark.parametrize("lat_sliced", [1, 0])
def test_sub_batch_on_the_small_batch_kernels(ver, world, lat_sliced):
    """The default "lat_max": the main batch (past it) on the arena, the
    sub-batch -- 9 items, then about a thousand -- on a fused small-batch
    kernel, sliced and not."""
    arena(ver, "world", world.resident_keys)
    reps = gvm.LAT_MAX_DEFAULT // len(world.pub) + 1
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1)))
    n = reps * len(world.pub)
    assert n > gvm.LAT_MAX_DEFAULT
    try:
        ver.set_option("lat_max", gvm.LAT_MAX_DEFAULT)
        ver.set_option("lat_sliced", lat_sliced)
        pub, sig, dig, want = (tile(a) for a in (world.pub, world.sig, world.dig, world.want))
        m = reps * len(world.miss_items)
        assert 512 < m <= gvm.LAT_SL_MAX_DEFAULT
        both_ways(ver, lambda: dev_digests(ver, pub, sig, dig), want, m, sub={"lat"})
        few, full = world.batch(600, [0, 1, 63, 64, 400, 401, 402, 500, 599]), world.batch(600, [])
        reps = gvm.LAT_MAX_DEFAULT // 600 + 1
        pub, sig, dig, want = (np.ascontiguousarray(np.concatenate([a, tile(b)])) for a, b in zip(few, full))
        assert len(pub) > gvm.LAT_MAX_DEFAULT and len(want) == len(pub)
        both_ways(ver, lambda: dev_digests(ver, pub, sig, dig), want, 9, sub={"lat"})
    finally:
        ver.set_option("lat_sliced", 1)
        ver.set_option("lat_max", 0)
        ver.set_option("keys_index_split", 0)


def test_sub_batch_on_the_per_item_pipeline(ver, world):
    """"lat_max" 0: the sub-batch takes the throughput pipeline by key bytes."""
    arena(ver, "world", world.resident_keys)
    try:
        both_ways(ver, lambda: dev_digests(ver, world.pub, world.sig, world.dig), world.want, len(world.miss_items),
                  sub={"pub33", "item_f"})
    finally:
        ver.set_option("keys_index_split", 0)


# ---------------------------------------------------------------- a key the index left out
def test_key_the_index_left_out_is_answered_by_the_sub_batch(ver):
    """Fixed seed: 16 probe windows filled end to end with keys homed on them,
    then real keys -- those whose home lies in the filled stretch find no word
    within the probe bound (the host model says which).  They are resident in
    the arena and a miss in the index: their items are split off."""
    lib = load_model()
    P = lib.kidx_probe_bound()
    ver.arena_tag = None
    start(ver, seed=SEED)
    ver.keys_load(homed_keys(lib, 512, 0, 1, stream=31))
    T = ver.get_option("keys_index_words")
    start(ver, seed=SEED)
    crowd = np.concatenate([homed_keys(lib, T, 1000 + P * w, P, stream=40 + w) for w in range(16)])
    rng = np.random.default_rng(0x5B2)
    priv = fresh_privs(rng, 120)
    real = O.pubkey_batch(priv, threads=8)
    m = Model(lib, T, cap=len(crowd) + len(real))
    m.load(crowd)
    assert m.left == 0
    m.load(real)
    left = m.find(real) == NONE
    assert 3 <= left.sum() == m.left < 60
    try:
        ver.keys_load(crowd)
        ver.keys_load(real)
        assert ver.get_option("keys_index_live") == 1 and ver.get_option("keys_index_left_out") == m.left
        assert np.array_equal(ver.keys_find(real) == NONE, left)
        who = np.arange(480) % 120
        sig, dig = signed_items(rng, priv[who])
        pub = np.ascontiguousarray(real[who])
        want = O.verify_digests(pub, sig, dig, threads=8)
        mm = int(left[who].sum())
        assert want[left[who]].sum() >= 6 and (want[left[who]] == 0).sum() >= 1
        both_ways(ver, lambda: dev_digests(ver, pub, sig, dig), want, mm)
    finally:
        ver.set_option("keys_index_split", 0)


# ---------------------------------------------------------------- messages
@pytest.mark.parametrize("keys_wide", [0, 2])
def test_message_batches(ver, keys_wide):
    pub, sig, msgs, ok, _ = load_msg_vectors()
    want = np.array([O.verify_bytes(bytes(pub[i]), msgs[i], bytes(sig[i])) for i in range(len(ok))], np.uint8)
    assert np.array_equal(want, ok)
    keys, key_of = first_seen(pub)
    out = np.zeros(len(keys), bool)
    out[key_of[0]] = True
    out[::3] = True
    is_out = out[key_of]
    assert want[is_out].sum() >= 5 and (want[is_out] == 0).sum() >= 1 and want[~is_out].sum() >= 5
    arena(ver, f"msgs{keys_wide}", keys[~out], keys_wide=keys_wide)
    st = ver.stream_create()
    try:
        for sort_keys in (1, 0):
            ver.set_option("sort_keys", sort_keys)
            for n in SIZES[:4] + [len(ok)]:
                for stream in (None, st):
                    plain = both_ways(ver, lambda: dev_msgs(ver, pub[:n], sig[:n], msgs[:n], stream=stream), want[:n],
                                      int(is_out[:n].sum()))
                    assert set(plain) <= {"pub33", "item_f"}
    finally:
        ver.stream_destroy(st)
        ver.set_option("sort_keys", 1)
        ver.set_option("keys_index_split", 0)


# ---------------------------------------------------------------- pipelined calls
def run_queued(ver, batches, d_bits_of):
    """The batches enqueued back to back on the context stream, no synchronise
    in between; d_bits_of(k, buffers) names call k's bitmap.  The bitmaps read
    back after one synchronise."""
    nw = [(len(b[0]) + 63) // 64 for b in batches]
    with DevBufs(ver) as bufs:
        dev = [[bufs.up(a) for a in b[:3]] for b in batches]
        bits = [bufs.zeros(w * 8) for w in nw]
        for k, (b, d) in enumerate(zip(batches, dev)):
            ver.dev_verify_digests(0, len(b[0]), d[0], d[1], d[2], d_bits_of(k, bits))
        ver.dev_sync()
        out = []
        for k, w in enumerate(nw):
            got = np.zeros(w, np.uint64)
            ver.dev_download(got, bits[k])
            out.append(unpack(got, len(batches[k][0])))
    return out


def test_pipelined_calls_with_different_miss_sets(ver, world):
    arena(ver, "world", world.resident_keys)
    assert ver.get_option("pipeline_dev") == 1
    specs = [(300, [0, 63, 64, 299]), (700, range(64, 128)), (257, [256]), (640, []), (300, [1, 2, 3, 70]),
             (849 - 100, range(0, 90)), (65, [64]), (512, [5, 300])]
    batches = [world.batch(n, at, rot=11 * k) for k, (n, at) in enumerate(specs)]
    try:
        ver.set_option("keys_index_split", BIG)
        c0 = counters(ver)
        got = run_queued(ver, batches, lambda k, bits: bits[k])
        c1 = counters(ver)
        m = [len(set(at)) for _, at in specs]
        assert c1["split_calls"] - c0["split_calls"] == sum(1 for x in m if x)
        assert c1["split_items"] - c0["split_items"] == sum(m)
        assert c1["hit"] - c0["hit"] == len(specs) and c1["miss"] == c0["miss"]
        for k, (g, b) in enumerate(zip(got, batches)):
            bad = np.nonzero(g != b[3])[0]
            assert bad.size == 0, (k, specs[k][0], bad[:10])
    finally:
        ver.set_option("keys_index_split", 0)


def test_two_calls_into_one_bitmap_end_with_the_second_calls_bits(ver, world):
    """The first call's missing items are all valid; the second call is
    all-resident with refused signatures at those positions.  A merge that ran
    after the second call's bitmap write would set them."""
    arena(ver, "world", world.resident_keys)
    n, at = 600, [0, 1, 63, 64, 65, 200, 201, 599]
    ok_miss = world.miss_items[world.want[world.miss_items] == 1]
    bad_hit = world.hit_items[world.want[world.hit_items] == 0]
    rest = world.hit_items[:n]
    pick1, pick2 = rest.copy(), np.roll(rest, 5)
    pick1[at] = ok_miss[:len(at)]
    pick2[at] = bad_hit[:len(at)]
    b1, b2 = ([np.ascontiguousarray(a[p]) for a in (world.pub, world.sig, world.dig)] + [world.want[p]]
              for p in (pick1, pick2))
    assert b1[3][at].all() and not b2[3][at].any() and not world.is_out[pick2].any()
    try:
        ver.set_option("keys_index_split", BIG)
        for _ in range(3):
            c0 = counters(ver)
            got = run_queued(ver, [b1, b2], lambda k, bits: bits[0])
            c1 = counters(ver)
            assert c1["split_calls"] - c0["split_calls"] == 1 and c1["hit"] - c0["hit"] == 2
            bad = np.nonzero(got[0] != b2[3])[0]
            assert bad.size == 0, bad[:10]
    finally:
        ver.set_option("keys_index_split", 0)


# ---------------------------------------------------------------- replace
def test_after_a_replace_the_old_keys_items_split_off_and_the_new_keys_hit(ver):
    rng = np.random.default_rng(0x5B3)
    priv = fresh_privs(rng, 41)
    keys = O.pubkey_batch(priv, threads=8)
    ver.arena_tag = None
    start(ver)
    ver.keys_load(keys[:40])
    ver.keys_replace(np.array([7], np.uint32), keys[40:41])
    assert ver.get_option("keys_index_live") == 1
    who = np.concatenate([np.arange(40), np.arange(40), [40] * 30, [7] * 25])
    who = who[rng.permutation(len(who))]
    sig, dig = signed_items(rng, priv[who])
    pub = np.ascontiguousarray(keys[who])
    want = O.verify_digests(pub, sig, dig, threads=8)
    assert want[who == 7].sum() >= 10 and want[who == 40].sum() >= 10
    try:
        both_ways(ver, lambda: dev_digests(ver, pub, sig, dig), want, int((who == 7).sum()))
        new_only = who != 7                            # the new key's items and the untouched ones: all resident
        got, delta, routes = moved(ver, lambda: dev_digests(ver, pub[new_only], sig[new_only], dig[new_only]))
        assert delta == {"hit": 1, "miss": 0, "launches": 1, "split_calls": 0, "split_items": 0}
        assert np.array_equal(got, want[new_only])
    finally:
        ver.set_option("keys_index_split", 0)


# ---------------------------------------------------------------- second device slot, budget
def test_second_device_slot(world):
    with gvm.Verifier([0, 0]) as v:
        v.set_option("lat_max", 0)
        start(v)
        v.keys_load(world.resident_keys)
        pub, sig, dig, want = world.batch(500, [0, 63, 64, 65, 300, 499])
        v.set_option("keys_index_split", 6)
        for slot in (1, 0):
            got, delta, routes = moved(v, lambda: dev_digests(v, pub, sig, dig, slot=slot), slot=slot)
            assert_split(delta, routes, 6)
            assert np.array_equal(got, want)


def test_budget_that_holds_the_index_but_not_the_miss_buffers(world):
    """8,192 rows of miss buffers are 1.04 MiB; a budget of the optional tables
    as they stand rounded up to a MiB leaves less than 1 MiB free: the call
    falls through with the right verdicts and no error, and splits once the
    budget is lifted."""
    reps = 7937 // len(world.miss_items) + 1
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1)))
    pub, sig, dig, want = (tile(a) for a in (world.pub, world.sig, world.dig, world.want))
    m = reps * len(world.miss_items)
    assert 7936 < m <= 8192
    with gvm.Verifier([0]) as v:
        v.set_option("lat_max", 0)
        v.set_option("group_keys", 0)
        start(v)
        v.keys_load(world.resident_keys)
        assert v.get_option("keys_index_live") == 1
        v.set_option("keys_index_split", 0)
        plain_bits, _, plain = moved(v, lambda: dev_digests(v, pub, sig, dig))
        assert np.array_equal(plain_bits, want)
        held = v.get_option("hbm_optional_bytes")
        v.set_option("hbm_budget_mb", (held + (1 << 20) - 1) >> 20)
        v.set_option("keys_index_split", BIG)
        got, delta, routes = moved(v, lambda: dev_digests(v, pub, sig, dig))
        assert_fell_through(delta, routes, plain)
        assert np.array_equal(got, want)
        assert v.get_option("hbm_optional_bytes") == held and v.get_option("keys_index_live") == 1
        v.set_option("hbm_budget_mb", 0)
        got, delta, routes = moved(v, lambda: dev_digests(v, pub, sig, dig))
        assert_split(delta, routes, m)
        assert np.array_equal(got, want)
        grown = v.get_option("hbm_optional_bytes") - held
        assert (1 << 20) < grown < (2 << 20)           # 8,192 rows, charged to the budget: not sized by the option
