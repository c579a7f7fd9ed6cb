"""GPU tests of gv_keys_replace (include/gpuverify.h): after it returns, a
replaced slot behaves on every keyed entry point and schedule as if the new
key had been loaded into it, and nothing else about the arena moves.

Expectations come from outside the code under test: oracle.verify_digests over
each item's effective key, and the pub33 path verify_batch_digests."""
import ctypes

import numpy as np
import pytest

import gpuverify as gvm
from oracle import oracle as O
from oracle import secp_ref as R
from test_gpu_parity import make_random_batch
from test_key_cache import KEYED_PATHS
from test_wide_narrow_gpu import MIB, chain_limits, routes_of

pytestmark = pytest.mark.gpu

FIXED = [0, 1, 63, 64, 255, 256, 257, 511, 512, 599]   # wave / block edges and the last slot
ARENA_STATE = ("kw_arena_qw", "kw_arena_ng")


def fresh_privs(rng, n):
    """n private keys, the recipe of test_gpu_parity.make_random_batch."""
    privs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    privs[:, 0] &= 0x7F
    privs[:, 31] |= 1
    return privs


def sign_items(rng, privs, bad=0.2):
    """One item per row of privs: a random digest signed by it; a share `bad`
    is then spoiled (high S, or one bit of the digest flipped)."""
    n = privs.shape[0]
    dig = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sig = O.sign_batch(np.ascontiguousarray(privs), dig, threads=8)
    for i in np.nonzero(rng.random(n) < bad)[0]:
        if rng.random() < 0.5:
            s = int.from_bytes(bytes(sig[i, 32:]), "big")
            sig[i, 32:] = np.frombuffer((R.N - s).to_bytes(32, "big"), np.uint8)
        else:
            dig[i, int(rng.integers(0, 32))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    return sig, dig


def off_curve_x(rng):
    """An x < p with x^3 + 7 a non-residue: no point of the curve has it."""
    while True:
        x = int.from_bytes(rng.integers(0, 256, size=32, dtype=np.uint8).tobytes(), "big") % R.P
        if pow((x * x * x + 7) % R.P, (R.P - 1) // 2, R.P) == R.P - 1:
            return x


class World:
    """600 loaded keys (a quarter spoiled: some slots hold rejected keys), 37
    replacements, 3,001 items over all 600 slots and their verdicts before and
    after the replacement."""

    def __init__(self):
        seed, nk = 0xE1, 600
        self.pub0 = np.ascontiguousarray(make_random_batch(nk, seed, adversarial=0.25, nkeys=nk)[0])
        priv0 = fresh_privs(np.random.default_rng(seed), nk)          # the same first draw as make_random_batch
        clean = (O.pubkey_batch(priv0, threads=8) == self.pub0).all(axis=1)
        assert 300 < clean.sum() < nk                                 # most keys as derived, some spoiled
        rng = np.random.default_rng(0xE2)
        rest = np.setdiff1d(np.arange(nk), FIXED)
        self.rep = np.concatenate([FIXED, rng.choice(rest, 27, replace=False)]).astype(np.uint32)
        rng.shuffle(self.rep)                                         # unsorted
        assert len(self.rep) == 37 and len(set(self.rep.tolist())) == 37
        untouched = np.setdiff1d(np.nonzero(clean)[0], self.rep)
        twin = int(untouched[len(untouched) // 2])                    # a resident key, its slot untouched
        new_priv = fresh_privs(rng, 37)
        new_priv[36] = priv0[twin]
        self.new_pub = O.pubkey_batch(new_priv, threads=8)
        self.new_pub[34, 0] = 0x05                                    # bad prefix byte (its x is on the curve)
        self.new_pub[35, 1:] = np.frombuffer(off_curve_x(rng).to_bytes(32, "big"), np.uint8)
        assert np.array_equal(self.new_pub[36], self.pub0[twin])
        self.final_pub = self.pub0.copy()
        self.final_pub[self.rep] = self.new_pub
        n = 3001
        self.slots = (np.arange(n) % nk).astype(np.uint32)
        signer = priv0[self.slots].copy()
        where = {int(s): j for j, s in enumerate(self.rep)}
        self.on_new = np.zeros(n, bool)                               # replaced slot, signed by the new key
        self.on_old = np.zeros(n, bool)                               # replaced slot, signed by the old key
        for i, s in enumerate(self.slots):
            if int(s) in where:
                if (i // nk) % 2 == 0:
                    signer[i] = new_priv[where[int(s)]]
                    self.on_new[i] = True
                else:
                    self.on_old[i] = True
        self.sig, self.dig = sign_items(rng, signer)
        self.before = O.verify_digests(np.ascontiguousarray(self.pub0[self.slots]), self.sig, self.dig, threads=16)
        self.after = O.verify_digests(np.ascontiguousarray(self.final_pub[self.slots]), self.sig, self.dig, threads=16)
        # the replacement is visible in the verdicts, in both directions
        assert self.after[self.on_new].sum() > 40 and self.before[self.on_new].sum() <= 3
        assert self.before[self.on_old].sum() > 20 and self.after[self.on_old].sum() <= 3
        other = ~(self.on_new | self.on_old)
        assert np.array_equal(self.before[other], self.after[other]) and 0 < self.after[other].mean() < 1


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    yield v
    v.close()


@pytest.fixture(scope="module")
def loaded_from_scratch(world):
    """keys_point of a second Verifier that loaded the final key list."""
    with gvm.Verifier([0]) as v:
        v.keys_load(world.final_pub)
        return v.keys_point(np.arange(600, dtype=np.uint32))


@pytest.fixture(params=sorted(KEYED_PATHS))
def path(request, ver):
    lat_max, sliced, keys_k6, keys_wide, lat_kw = KEYED_PATHS[request.param]
    ver.set_option("lat_kw", lat_kw)
    ver.set_option("lat_max", lat_max)
    ver.set_option("lat_sliced", sliced)
    ver.set_option("lat_sl_max", 1 << 30)
    ver.set_option("keys_k6", keys_k6)
    ver.set_option("keys_wide", keys_wide)
    yield request.param
    ver.reset_schedule()
    ver.set_option("lat_sliced", 1)
    ver.set_option("keys_k6", 1)
    ver.set_option("keys_wide", 2)
    ver.set_option("lat_kw", 1)


def arena_state(v):
    return (v.keys_count, v.keys_generation()) + tuple(v.get_option(k) for k in ARENA_STATE)


def load_world(v, world):
    v.keys_reset()
    assert np.array_equal(v.keys_load(world.pub0), np.arange(600))


def test_every_schedule(ver, path, world, loaded_from_scratch):
    load_world(ver, world)
    state, r0 = arena_state(ver), ver.get_option("keys_replaced")
    assert np.array_equal(ver.verify_batch_digests_keyed(world.slots, world.sig, world.dig), world.before)
    ver.keys_replace(world.rep, world.new_pub)
    got = ver.verify_batch_digests_keyed(world.slots, world.sig, world.dig)
    bad = np.nonzero(got != world.after)[0]
    assert bad.size == 0, (bad[:10], world.slots[bad[:10]])
    assert np.array_equal(got, ver.verify_batch_digests(world.final_pub[world.slots], world.sig, world.dig))
    xy, ok = ver.keys_point(np.arange(600, dtype=np.uint32))
    assert np.array_equal(ok, loaded_from_scratch[1])
    assert xy.tobytes() == loaded_from_scratch[0].tobytes()
    assert arena_state(ver) == state
    assert ver.get_option("keys_replaced") - r0 == 37


# ---- layouts C and D, and a stopped wide arena (keys_wide_mb as tests/test_wide_narrow_gpu.py)
class BigWorld:
    """6,000 valid keys, 300 of their slots replaced, 15,000 items (past the
    small-batch bound) over all the slots."""

    def __init__(self):
        rng = np.random.default_rng(0xE3)
        nk, n = 6000, 15000
        assert n > gvm.LAT_MAX_KEYED_DEFAULT
        priv0 = fresh_privs(rng, nk)
        self.pub0 = O.pubkey_batch(priv0, threads=16)
        self.rep = rng.choice(nk, 300, replace=False).astype(np.uint32)
        new_priv = fresh_privs(rng, 300)
        self.new_pub = O.pubkey_batch(new_priv, threads=16)
        final_pub = self.pub0.copy()
        final_pub[self.rep] = self.new_pub
        self.slots = (np.arange(n) % nk).astype(np.uint32)
        signer = priv0[self.slots].copy()
        where = np.full(nk, -1)
        where[self.rep] = np.arange(300)
        use_new = (where[self.slots] >= 0) & ((np.arange(n) // nk) % 2 == 0)
        signer[use_new] = new_priv[where[self.slots[use_new]]]
        self.sig, self.dig = sign_items(rng, signer)
        self.pub = np.ascontiguousarray(final_pub[self.slots])
        self.after = O.verify_digests(self.pub, self.sig, self.dig, threads=16)
        assert self.after[use_new].sum() > 200
        old = (where[self.slots] >= 0) & ~use_new
        assert old.sum() > 200 and self.after[old].sum() == 0


@pytest.fixture(scope="module")
def big():
    return BigWorld()


@pytest.mark.parametrize("end", ["C", "D", "none"])
def test_narrow_and_stopped_wide_layouts(ver, big, end):
    key_cap = ver.get_option("key_cap")
    limit = chain_limits(key_cap)["C D none".split().index(end)]
    try:
        ver.keys_reset()
        ver.set_option("keys_wide_mb", limit // MIB)
        ver.keys_load(big.pub0[:3000])
        ver.keys_load(big.pub0[3000:])                                # the growth is refused: the arena moves down
        layout = {"C": (9, 15), "D": (9, 8), "none": (0, 0)}[end]
        assert tuple(ver.get_option(k) for k in ARENA_STATE) == layout
        state = arena_state(ver)
        ver.keys_replace(big.rep, big.new_pub)
        assert arena_state(ver) == state
        got, routes = routes_of(ver, lambda: ver.verify_batch_digests_keyed(big.slots, big.sig, big.dig))
        assert routes.get({"C": "kw", "D": "kw2", "none": "kn"}[end], 0) >= 1, routes
        bad = np.nonzero(got != big.after)[0]
        assert bad.size == 0, (bad[:10], big.slots[bad[:10]])
        assert np.array_equal(got, ver.verify_batch_digests(big.pub, big.sig, big.dig))
    finally:
        ver.set_option("keys_wide_mb", 0)
        ver.keys_reset()


def test_chunk_edges(ver):
    """max_batch 256 (the smallest the option accepts) under 1,100 replaced
    slots: four full chunks and a tail of 76 in the k4, k6 and wide loops; then
    a replacement of one slot."""
    rng = np.random.default_rng(0xE4)
    nk, n = 1300, 3001
    priv = fresh_privs(rng, nk)
    pub = O.pubkey_batch(priv, threads=8)
    rep = rng.choice(nk, 1100, replace=False).astype(np.uint32)
    new_priv = fresh_privs(rng, 1101)
    new_pub = O.pubkey_batch(new_priv, threads=8)
    slots = (np.arange(n) % nk).astype(np.uint32)
    ver.keys_reset()
    ver.keys_load(pub)
    assert ver.get_option("kw_arena_qw") == 11                        # the wide loop runs too
    mb = ver.get_option("max_batch")
    ver.set_option("max_batch", 256)
    try:
        ver.keys_replace(rep, new_pub[:1100])
    finally:
        ver.set_option("max_batch", mb)
    priv[rep] = new_priv[:1100]
    pub[rep] = new_pub[:1100]
    for step in range(2):
        signer = priv[slots].copy()
        stale = rng.random(n) < 0.3                                   # a key that is nowhere in the arena
        signer[stale] = fresh_privs(rng, int(stale.sum()))
        sig, dig = sign_items(rng, signer)
        want = O.verify_digests(np.ascontiguousarray(pub[slots]), sig, dig, threads=16)
        assert 0.3 < want.mean() < 0.7
        assert np.array_equal(ver.verify_batch_digests_keyed(slots, sig, dig), want)
        if step == 0:
            one = np.array([777], np.uint32)
            ver.keys_replace(one, new_pub[1100:])
            priv[777], pub[777] = new_priv[1100], new_pub[1100]


@pytest.fixture(scope="module")
def edge_load():
    """1,300 keys, 3,001 items over their slots (30 % signed by a key that is
    nowhere in the arena) with the oracle's verdicts, and keys_point of a
    second Verifier that loaded the keys at the default max_batch."""
    rng = np.random.default_rng(0xE6)
    nk, n = 1300, 3001
    priv = fresh_privs(rng, nk)
    pub = O.pubkey_batch(priv, threads=8)
    slots = (np.arange(n) % nk).astype(np.uint32)
    signer = priv[slots].copy()
    stale = rng.random(n) < 0.3
    signer[stale] = fresh_privs(rng, int(stale.sum()))
    sig, dig = sign_items(rng, signer)
    item_pub = np.ascontiguousarray(pub[slots])
    want = O.verify_digests(item_pub, sig, dig, threads=16)
    assert 0.3 < want.mean() < 0.7
    with gvm.Verifier([0]) as v:
        assert v.get_option("max_batch") > nk                         # one chunk
        v.keys_load(pub)
        point = v.keys_point(np.arange(nk, dtype=np.uint32))
    return pub, slots, sig, dig, item_pub, want, point


def test_load_chunk_edges(ver, path, edge_load):
    """max_batch 256 under one gv_keys_load of 1,300 keys: five full chunks and
    a tail of 20 in the k4, k6 and wide loops.  The slots then hold what a load
    in one chunk gives them, and serve every keyed schedule."""
    pub, slots, sig, dig, item_pub, want, point = edge_load
    keys_k6, keys_wide = KEYED_PATHS[path][2:4]
    mb = ver.get_option("max_batch")
    ver.keys_reset()
    ver.set_option("keys_k6", 1)                                      # the load builds every table set
    ver.set_option("keys_wide", 2)
    ver.set_option("max_batch", 256)
    try:
        assert np.array_equal(ver.keys_load(pub), np.arange(len(pub)))
    finally:
        ver.set_option("max_batch", mb)
        ver.set_option("keys_k6", keys_k6)
        ver.set_option("keys_wide", keys_wide)
    assert ver.get_option("kw_arena_qw") == 11                        # the wide loop ran too
    xy, ok = ver.keys_point(np.arange(len(pub), dtype=np.uint32))
    assert np.array_equal(ok, point[1])
    assert xy.tobytes() == point[0].tobytes()
    got = ver.verify_batch_digests_keyed(slots, sig, dig)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:10], slots[bad[:10]])
    assert np.array_equal(got, ver.verify_batch_digests(item_pub, sig, dig))


def test_validation_changes_nothing(ver, world):
    load_world(ver, world)
    L, ctx = ver._L, ver._ctx
    state, r0 = arena_state(ver), ver.get_option("keys_replaced")
    two = np.ascontiguousarray(world.new_pub[:2])

    def call(slots, pub=two):
        s = np.array(slots, np.uint32)
        return L.gv_keys_replace(ctx, len(s), s.ctypes.data_as(ctypes.c_void_p), pub.ctypes.data_as(ctypes.c_void_p))

    def unchanged():
        assert np.array_equal(ver.verify_batch_digests_keyed(world.slots, world.sig, world.dig), world.before)
        assert arena_state(ver) == state and ver.get_option("keys_replaced") == r0

    assert call([5, 5]) == gvm.GV_EINVAL                              # a slot twice
    unchanged()
    assert call([5, ver.keys_count]) == gvm.GV_EINVAL                 # the first slot that is not loaded
    unchanged()
    s = np.array([5, 6], np.uint32)
    assert L.gv_keys_replace(ctx, 2, None, two.ctypes.data_as(ctypes.c_void_p)) == gvm.GV_EINVAL
    assert L.gv_keys_replace(ctx, 2, s.ctypes.data_as(ctypes.c_void_p), None) == gvm.GV_EINVAL
    assert L.gv_keys_replace(None, 2, s.ctypes.data_as(ctypes.c_void_p),
                             two.ctypes.data_as(ctypes.c_void_p)) == gvm.GV_EINVAL
    unchanged()
    assert L.gv_keys_replace(ctx, 0, None, None) == gvm.GV_OK
    ver.keys_replace(np.zeros(0, np.uint32), np.zeros((0, 33), np.uint8))
    unchanged()
    with pytest.raises(gvm.GpuVerifyError):
        ver.keys_replace(np.array([5, 5], np.uint32), two)
    unchanged()


def test_loads_around_a_replacement(ver):
    """load, replace, load (and load again past the arena's first 4,096 slots,
    so it regrows and copies): the replaced slots keep their new keys; after
    keys_reset a load starts at slot 0 as before."""
    rng = np.random.default_rng(0xE5)
    priv = fresh_privs(rng, 600 + 3800)
    pub = O.pubkey_batch(priv, threads=16)
    ver.keys_reset()
    assert np.array_equal(ver.keys_load(pub[:300]), np.arange(300))
    rep = rng.choice(300, 10, replace=False).astype(np.uint32)
    new_priv = fresh_privs(rng, 10)
    new_pub = O.pubkey_batch(new_priv, threads=8)
    ver.keys_replace(rep, new_pub)
    assert np.array_equal(ver.keys_load(pub[300:600]), np.arange(300, 600))
    assert np.array_equal(ver.keys_load(pub[600:]), np.arange(600, 4400))
    assert ver.keys_count == 4400
    final_pub = pub.copy()
    final_pub[rep] = new_pub
    n = 3001
    slots = (np.arange(n) % 600).astype(np.uint32)
    slots[-200:] = np.arange(4400 - 200, 4400)
    signer = priv[slots].copy()
    where = np.full(4400, -1)
    where[rep] = np.arange(10)
    use_new = (where[slots] >= 0) & ((np.arange(n) // 600) % 2 == 0)
    signer[use_new] = new_priv[where[slots[use_new]]]
    sig, dig = sign_items(rng, signer)
    want = O.verify_digests(np.ascontiguousarray(final_pub[slots]), sig, dig, threads=16)
    assert want[use_new].sum() >= 15 and want[(where[slots] >= 0) & ~use_new].sum() == 0
    assert np.array_equal(ver.verify_batch_digests_keyed(slots, sig, dig), want)
    ver.keys_reset()
    assert np.array_equal(ver.keys_load(pub[:600]), np.arange(600))
    slots = (np.arange(n) % 600).astype(np.uint32)
    sig, dig = sign_items(rng, priv[slots])
    want = O.verify_digests(np.ascontiguousarray(pub[slots]), sig, dig, threads=16)
    assert np.array_equal(ver.verify_batch_digests_keyed(slots, sig, dig), want)


def test_two_slots_of_one_device(world):
    with gvm.Verifier([0, 0]) as v2:
        load_world(v2, world)
        v2.keys_replace(world.rep, world.new_pub)
        got = v2.verify_batch_digests_keyed(world.slots, world.sig, world.dig)   # split over both arenas
        assert len(v2.last_slices()) == 2 and all(n > 0 for _, n in v2.last_slices())
        assert np.array_equal(got, world.after)
        assert v2.get_option("keys_replaced") == 37


def test_submitted_batch_sees_the_old_keys(ver, world):
    load_world(ver, world)
    pending = ver.submit_digests_keyed(world.slots, world.sig, world.dig)
    ver.keys_replace(world.rep, world.new_pub)                        # waits for the submitted batch first
    assert np.array_equal(ver.wait(pending), world.before)
    pending = ver.submit_digests_keyed(world.slots, world.sig, world.dig)
    assert np.array_equal(ver.wait(pending), world.after)


def test_device_resident_after_a_replacement(ver, world):
    load_world(ver, world)
    ver.keys_replace(world.rep, world.new_pub)
    n = len(world.slots)
    arrays = (world.slots, world.sig, world.dig)
    bufs = [ver.dev_alloc(a.nbytes) for a in arrays]
    d_bits = ver.dev_alloc(((n + 63) // 64) * 8)
    try:
        for p, a in zip(bufs, arrays):
            ver.dev_upload(p, a)
        ver.dev_verify_digests_keyed(0, n, bufs[0], bufs[1], bufs[2], d_bits)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        ver.dev_download(bits, d_bits)
    finally:
        for p in bufs + [d_bits]:
            ver.dev_free(p)
    got = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n]
    assert np.array_equal(got, world.after)
