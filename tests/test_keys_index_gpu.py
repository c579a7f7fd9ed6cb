"""GPU tests of the key arena's pubkey index (include/gpuverify.h "keys_index",
gv_keys_find, gv_dev_keys_find) and of the pub33 device-resident calls routed
through it.

Expectations come from outside the code under test: the C oracle's verdicts,
the host model of csrc/gv_kidx.h (kidx_model.py) and the load order.  Verdict
bitmaps are compared for equality.  "lat_max" 0 sends every batch, however
small, to the throughput pipeline, the only one the index routes."""
import numpy as np
import pytest

import gpuverify as gvm
from golden_io import load_digest_vectors, load_msg_vectors
from kidx_model import NONE, SEED, Model, homed_keys, load_model
from oracle import oracle as O
from oracle import secp_ref as R

pytestmark = pytest.mark.gpu

ARENA_ROUTES = {"kw", "kw2", "kn", "k4", "k4f"}
ITEM_ROUTES = {"pub33", "item_f"}
SIZES = [1, 63, 64, 65, 255, 256, 257]


# ---------------------------------------------------------------- helpers
def fresh_privs(rng, n):
    privs = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    privs[:, 0] &= 0x7F
    privs[:, 31] |= 1
    return privs


def rand_keys(rng, n):
    """n distinct 33-byte strings with an 02 / 03 prefix (about half of them points)."""
    k = rng.integers(0, 256, (n, 33), dtype=np.uint8)
    k[:, 0] = 2 + (k[:, 0] & 1)
    return k


def signed_items(rng, privs, bad=0.25):
    """One item per row of privs; a share `bad` of the signatures is corrupted
    (high S, or one bit of r or s flipped)."""
    n = privs.shape[0]
    dig = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sig = O.sign_batch(np.ascontiguousarray(privs), dig, threads=8)
    for i in np.nonzero(rng.random(n) < bad)[0]:
        if rng.random() < 0.5:
            s = int.from_bytes(bytes(sig[i, 32:]), "big")
            sig[i, 32:] = np.frombuffer((R.N - s).to_bytes(32, "big"), np.uint8)
        else:
            sig[i, int(rng.integers(0, 64))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    return sig, dig


def first_seen(pub):
    """The distinct keys of pub in first-seen order and each item's index into them."""
    seen, keys, idx = {}, [], np.zeros(len(pub), np.int64)
    for i, k in enumerate(pub):
        b = k.tobytes()
        if b not in seen:
            seen[b] = len(keys)
            keys.append(k)
        idx[i] = seen[b]
    return np.array(keys, np.uint8), idx


def unpack(bits, n):
    return np.unpackbits(bits.view(np.uint8), bitorder="little")[:n]


class DevBufs:
    """Device copies of host arrays on one device slot, freed on exit."""

    def __init__(self, ver, slot=0):
        self.ver, self.slot, self.ptrs = ver, slot, []

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.ver.dev_alloc(max(arr.nbytes, 4), self.slot)
        self.ptrs.append(p)
        if arr.nbytes:
            self.ver.dev_upload(p, arr, self.slot)
        return p

    def zeros(self, nbytes):
        return self.up(np.zeros(nbytes, np.uint8))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for p in self.ptrs:
            self.ver.dev_free(p, self.slot)


def dev_digests(ver, pub, sig, dig, slot=0, stream=None):
    """gv_dev_verify_digests over host arrays: the accept bits, one per item."""
    n = len(pub)
    nw = (n + 63) // 64
    with DevBufs(ver, slot) as b:
        d_bits = b.zeros(nw * 8)
        ver.dev_verify_digests(slot, n, b.up(pub), b.up(sig), b.up(dig), d_bits, stream=stream)
        if stream:
            ver.stream_sync(stream, slot)
        bits = np.zeros(nw, np.uint64)
        ver.dev_download(bits, d_bits, slot)
    return unpack(bits, n)


def dev_msgs(ver, pub, sig, msgs, slot=0, stream=None):
    n = len(pub)
    nw = (n + 63) // 64
    blob, off, ln = gvm.pack_msgs(msgs)
    with DevBufs(ver, slot) as b:
        d_bits = b.zeros(nw * 8)
        ver.dev_verify_msgs(slot, n, b.up(pub), b.up(sig), b.up(blob), b.up(off), b.up(ln), d_bits, stream=stream)
        if stream:
            ver.stream_sync(stream, slot)
        bits = np.zeros(nw, np.uint64)
        ver.dev_download(bits, d_bits, slot)
    return unpack(bits, n)


def dev_find(ver, pub, slot=0, stream=None, misalign=0):
    """gv_dev_keys_find over a host array; misalign: the key bytes start that
    many bytes past an aligned device address."""
    n = len(pub)
    with DevBufs(ver, slot) as b:
        d_pub = b.up(np.concatenate([np.zeros(misalign, np.uint8), np.ascontiguousarray(pub).reshape(-1)]))
        d_out = b.up(np.full(n, 12345, np.uint32))
        ver.dev_keys_find(slot, n, d_pub + misalign, d_out, stream=stream)
        if stream:
            ver.stream_sync(stream, slot)
        out = np.zeros(n, np.uint32)
        ver.dev_download(out, d_out, slot)
    return out


def counters(ver, slot=0):
    c = {k: ver.get_option("keys_index_" + k) for k in ("hit", "miss", "launches")}
    c["routes"] = ver.route_stats(slot)
    return c


def moved(ver, fn, slot=0):
    """fn's result, the hit / miss / launch counters it moved, the routes it took."""
    c0 = counters(ver, slot)
    out = fn()
    c1 = counters(ver, slot)
    routes = {k: c1["routes"][k] - c0["routes"][k] for k in c1["routes"] if c1["routes"][k] != c0["routes"][k]}
    return out, {k: c1[k] - c0[k] for k in ("hit", "miss", "launches")}, routes


def assert_hit(delta, routes):
    assert delta["hit"] == 1 and delta["miss"] == 0 and delta["launches"] == 1, delta
    assert set(routes) <= ARENA_ROUTES and sum(routes.values()) == 1, routes


def assert_fell_through(delta, routes, expect_routes):
    assert delta["hit"] == 0 and delta["miss"] == 1 and delta["launches"] == 1, delta
    assert routes == expect_routes and set(routes) <= ITEM_ROUTES, (routes, expect_routes)


def start(ver, keys_wide=0, seed=None):
    """An empty arena that takes the index from slot 0."""
    ver.keys_reset()
    ver.set_option("keys_wide", keys_wide)
    ver.set_option("keys_index", 1)
    if seed is not None:
        ver.set_option("keys_index_seed", seed)


# ---------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    v.set_option("lat_max", 0)
    assert v.get_option("keys_index") == 0             # the default
    yield v
    v.close()


class Digests:
    """The digest goldens (every rejection class) and 300 random items, a
    quarter with a corrupted signature, in a fixed shuffled order; their keys
    in first-seen order; the C oracle's verdicts."""

    def __init__(self):
        pub, sig, dig, ok, cats = load_digest_vectors()
        assert {"bad_prefix", "x_ge_p", "x_nonresidue", "high_s", "wrong_msg", "valid"} <= set(cats)
        rng = np.random.default_rng(0x1D1)
        privs = fresh_privs(rng, 60)
        kp = O.pubkey_batch(privs, threads=8)
        who = np.arange(300) % 60
        rsig, rdig = signed_items(rng, privs[who])
        perm = rng.permutation(len(ok) + 300)
        self.pub = np.ascontiguousarray(np.concatenate([pub, kp[who]])[perm])
        self.sig = np.ascontiguousarray(np.concatenate([sig, rsig])[perm])
        self.dig = np.ascontiguousarray(np.concatenate([dig, rdig])[perm])
        self.want = O.verify_digests(self.pub, self.sig, self.dig, threads=16)
        golden = np.concatenate([ok, np.zeros(300, np.uint8)])[perm]
        is_golden = (perm < len(ok))
        assert np.array_equal(self.want[is_golden], golden[is_golden])
        assert 200 < self.want[~is_golden].sum() < 260             # the corrupted quarter fails
        self.keys, self.key_of = first_seen(self.pub)
        self.rejected = np.array([cats[p] in ("bad_prefix", "x_ge_p", "x_nonresidue") if p < len(ok) else False
                                  for p in perm])
        assert self.rejected.sum() >= 20


@pytest.fixture(scope="module")
def digests():
    return Digests()


# ---------------------------------------------------------------- find
def test_find_returns_each_keys_load_slot(ver, digests):
    """Loads of 1, 255, 256 and 257 keys in turn, rejected golden keys among
    them: every key is found at the slot its load returned, by the host call
    and by the device call; unknown keys and one-byte variants are not."""
    rng = np.random.default_rng(0x1D2)
    rejected = np.unique(digests.pub[digests.rejected], axis=0)
    pool = np.concatenate([rejected, rand_keys(rng, 769 - len(rejected))])
    pool = pool[rng.permutation(769)]
    assert len({k.tobytes() for k in pool}) == 769
    start(ver)
    assert ver.get_option("keys_index_live") == 1 and np.all(ver.keys_find(pool[:5]) == NONE)   # the empty arena
    lo = 0
    for n in (1, 255, 256, 257):
        slots = ver.keys_load(pool[lo:lo + n])
        assert np.array_equal(slots, np.arange(lo, lo + n))
        lo += n
        assert ver.get_option("keys_index_live") == 1 and ver.get_option("keys_index_keys") == lo
        assert np.array_equal(ver.keys_find(pool[:lo]), np.arange(lo, dtype=np.uint32))
        assert np.all(ver.keys_find(pool[lo:]) == NONE)                # not loaded yet
    assert ver.get_option("keys_index_left_out") == 0
    assert ver.get_option("keys_index_words") >= max(512, 2 * lo)
    for mis in (0, 1, 3):
        assert np.array_equal(dev_find(ver, pool, misalign=mis), np.arange(769, dtype=np.uint32))
    variants = np.repeat(pool[::7], 3, axis=0)
    for i, v in enumerate(variants):
        v[(0, 1, 32)[i % 3]] ^= (1, 0x80, 1)[i % 3]                    # the prefix, the first x byte, the last byte
    unknown = np.concatenate([variants, rand_keys(rng, 100)])
    resident = {k.tobytes() for k in pool}
    unknown = np.array([k for k in unknown if k.tobytes() not in resident])
    assert len(unknown) > 400
    assert np.all(ver.keys_find(unknown) == NONE) and np.all(dev_find(ver, unknown) == NONE)
    st = ver.stream_create()
    try:
        mixed = np.concatenate([pool[500:520], unknown[:20]])
        want = np.concatenate([np.arange(500, 520), np.full(20, NONE)]).astype(np.uint32)
        assert np.array_equal(dev_find(ver, mixed, stream=st), want)
    finally:
        ver.stream_destroy(st)


def test_find_names_the_lower_of_two_slots_with_the_same_bytes(ver):
    rng = np.random.default_rng(0x1D3)
    keys = rand_keys(rng, 300)
    keys[200] = keys[17]
    keys[299] = keys[17]
    start(ver)
    ver.keys_load(keys)
    want = np.arange(300, dtype=np.uint32)
    want[[200, 299]] = 17
    assert np.array_equal(ver.keys_find(keys), want) and np.array_equal(dev_find(ver, keys), want)
    assert ver.get_option("keys_index_left_out") == 0
    # replacing the lower slot hands the name to the next one
    ver.keys_replace(np.array([17], np.uint32), rand_keys(rng, 1))
    assert ver.keys_find(keys[200:201])[0] == 200
    ver.keys_replace(np.array([299, 200], np.uint32), rand_keys(rng, 2))
    assert ver.keys_find(keys[200:201])[0] == NONE


def test_find_validation(ver):
    import ctypes
    start(ver)
    ver.keys_load(rand_keys(np.random.default_rng(0x1D4), 10))
    L, ctx, vp = ver._L, ver._ctx, ctypes.c_void_p
    assert L.gv_keys_find(ctx, 0, None, None) == gvm.GV_OK
    assert L.gv_keys_find(ctx, 2, None, vp(8)) == gvm.GV_EINVAL
    assert L.gv_dev_keys_find(ctx, 0, 0, None, None, None) == gvm.GV_OK
    assert L.gv_dev_keys_find(ctx, 9, 2, vp(256), vp(512), None) == gvm.GV_ENODEV
    with DevBufs(ver) as b:
        d_pub, d_out = b.up(np.zeros(66, np.uint8)), b.up(np.full(4, 777, np.uint32))
        assert L.gv_dev_keys_find(ctx, 0, 2, vp(d_pub), None, None) == gvm.GV_EINVAL
        assert L.gv_dev_keys_find(ctx, 0, 2, None, vp(d_out), None) == gvm.GV_EINVAL
        for mis in (1, 2, 3):
            assert L.gv_dev_keys_find(ctx, 0, 2, vp(d_pub), vp(d_out + mis), None) == gvm.GV_EINVAL
        ver.dev_sync()
        out = np.zeros(4, np.uint32)
        ver.dev_download(out, d_out)
        assert list(out) == [777] * 4                                  # nothing was written
    ver.set_option("keys_index", 0)                                    # off at once: "cannot tell"
    assert ver.get_option("keys_index_live") == 0
    with pytest.raises(gvm.GpuVerifyError) as e:
        ver.keys_find(np.zeros((1, 33), np.uint8))
    assert e.value.code == gvm.GV_EINVAL
    ver.set_option("keys_index", 1)
    with pytest.raises(gvm.GpuVerifyError):                            # the seed is fixed while keys are resident
        ver.set_option("keys_index_seed", 5)


# ---------------------------------------------------------------- fixed seed
def test_fixed_seed_wrap_around_and_probe_bound_match_the_host_model(ver):
    lib = load_model()
    P = lib.kidx_probe_bound()
    start(ver, seed=SEED)
    ver.keys_load(rand_keys(np.random.default_rng(0x1D5), 1))
    T = ver.get_option("keys_index_words")                             # the arena's table (its capacity is kept)
    start(ver, seed=SEED)
    wrap = homed_keys(lib, T, T - 1, 3, stream=21)
    crowd = homed_keys(lib, T, 1000, P + 6, stream=22)
    keys = np.concatenate([wrap, crowd])
    m = Model(lib, T, cap=len(keys))
    m.load(keys)
    assert m.left == 6 and list(m.find(wrap)) == [0, 1, 2] and list(m.table[[T - 1, 0, 1]]) == [0, 1, 2]
    ver.keys_load(keys)
    assert ver.get_option("keys_index_live") == 1 and ver.get_option("keys_index_keys") == len(keys)
    assert ver.get_option("keys_index_left_out") == m.left             # exactly the model's count
    assert list(ver.keys_find(wrap)) == [0, 1, 2]                      # home word T - 1: the probe wrapped
    got = ver.keys_find(crowd)
    placed = got != NONE
    assert placed.sum() == P                                           # which ones: the launch's order
    assert np.array_equal(got[placed], 3 + np.nonzero(placed)[0])
    assert np.all(ver.keys_find(rand_keys(np.random.default_rng(0x1D6), 200)) == NONE)
    # a batch on a placed key is routed; one that names a left-out key falls through
    rng = np.random.default_rng(0x1D7)
    sig = rng.integers(0, 256, (40, 64), dtype=np.uint8)
    dig = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    pub_in = np.ascontiguousarray(np.repeat(crowd[placed][:1], 40, axis=0))
    pub_in[::3] = wrap[1]
    ver.set_option("keys_index", 0)
    plain, _, plain_routes = moved(ver, lambda: dev_digests(ver, pub_in, sig, dig))
    ver.set_option("keys_index", 1)
    got_v, delta, routes = moved(ver, lambda: dev_digests(ver, pub_in, sig, dig))
    assert_hit(delta, routes)
    want = O.verify_digests(pub_in, sig, dig, threads=4)
    assert np.array_equal(got_v, want) and np.array_equal(plain, want)
    pub_out = pub_in.copy()
    pub_out[7] = crowd[~placed][0]
    got_v, delta, routes = moved(ver, lambda: dev_digests(ver, pub_out, sig, dig))
    assert_fell_through(delta, routes, plain_routes)
    assert np.array_equal(got_v, O.verify_digests(pub_out, sig, dig, threads=4))


# ---------------------------------------------------------------- routing and parity
@pytest.fixture(scope="module")
def plain_routes(ver, digests):
    """What a batch of this size takes with the option off, and its verdicts."""
    ver.set_option("keys_index", 0)
    got, delta, routes = moved(ver, lambda: dev_digests(ver, digests.pub, digests.sig, digests.dig))
    assert delta == {"hit": 0, "miss": 0, "launches": 0} and set(routes) <= ITEM_ROUTES
    assert np.array_equal(got, digests.want)
    return routes


@pytest.mark.parametrize("keys_wide", [0, 2])
def test_all_resident_batch_runs_keyed_with_the_same_bits(ver, digests, plain_routes, keys_wide):
    start(ver, keys_wide=keys_wide)
    slots = ver.keys_load(digests.keys)
    got, delta, routes = moved(ver, lambda: dev_digests(ver, digests.pub, digests.sig, digests.dig))
    assert_hit(delta, routes)
    assert set(routes) <= ({"kw", "kw2"} if keys_wide else {"kn", "k4", "k4f"}), routes
    bad = np.nonzero(got != digests.want)[0]
    assert bad.size == 0, (bad[:10], digests.key_of[bad[:10]])
    # the same slots, named by the caller: the same route and the same bits
    keyed, _, kroutes = moved(ver, lambda: ver.verify_batch_digests_keyed(slots[digests.key_of], digests.sig,
                                                                         digests.dig))
    assert np.array_equal(keyed, got) and set(kroutes) == set(routes)
    ver.set_option("keys_index", 0)
    off, delta, routes = moved(ver, lambda: dev_digests(ver, digests.pub, digests.sig, digests.dig))
    assert delta == {"hit": 0, "miss": 0, "launches": 0} and routes == plain_routes
    assert np.array_equal(off, got)


@pytest.fixture
def loaded(ver, digests):
    """ver with exactly the digest world's keys resident (other tests reset the arena)."""
    start(ver)
    ver.keys_load(digests.keys)
    return ver


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_wave_and_block_edges(loaded, digests, n):
    ver = loaded
    ver.set_option("keys_index", 1)
    pub, sig, dig = digests.pub[:n], digests.sig[:n], digests.dig[:n]
    got, delta, routes = moved(ver, lambda: dev_digests(ver, pub, sig, dig))
    assert_hit(delta, routes)
    assert np.array_equal(got, digests.want[:n])
    ver.set_option("keys_index", 0)
    off, delta, routes = moved(ver, lambda: dev_digests(ver, pub, sig, dig))
    assert delta == {"hit": 0, "miss": 0, "launches": 0} and set(routes) <= ITEM_ROUTES
    assert np.array_equal(off, got)
    ver.set_option("keys_index", 1)


def test_caller_stream(loaded, digests):
    ver = loaded
    ver.set_option("keys_index", 1)
    st = ver.stream_create()
    try:
        for n in (257, len(digests.pub)):
            got, delta, routes = moved(ver, lambda: dev_digests(ver, digests.pub[:n], digests.sig[:n],
                                                                digests.dig[:n], stream=st))
            assert_hit(delta, routes)
            assert np.array_equal(got, digests.want[:n])
    finally:
        ver.stream_destroy(st)


def test_message_batches(ver):
    pub, sig, msgs, ok, _ = load_msg_vectors()
    want = np.array([O.verify_bytes(bytes(pub[i]), msgs[i], bytes(sig[i])) for i in range(len(ok))], np.uint8)
    assert np.array_equal(want, ok) and 0 < want.mean() < 1
    keys, _ = first_seen(pub)
    start(ver)
    ver.keys_load(keys)
    st = ver.stream_create()
    try:
        for n in SIZES[:4] + [len(ok)]:
            for stream in (None, st):
                got, delta, routes = moved(ver, lambda: dev_msgs(ver, pub[:n], sig[:n], msgs[:n], stream=stream))
                assert_hit(delta, routes)
                assert np.array_equal(got, want[:n])
        ver.set_option("keys_index", 0)
        off, delta, routes = moved(ver, lambda: dev_msgs(ver, pub, sig, msgs))
        assert delta == {"hit": 0, "miss": 0, "launches": 0} and set(routes) <= ITEM_ROUTES
        assert np.array_equal(off, want)
        ver.set_option("keys_index", 1)
        # one key that is not resident: the batch falls through, same verdicts
        pub2 = pub.copy()
        pub2[5, 32] ^= 1
        want2 = np.array([O.verify_bytes(bytes(pub2[i]), msgs[i], bytes(sig[i])) for i in range(len(ok))], np.uint8)
        got, delta, r2 = moved(ver, lambda: dev_msgs(ver, pub2, sig, msgs))
        assert_fell_through(delta, r2, routes)
        assert np.array_equal(got, want2)
    finally:
        ver.stream_destroy(st)


def test_one_key_not_resident_falls_through(loaded, digests, plain_routes):
    ver = loaded
    ver.set_option("keys_index", 1)
    rng = np.random.default_rng(0x1D8)
    priv = fresh_privs(rng, 1)
    sig1, dig1 = signed_items(rng, priv, bad=0)
    pub, sig, dig = digests.pub.copy(), digests.sig.copy(), digests.dig.copy()
    i = 400
    pub[i], sig[i], dig[i] = O.pubkey_batch(priv, threads=1)[0], sig1[0], dig1[0]
    want = digests.want.copy()
    want[i] = 1
    assert np.array_equal(O.verify_digests(pub, sig, dig, threads=16), want)
    got, delta, routes = moved(ver, lambda: dev_digests(ver, pub, sig, dig))
    assert_fell_through(delta, routes, plain_routes)
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- replace
def test_replace_moves_the_bytes_the_index_knows(ver):
    rng = np.random.default_rng(0x1D9)
    nk, nr = 300, 40
    priv0, priv1 = fresh_privs(rng, nk), fresh_privs(rng, nr)
    pub0, pub1 = O.pubkey_batch(priv0, threads=8), O.pubkey_batch(priv1, threads=8)
    pub1[0, 0] = 0x05                                                  # a key ParsePubKey rejects goes in too
    rep = rng.choice(nk, nr, replace=False).astype(np.uint32)
    start(ver)
    ver.keys_load(pub0)
    r0 = ver.get_option("keys_replaced")
    ver.keys_replace(rep, pub1)
    assert ver.get_option("keys_replaced") - r0 == nr and ver.get_option("keys_index_live") == 1
    assert ver.get_option("keys_index_keys") == nk and ver.get_option("keys_index_left_out") == 0
    want = np.arange(nk, dtype=np.uint32)
    want[rep] = NONE
    assert np.array_equal(ver.keys_find(pub0), want)                   # the old bytes are gone
    assert np.array_equal(ver.keys_find(pub1), rep)                    # the new ones sit in the replaced slots
    assert np.array_equal(dev_find(ver, pub1), rep)
    # a batch on the new keys and untouched ones is routed ...
    final_priv = priv0.copy()
    final_priv[rep] = priv1
    final_pub = pub0.copy()
    final_pub[rep] = pub1
    who = np.concatenate([rep, rng.choice(np.setdiff1d(np.arange(nk), rep), 160)]).astype(np.int64)
    sig, dig = signed_items(rng, final_priv[who])
    pub = np.ascontiguousarray(final_pub[who])
    want_v = O.verify_digests(pub, sig, dig, threads=8)
    assert want_v[0] == 0 and 20 <= want_v[:nr].sum() and 100 <= want_v[nr:].sum() < 160
    got, delta, routes = moved(ver, lambda: dev_digests(ver, pub, sig, dig))
    assert_hit(delta, routes)
    assert np.array_equal(got, want_v)
    # ... one that still names the old keys falls through, with the old keys' verdicts
    sig, dig = signed_items(rng, priv0[who])
    pub = np.ascontiguousarray(pub0[who])
    want_v = O.verify_digests(pub, sig, dig, threads=8)
    assert want_v[:nr].sum() >= 20
    got, delta, routes = moved(ver, lambda: dev_digests(ver, pub, sig, dig))
    assert delta["miss"] == 1 and delta["hit"] == 0 and set(routes) <= ITEM_ROUTES
    assert np.array_equal(got, want_v)


# ---------------------------------------------------------------- growth, reset, second device
def test_growth_reset_reload_and_second_device_slot():
    rng = np.random.default_rng(0x1DA)
    priv = fresh_privs(rng, 50)
    real = O.pubkey_batch(priv, threads=8)
    bulk = rand_keys(rng, 4400)
    keys = np.concatenate([real, bulk])
    who = np.arange(200) % 50
    sig, dig = signed_items(rng, priv[who])
    pub = np.ascontiguousarray(real[who])
    want = O.verify_digests(pub, sig, dig, threads=8)
    assert 120 < want.sum() < 180
    with gvm.Verifier([0, 0]) as v:
        v.set_option("lat_max", 0)
        v.set_option("keys_k6", 0)                                     # k4 tables only: the loads stay short
        start(v)
        v.keys_load(keys[:300])
        words0 = v.get_option("keys_index_words")
        assert np.array_equal(v.keys_load(keys[300:]), np.arange(300, 4450))   # past 4,096 slots: the arena grows
        assert v.get_option("keys_index_words") > words0
        assert v.get_option("keys_index_live") == 1 and v.get_option("keys_index_keys") == 4450
        assert v.get_option("keys_index_left_out") == 0
        every = np.arange(4450, dtype=np.uint32)
        assert np.array_equal(v.keys_find(keys), every)
        for slot in (0, 1):
            assert np.array_equal(dev_find(v, keys, slot=slot), every)
            got, delta, routes = moved(v, lambda: dev_digests(v, pub, sig, dig, slot=slot), slot=slot)
            assert_hit(delta, routes)
            assert np.array_equal(got, want)
        # reset: everything misses, and an empty arena launches nothing
        v.keys_reset()
        assert v.get_option("keys_index_keys") == 0 and v.get_option("keys_index_live") == 1
        out, delta, routes = moved(v, lambda: v.keys_find(keys[:500]))
        assert np.all(out == NONE) and delta["launches"] == 0
        got, delta, routes = moved(v, lambda: dev_digests(v, pub, sig, dig, slot=1), slot=1)
        assert delta == {"hit": 0, "miss": 0, "launches": 0} and set(routes) <= ITEM_ROUTES
        assert np.array_equal(got, want)
        assert np.all(dev_find(v, keys[:100], slot=1) == NONE)
        # a reload from slot 0, other keys first: found again at their new slots
        order = rng.permutation(350)
        assert np.array_equal(v.keys_load(keys[order]), np.arange(350))
        assert np.array_equal(v.keys_find(keys[order]), np.arange(350, dtype=np.uint32))
        assert np.all(v.keys_find(keys[350:900]) == NONE)              # the earlier arena's keys are gone
        got, delta, routes = moved(v, lambda: dev_digests(v, pub, sig, dig, slot=1), slot=1)
        assert_hit(delta, routes)
        assert np.array_equal(got, want)


# ---------------------------------------------------------------- option off, budget
def test_option_off_and_a_budget_too_small_for_the_index(digests):
    with gvm.Verifier([0]) as v:
        v.set_option("lat_max", 0)
        v.set_option("keys_wide", 0)
        # off from the start: no index, no lookup, "cannot tell"
        v.keys_load(digests.keys)
        assert v.get_option("keys_index_live") == 0 and v.get_option("keys_index_keys") == 0
        with pytest.raises(gvm.GpuVerifyError) as e:
            v.keys_find(digests.keys[:3])
        assert e.value.code == gvm.GV_EINVAL
        got, delta, routes = moved(v, lambda: dev_digests(v, digests.pub, digests.sig, digests.dig))
        assert delta == {"hit": 0, "miss": 0, "launches": 0} and set(routes) <= ITEM_ROUTES
        assert np.array_equal(got, digests.want)
        v.set_option("keys_index", 1)                                  # a running arena keeps what it has: nothing
        assert v.get_option("keys_index_live") == 0
        got, delta, r1 = moved(v, lambda: dev_digests(v, digests.pub, digests.sig, digests.dig))
        assert delta == {"hit": 0, "miss": 0, "launches": 0} and r1 == routes
        assert v.get_option("keys_index_launches") == 0
        # the arena and every G table are allocated: 1 MiB of budget refuses the index alone
        v.keys_reset()
        v.set_option("hbm_budget_mb", 1)
        assert np.array_equal(v.keys_load(digests.keys), np.arange(len(digests.keys)))
        assert v.get_option("keys_index_live") == 0 and v.get_option("keys_index_keys") == 0
        with pytest.raises(gvm.GpuVerifyError):
            v.keys_find(digests.keys[:3])
        got, delta, r2 = moved(v, lambda: dev_digests(v, digests.pub, digests.sig, digests.dig))
        assert delta == {"hit": 0, "miss": 0, "launches": 0} and r2 == routes
        assert np.array_equal(got, digests.want)
        keyed = v.verify_batch_digests_keyed(np.arange(len(digests.keys), dtype=np.uint32)[digests.key_of],
                                             digests.sig, digests.dig)
        assert np.array_equal(keyed, digests.want)
        # the budget lifted and the arena restarted: the index comes back
        v.set_option("hbm_budget_mb", 0)
        v.keys_reset()
        v.keys_load(digests.keys)
        assert v.get_option("keys_index_live") == 1
        got, delta, routes = moved(v, lambda: dev_digests(v, digests.pub, digests.sig, digests.dig))
        assert_hit(delta, routes)
        assert np.array_equal(got, digests.want)


# ---------------------------------------------------------------- find -> keyed verify, chained on one stream
@pytest.mark.parametrize("own_stream", [False, True])
def test_find_output_feeds_the_keyed_call_without_a_host_sync(own_stream):
    """Default "lat_max" / "pipeline_dev", batches past "lat_max_keyed" (the
    pipelined path): find(A), keyed(A), find(B), keyed(B), ... enqueued back
    to back through ONE slot buffer, no synchronise in between.  A and B give
    every item another key, so a keyed call whose front kernels read the
    buffer before its own lookup wrote it sees the other set's (valid) slots
    and gets valid signatures wrong."""
    rng = np.random.default_rng(0x1DB)
    nk, base, reps, rounds = 200, 2000, 10, 3
    n = base * reps
    assert n > gvm.LAT_MAX_KEYED_DEFAULT
    priv = fresh_privs(rng, nk)
    keys = O.pubkey_batch(priv, threads=8)
    who = {"A": np.arange(base) % nk, "B": (np.arange(base) * 7 + 3) % nk}
    assert np.all(who["A"] != who["B"])
    items = {}
    for name, w in who.items():
        sig, dig = signed_items(rng, priv[w])
        pub = np.ascontiguousarray(keys[w])
        want = O.verify_digests(pub, sig, dig, threads=8)
        assert 0.6 < want.mean() < 0.9
        items[name] = [np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))) for a in (pub, sig, dig, want)]
    nw = (n + 63) // 64
    with gvm.Verifier([0]) as v:
        assert v.get_option("pipeline_dev") == 1
        v.set_option("keys_wide", 0)
        v.set_option("keys_index", 1)
        v.keys_load(keys)
        st = v.stream_create() if own_stream else None
        try:
            with DevBufs(v) as b:
                dev = {name: [b.up(a) for a in it[:3]] for name, it in items.items()}
                d_slots = b.up(np.zeros(n, np.uint32))
                order = ["A", "B"] * rounds
                d_bits = [b.zeros(nw * 8) for _ in order]
                r0, l0 = v.route_stats(), v.get_option("keys_index_launches")
                for name, bits in zip(order, d_bits):
                    d_pub, d_sig, d_dig = dev[name]
                    v.dev_keys_find(0, n, d_pub, d_slots, stream=st)
                    v.dev_verify_digests_keyed(0, n, d_slots, d_sig, d_dig, bits, stream=st)
                if st:
                    v.stream_sync(st)
                else:
                    v.dev_sync()
                r1 = v.route_stats()
                assert v.get_option("keys_index_launches") - l0 == len(order)
                assert r1["lat_keyed"] == r0["lat_keyed"]              # the throughput pipeline, not a small-batch kernel
                assert sum(r1[k] - r0[k] for k in ARENA_ROUTES) == len(order)
                for k, (name, bits) in enumerate(zip(order, d_bits)):
                    got = np.zeros(nw, np.uint64)
                    v.dev_download(got, bits)
                    bad = np.nonzero(unpack(got, n) != items[name][3])[0]
                    assert bad.size == 0, (k, name, bad[:10])
        finally:
            if st:
                v.stream_destroy(st)
