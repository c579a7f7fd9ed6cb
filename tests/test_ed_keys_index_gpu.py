"""GPU tests of the ed25519 key arena's pubkey index (option "ed_keys_index"):
gv_ed_keys_find / gv_dev_ed_keys_find, and gv_dev_verify_ed25519_msgs running a
pub32 device batch whose keys are all resident as
gv_dev_verify_ed25519_msgs_keyed would (include/gpuverify.h, DESIGN section
4.3e).

Expectations come from outside the code under test: oracle/ed25519_ref.py
(verdicts, point decoding), tests/ed_openssl.py (signing),
tests/golden/ed25519_vectors.json (every rejection class), the host model
(tests/kidx_model.py at 8-word rows, over tools/fe29/kidx_host.cpp) and the
load order.
Bitmaps are compared for equality."""
import ctypes
import json
import os
import random
from functools import partial

import numpy as np
import pytest

import ed_openssl as OSSL
import gpuverify as gvm
import kidx_model
from kidx_model import SEED, load_model
from oracle import ed25519_ref as E

pytestmark = pytest.mark.gpu
Model = partial(kidx_model.Model, row=8)                 # the ed25519 arena's rows
homed_keys = partial(kidx_model.homed_keys, row=8)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = 0xFFFFFFFF
ED_LAT_MAX = 2048                       # the option's default
ED_GROUP_MIN = 196608                   # the option's default
SENTINEL = 0xA5A5A5A5A5A5A5A5
SIZES = (1, 63, 64, 65, 255, 256, 257, 2048, 2049, 4097)   # wave and block edges, both sides of ed_lat_max


def arr32(keys):
    return np.array([np.frombuffer(k, np.uint8) for k in keys], np.uint8).reshape(-1, 32)


def sigs(items):
    return np.array([np.frombuffer(s, np.uint8) for s in items], np.uint8).reshape(-1, 64)


def flip(b, rng):
    if not b:
        return b"\x01"
    b = bytearray(b)
    b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
    return bytes(b)


def rand_strings(rng, n, avoid=()):
    """n distinct 32-byte strings (bytes, not points: about half decode)."""
    seen, out = set(avoid), []
    while len(out) < n:
        k = rng.randbytes(32)
        if k not in seen:
            seen.add(k)
            out.append(k)
    return out


def one_bit_variants(keys):
    """Per key three neighbours: byte 0 bit 0, byte 31 bit 7 (the sign bit), byte 31 bit 0."""
    out = np.repeat(keys, 3, axis=0)
    out[0::3, 0] ^= 1
    out[1::3, 31] ^= 0x80
    out[2::3, 31] ^= 1
    return out


def signed_items(rng, keys, seeds, who, bad=0.3):
    """(key, msg, sig) per entry of who: signed by the key's seed, `bad` of them
    with a flipped signature or message bit."""
    items = []
    for k in who:
        msg = rng.randbytes(rng.randrange(0, 300))
        sig = OSSL.sign(seeds[keys[k]], msg)
        r = rng.random()
        if r < bad / 2:
            sig = flip(sig, rng)
        elif r < bad:
            msg = flip(msg, rng)
        items.append((keys[k], msg, sig))
    return items


def oracle(items):
    return np.array([E.verify(k, m, s) for k, m, s in items])


class World:
    """The key world of tests/test_ed_keys_wide_gpu.py by key bytes: every key of
    the golden vectors (ordinary ones, keys FromBytes rejects, small-order keys,
    non-canonical-y keys) and 12 OpenSSL keys, in first-seen order -- the load
    order; the golden rejection classes and 500 random items (valid, a flipped
    signature or message, on another key), shuffled; the oracle's verdicts."""

    def __init__(self):
        g = json.load(open(os.path.join(GOLD, "ed25519_vectors.json")))["categories"]
        rng = random.Random(0xED1D)
        self.seeds = {}
        for _ in range(12):
            s = rng.randbytes(32)
            self.seeds[OSSL.public_key(s)] = s
        self.signers = list(self.seeds)
        classes = ("s_ge_l", "s_eq_l", "s_high_bits", "r_noncanonical", "r_identity", "mixed_order", "valid",
                   "wrong_msg", "bad_r", "bad_s", "small_order", "pub_noncanonical", "pub_not_on_curve", "pub_x0_sign")
        items = [tuple(bytes.fromhex(v[k]) for k in ("pub", "msg", "sig")) for c in classes for v in g[c]]
        self.rejected = bytes.fromhex(g["pub_not_on_curve"][0]["pub"])
        self.small = bytes.fromhex(g["small_order"][0]["pub"])
        self.noncanon = next(bytes.fromhex(v["pub"]) for v in sorted(g["pub_noncanonical"], key=lambda v: not v["ok"])
                             if E.decode_point(bytes.fromhex(v["pub"])) is not None)
        self.noncanon_items = [it for it in items if it[0] == self.noncanon]
        assert E.decode_point(self.rejected) is None
        assert E.point_mul(8, E.decode_point(self.small)) == E.IDENT
        assert int.from_bytes(self.noncanon, "little") & ((1 << 255) - 1) >= E.P
        golden_keys = list(dict.fromkeys(it[0] for it in items))
        for i in range(500):
            k, msg, sig = signed_items(rng, self.signers, self.seeds, [i % 12], bad=0.3)[0]
            if rng.random() < 0.2:
                k = rng.choice(self.signers + golden_keys)             # on another key
            items.append((k, msg, sig))
        rng.shuffle(items)
        self.items = items
        self.keys = list(dict.fromkeys(it[0] for it in items))         # first seen: the load order
        assert {self.rejected, self.small, self.noncanon} <= set(self.keys) and set(self.signers) <= set(self.keys)
        assert len(self.keys) <= 200
        self.pub = arr32(self.keys)
        self.slot_of = {k: i for i, k in enumerate(self.keys)}
        self.want = oracle(items)
        assert 0.2 < self.want.mean() < 0.8

    def batch(self, n, only=None):
        """n items: the pool (or its items whose key `only` accepts) tiled."""
        pool = [i for i, it in enumerate(self.items) if only is None or only(it[0])]
        idx = [pool[i % len(pool)] for i in range(n)]
        return [self.items[i] for i in idx], self.want[idx]


@pytest.fixture(scope="module")
def world():
    return World()


class DevBatch:
    """(key, msg, sig) items in device memory of one device slot, their load
    slots when given, and a sentinel-filled bitmap with one guard word."""

    def __init__(self, v, items, slots=None, dslot=0):
        blob, off, ln = gvm.pack_msgs([it[1] for it in items])
        self.v, self.n, self.dslot = v, len(items), dslot
        self.words = (self.n + 63) // 64
        sl = np.zeros(self.n, np.uint32) if slots is None else np.ascontiguousarray(slots, np.uint32)
        self.ptr = []
        for a in (arr32([it[0] for it in items]), sigs([it[2] for it in items]), blob, off, ln, sl):
            p = v.dev_alloc(max(a.nbytes, 16) + 16, dslot)
            v.dev_upload(p, a, dslot)
            self.ptr.append(p)
        self.d_bits = v.dev_alloc(8 * (self.words + 1), dslot)

    def _fill(self):
        self.v.dev_upload(self.d_bits, np.full(self.words + 1, SENTINEL, np.uint64), self.dslot)

    def by_key(self, stream=None):
        self._fill()
        p = self.ptr
        self.v.dev_verify_ed25519(self.dslot, self.n, p[0], p[1], p[2], p[3], p[4], self.d_bits, stream=stream)
        return self

    def by_slot(self, stream=None, d_slots=None, fill=True):
        if fill:
            self._fill()
        p = self.ptr
        self.v.dev_verify_ed25519_keyed(self.dslot, self.n, d_slots or p[5], p[1], p[2], p[3], p[4], self.d_bits,
                                        stream=stream)
        return self

    def bits(self, stream=None):
        if stream:
            self.v.stream_sync(stream, self.dslot)
        else:
            self.v.dev_sync(self.dslot)
        w = np.zeros(self.words + 1, np.uint64)
        self.v.dev_download(w, self.d_bits, self.dslot)
        assert w[-1] == SENTINEL, "wrote past ceil(n / 64) words"
        b = np.unpackbits(w[:-1].view(np.uint8), bitorder="little")
        assert not b[self.n:].any(), "unused high bits of the last word"
        return b[:self.n].astype(bool)

    def free(self):
        for p in self.ptr + [self.d_bits]:
            self.v.dev_free(p, self.dslot)


def dev_find(v, pub, dslot=0, stream=None, misalign=0):
    """gv_dev_ed_keys_find over a host array; misalign: the key bytes start that
    many bytes past an aligned device address."""
    n = len(pub)
    host = np.concatenate([np.zeros(misalign, np.uint8), np.ascontiguousarray(pub, np.uint8).reshape(-1)])
    d_pub, d_out = v.dev_alloc(host.nbytes + 16, dslot), v.dev_alloc(4 * n + 16, dslot)
    try:
        v.dev_upload(d_pub, host, dslot)
        v.dev_upload(d_out, np.full(n, 12345, np.uint32), dslot)
        v.dev_ed_keys_find(dslot, n, d_pub + misalign, d_out, stream=stream)
        if stream:
            v.stream_sync(stream, dslot)
        else:
            v.dev_sync(dslot)
        out = np.zeros(n, np.uint32)
        v.dev_download(out, d_out, dslot)
    finally:
        v.dev_free(d_pub, dslot)
        v.dev_free(d_out, dslot)
    return out


def counters(v, dslot=0):
    c = {k: v.get_option("ed_keys_index_" + k) for k in ("hit", "miss", "launches")}
    c["grouped"] = v.group_stats(dslot)[0]
    c["wide"] = v.get_option("ed_keyed_wide")
    return c


def moved(v, fn, dslot=0):
    """fn's result and the counters it moved."""
    c0 = counters(v, dslot)
    out = fn()
    c1 = counters(v, dslot)
    return out, {k: c1[k] - c0[k] for k in c0}


HIT = {"hit": 1, "miss": 0, "launches": 1, "grouped": 0}
MISS = {"hit": 0, "miss": 1, "launches": 1}
QUIET = {"hit": 0, "miss": 0, "launches": 0}


def has(delta, want):
    return all(delta[k] == x for k, x in want.items())


def run_by_key(v, items, dslot=0, stream=None):
    b = DevBatch(v, items, dslot=dslot)
    try:
        return moved(v, lambda: b.by_key(stream).bits(stream), dslot)
    finally:
        b.free()


def start(v, wide=0, seed=None):
    """An empty ed25519 arena that takes the index from slot 0."""
    v.ed_keys_reset()
    v.set_option("ed_keys_wide", wide)
    v.set_option("ed_keys_index", 1)
    if seed is not None:
        v.set_option("ed_keys_index_seed", seed)


@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    assert v.get_option("ed_keys_index") == 0            # the default
    yield v
    v.close()


# ---------------------------------------------------------------- find
def test_find_returns_each_keys_load_slot(ver, world):
    """Loads of 1, 255, 256 and 257 keys in turn, the world's keys among them:
    every key is found at the slot its load returned, by the host call and by
    the device call; unknown keys and one-bit variants are not."""
    rng = random.Random(0xE1)
    pool = arr32(world.keys + rand_strings(rng, 769 - len(world.keys), world.keys))
    pool = pool[np.random.default_rng(0xE1).permutation(769)]
    start(ver)
    assert ver.get_option("ed_keys_index_live") == 1 and np.all(ver.ed_keys_find(pool[:5]) == NONE)   # the empty arena
    assert ver.get_option("ed_keys_index_launches") == 0
    lo = 0
    for n in (1, 255, 256, 257):
        slots = ver.ed_keys_load(pool[lo:lo + n])
        assert np.array_equal(slots, np.arange(lo, lo + n))
        lo += n
        assert ver.get_option("ed_keys_index_live") == 1 and ver.get_option("ed_keys_index_keys") == lo
        assert np.array_equal(ver.ed_keys_find(pool[:lo]), np.arange(lo, dtype=np.uint32))
        assert np.all(ver.ed_keys_find(pool[lo:]) == NONE)              # not loaded yet
        assert np.array_equal(dev_find(ver, pool[:lo]), np.arange(lo, dtype=np.uint32))
    assert ver.get_option("ed_keys_index_left_out") == 0
    assert ver.get_option("ed_keys_index_words") >= max(512, 2 * lo)
    for mis in (0, 1, 3):
        assert np.array_equal(dev_find(ver, pool, misalign=mis), np.arange(769, dtype=np.uint32))
    resident = {k.tobytes() for k in pool}
    unknown = np.concatenate([one_bit_variants(pool[::5]), arr32(rand_strings(rng, 100))])
    unknown = np.array([k for k in unknown if k.tobytes() not in resident])
    assert len(unknown) > 500
    assert np.all(ver.ed_keys_find(unknown) == NONE)
    for mis in (0, 1, 3):
        assert np.all(dev_find(ver, unknown, misalign=mis) == NONE)
    st = ver.stream_create()
    try:
        mixed = np.concatenate([pool[500:520], unknown[:20]])
        want = np.concatenate([np.arange(500, 520), np.full(20, NONE)]).astype(np.uint32)
        assert np.array_equal(dev_find(ver, mixed, stream=st), want)
        assert np.array_equal(dev_find(ver, pool, stream=st, misalign=3), np.arange(769, dtype=np.uint32))
    finally:
        ver.stream_destroy(st)
    # a key FromBytes rejects is resident like any other
    assert ver.ed_keys_find(arr32([world.rejected]))[0] == [k.tobytes() for k in pool].index(world.rejected)


def test_find_names_the_lower_of_two_slots_with_the_same_bytes(ver):
    rng = random.Random(0xE3)
    keys = arr32(rand_strings(rng, 300))
    keys[200] = keys[17]
    keys[299] = keys[17]
    start(ver)
    ver.ed_keys_load(keys)
    want = np.arange(300, dtype=np.uint32)
    want[[200, 299]] = 17
    assert np.array_equal(ver.ed_keys_find(keys), want) and np.array_equal(dev_find(ver, keys), want)
    assert ver.get_option("ed_keys_index_left_out") == 0
    ver.ed_keys_replace(np.array([17], np.uint32), arr32(rand_strings(rng, 1)))   # the name goes to the next slot
    assert ver.ed_keys_find(keys[200:201])[0] == 200
    ver.ed_keys_replace(np.array([299, 200], np.uint32), arr32(rand_strings(rng, 2)))
    assert ver.ed_keys_find(keys[200:201])[0] == NONE


def test_find_validation(ver):
    start(ver)
    ver.ed_keys_load(arr32(rand_strings(random.Random(0xE4), 10)))
    L, ctx, vp = ver._L, ver._ctx, ctypes.c_void_p
    assert L.gv_ed_keys_find(ctx, 0, None, None) == gvm.GV_OK
    assert L.gv_ed_keys_find(ctx, 2, None, vp(8)) == gvm.GV_EINVAL
    out = np.full(2, 777, np.uint32)
    assert L.gv_ed_keys_find(ctx, 2, None, out.ctypes.data_as(vp)) == gvm.GV_EINVAL and list(out) == [777, 777]
    assert L.gv_ed_keys_find(ctx, 2, np.zeros(64, np.uint8).ctypes.data_as(vp), None) == gvm.GV_EINVAL
    assert L.gv_dev_ed_keys_find(ctx, 0, 0, None, None, None) == gvm.GV_OK
    assert L.gv_dev_ed_keys_find(ctx, 9, 2, vp(256), vp(512), None) == gvm.GV_ENODEV
    assert L.gv_dev_ed_keys_find(ctx, -1, 2, vp(256), vp(512), None) == gvm.GV_ENODEV
    d_pub, d_out = ver.dev_alloc(64), ver.dev_alloc(16)
    try:
        ver.dev_upload(d_pub, np.zeros(64, np.uint8))
        ver.dev_upload(d_out, np.full(4, 777, np.uint32))
        assert L.gv_dev_ed_keys_find(ctx, 0, 2, vp(d_pub), None, None) == gvm.GV_EINVAL
        assert L.gv_dev_ed_keys_find(ctx, 0, 2, None, vp(d_out), None) == gvm.GV_EINVAL
        for mis in (1, 2, 3):
            assert L.gv_dev_ed_keys_find(ctx, 0, 2, vp(d_pub), vp(d_out + mis), None) == gvm.GV_EINVAL
        ver.dev_sync()
        out = np.zeros(4, np.uint32)
        ver.dev_download(out, d_out)
        assert list(out) == [777] * 4                                  # nothing was written
    finally:
        ver.dev_free(d_pub)
        ver.dev_free(d_out)
    ver.set_option("ed_keys_index", 0)                                 # off at once: "cannot tell"
    assert ver.get_option("ed_keys_index_live") == 0
    with pytest.raises(gvm.GpuVerifyError) as e:
        ver.ed_keys_find(np.zeros((1, 32), np.uint8))
    assert e.value.code == gvm.GV_EINVAL
    with pytest.raises(gvm.GpuVerifyError) as e:
        dev_find(ver, np.zeros((1, 32), np.uint8))
    assert e.value.code == gvm.GV_EINVAL
    ver.set_option("ed_keys_index", 1)
    assert ver.get_option("ed_keys_index_live") == 1
    with pytest.raises(gvm.GpuVerifyError):                            # the seed is fixed while keys are resident
        ver.set_option("ed_keys_index_seed", 5)
    for bad in (-1, 2, 6, 8, 256):
        with pytest.raises(gvm.GpuVerifyError):
            ver.set_option("ed_keys_index", bad)
    assert ver.get_option("ed_keys_index") == 1


# ---------------------------------------------------------------- fixed seed
def test_fixed_seed_wrap_around_and_probe_bound_match_the_host_model(ver, world):
    lib = load_model()
    P = lib.edkidx_probe_bound()
    start(ver, seed=SEED)
    ver.ed_keys_load(world.pub[:1])
    T = ver.get_option("ed_keys_index_words")                          # the arena's table (its capacity is kept)
    start(ver, seed=SEED)
    # a signing key whose probe run stays clear of the wrap's and the crowd's words
    probe = Model(lib, T)
    signer = next(k for k in world.signers if 200 <= probe.home(np.frombuffer(k, np.uint8)) < T - 100)
    wrap = homed_keys(lib, T, T - 1, 3, stream=21)
    crowd = homed_keys(lib, T, 100, P + 6, stream=22)
    keys = np.concatenate([wrap, crowd, arr32([signer])])
    m = Model(lib, T, cap=len(keys))
    m.load(keys)
    assert m.left == 6 and list(m.find(wrap)) == [0, 1, 2] and list(m.table[[T - 1, 0, 1]]) == [0, 1, 2]
    ver.ed_keys_load(keys)
    assert ver.get_option("ed_keys_index_live") == 1 and ver.get_option("ed_keys_index_keys") == len(keys)
    assert ver.get_option("ed_keys_index_left_out") == m.left          # exactly the model's count
    assert list(ver.ed_keys_find(wrap)) == [0, 1, 2]                   # home word T - 1: the probe wrapped
    got = ver.ed_keys_find(crowd)
    placed = got != NONE
    assert placed.sum() == P                                           # which ones: the launch's order
    assert np.array_equal(got[placed], 3 + np.nonzero(placed)[0])
    assert ver.ed_keys_find(arr32([signer]))[0] == len(keys) - 1
    assert np.all(ver.ed_keys_find(arr32(rand_strings(random.Random(0xE6), 200))) == NONE)
    # a batch on placed keys is routed; one that names a left-out key falls through
    rng = random.Random(0xE7)
    items = signed_items(rng, [signer], world.seeds, [0] * 40)
    for i in range(0, 40, 3):
        items[i] = (crowd[placed][i % P].tobytes(), items[i][1], items[i][2])
    items[1] = (wrap[1].tobytes(), items[1][1], items[1][2])
    want = oracle(items)
    assert want.any() and not want.all()
    got_v, delta = run_by_key(ver, items)
    assert has(delta, HIT) and np.array_equal(got_v, want)
    items[7] = (crowd[~placed][0].tobytes(), items[7][1], items[7][2])
    want = oracle(items)
    got_v, delta = run_by_key(ver, items)
    assert has(delta, MISS) and np.array_equal(got_v, want)


# ---------------------------------------------------------------- routing and parity
@pytest.fixture(scope="module")
def routed(world):
    """One context per "ed_keys_wide" value with the world loaded from slot 0 and the index on."""
    out = {}
    for wide in (0, 8):
        v = gvm.Verifier([0])
        start(v, wide=wide)
        assert np.array_equal(v.ed_keys_load(world.pub), np.arange(len(world.keys)))
        assert v.get_option("ed_keys_index_live") == 1 and v.get_option("ed_keys_index_left_out") == 0
        assert v.get_option("ed_kw_rb") == wide
        out[wide] = v
    yield out
    for v in out.values():
        v.close()


@pytest.mark.parametrize("wide", [0, 8])
def test_routed_batches_equal_the_oracle_the_keyed_call_and_the_option_off(routed, world, wide):
    v = routed[wide]
    for n in SIZES:
        items, want = world.batch(n)
        slots = np.array([world.slot_of[it[0]] for it in items], np.uint32)
        b = DevBatch(v, items, slots)
        try:
            got, delta = moved(v, lambda: b.by_key().bits())
            assert has(delta, HIT), (n, delta)                         # one hit, one launch, no grouping
            assert delta["wide"] == (1 if wide and n > ED_LAT_MAX else 0), (n, delta)
            assert np.array_equal(got, want), (n, np.nonzero(got != want)[0][:10])
            keyed, delta = moved(v, lambda: b.by_slot().bits())
            assert has(delta, QUIET) and np.array_equal(keyed, got), n
            v.set_option("ed_keys_index", 0)
            try:
                off, delta = moved(v, lambda: b.by_key().bits())
            finally:
                v.set_option("ed_keys_index", 1)
            assert has(delta, QUIET) and delta["wide"] == 0, (n, delta)
            assert np.array_equal(off, got), n
        finally:
            b.free()
    assert v.get_option("ed_keys_index_live") == 1                     # on again over the running arena: it kept its index


def test_caller_stream(routed, world):
    v = routed[0]
    st = v.stream_create()
    try:
        for n in (65, 2049):
            items, want = world.batch(n)
            got, delta = run_by_key(v, items, stream=st)
            assert has(delta, HIT) and np.array_equal(got, want), n
    finally:
        v.stream_destroy(st)


def test_identity_is_the_byte_string_not_the_point(world):
    twin = E.encode_point(E.decode_point(world.noncanon))
    assert twin != world.noncanon and E.decode_point(twin) == E.decode_point(world.noncanon)
    with gvm.Verifier([0]) as v:
        start(v)
        v.ed_keys_load(arr32([world.noncanon, world.rejected]))
        assert list(v.ed_keys_find(arr32([world.noncanon, twin, world.rejected]))) == [0, NONE, 1]
        assert list(dev_find(v, arr32([twin, world.rejected, world.noncanon]))) == [NONE, 1, 0]
        base = (world.noncanon_items * 70)[:70]
        own_want = oracle(base)
        assert own_want.any()
        got, delta = run_by_key(v, base)
        assert has(delta, HIT) and np.array_equal(got, own_want)
        twins = [(twin, m, s) for _, m, s in base]
        got, delta = run_by_key(v, twins)                              # the same point, other bytes: not resident
        assert has(delta, MISS) and np.array_equal(got, oracle(twins))
        on_rejected = [(world.rejected, m, s) for _, m, s in base]
        assert not oracle(on_rejected).any()
        got, delta = run_by_key(v, on_rejected)                        # found, and every item on it is 0
        assert has(delta, HIT) and not got.any()


def test_one_key_not_resident_falls_through(routed, world):
    v = routed[0]
    rng = random.Random(0xE8)
    seed = rng.randbytes(32)
    stranger = OSSL.public_key(seed)
    assert stranger not in world.slot_of
    for n, group_min, grouped in ((300, ED_GROUP_MIN, 0), (4097, 4096, 1)):
        items, want = world.batch(n)
        want = want.copy()
        msg = rng.randbytes(77)
        items[137] = (stranger, msg, OSSL.sign(seed, msg))
        want[137] = E.verify(*items[137])
        assert want[137]
        v.set_option("ed_group_min", group_min)
        try:
            got, delta = run_by_key(v, items)
        finally:
            v.set_option("ed_group_min", ED_GROUP_MIN)
        assert has(delta, MISS) and delta["grouped"] == grouped, (n, delta)   # the per-item / the grouped path
        assert np.array_equal(got, want), n


# ---------------------------------------------------------------- replace
def test_replace_moves_the_bytes_the_index_knows(world):
    rng = random.Random(0xE9)
    filler = rand_strings(rng, 300 - len(world.keys), world.keys)
    keys = world.keys + filler
    new_seeds = {}
    for _ in range(39):
        s = rng.randbytes(32)
        new_seeds[OSSL.public_key(s)] = s
    new_rejected = next(k for k in rand_strings(rng, 64, keys) if E.decode_point(k) is None)
    new_keys = list(new_seeds) + [new_rejected]
    old_slots = [world.slot_of[k] for k in world.signers] + list(range(len(world.keys), len(world.keys) + 28))
    slots = np.array(old_slots, np.uint32)
    old_keys = [keys[s] for s in slots]
    assert len(slots) == 40 and len(set(old_slots)) == 40
    with gvm.Verifier([0]) as v:
        start(v)
        v.ed_keys_load(arr32(keys))
        # 16,384 routed items on a caller stream, then the replacement with no sync in between
        before, want_before = world.batch(16384)
        after = signed_items(rng, new_keys[:12], new_seeds, [i % 12 for i in range(120)])
        after += [(new_rejected, m, s) for _, m, s in after[:8]]
        untouched, want_untouched = world.batch(200, only=lambda k: k not in world.seeds)
        want_after = np.concatenate([oracle(after), want_untouched])
        after += untouched
        assert 0.2 < want_after.mean() < 0.9
        st = v.stream_create()
        b0, b1 = DevBatch(v, before), DevBatch(v, after)
        try:
            c0 = counters(v)
            b0.by_key(st)
            v.ed_keys_replace(slots, arr32(new_keys))
            got = b0.bits(st)
            assert np.array_equal(got, want_before), np.nonzero(got != want_before)[0][:10]   # the old keys' verdicts
            assert counters(v)["hit"] - c0["hit"] == 1
            got, delta = moved(v, lambda: b1.by_key(st).bits(st))
            assert has(delta, HIT) and np.array_equal(got, want_after)                        # the new keys'
        finally:
            b0.free()
            b1.free()
            v.stream_destroy(st)
        assert v.get_option("ed_keys_index_live") == 1 and v.get_option("ed_keys_index_keys") == 300
        assert v.get_option("ed_keys_index_left_out") == 0
        assert np.all(v.ed_keys_find(arr32(old_keys)) == NONE)         # the old bytes are gone
        assert np.array_equal(v.ed_keys_find(arr32(new_keys)), slots)
        assert np.array_equal(dev_find(v, arr32(new_keys)), slots)
        rest = [s for s in range(300) if s not in set(old_slots)]
        assert np.array_equal(v.ed_keys_find(arr32([keys[s] for s in rest])), np.array(rest, np.uint32))
        # a batch on the old keys is no longer resident: it falls through, by its bytes
        old_items, old_want = world.batch(300, only=lambda k: k in world.seeds)
        assert old_want.any()
        got, delta = run_by_key(v, old_items)
        assert has(delta, MISS) and np.array_equal(got, old_want)


# ---------------------------------------------------------------- growth, reset, second device slot
def test_growth_reset_reload_and_second_device_slot(world):
    rng = random.Random(0xEA)
    keys = arr32(world.keys + rand_strings(rng, 500 - len(world.keys), world.keys))
    items, want = world.batch(300)
    with gvm.Verifier([0, 0]) as v:
        start(v)
        v.ed_keys_load(keys[:200])
        w0 = v.get_option("ed_keys_index_words")
        assert w0 >= 512 and v.get_option("ed_keys_index_keys") == 200
        v.ed_keys_load(keys[200:])                                     # the arena and the table grow
        assert v.get_option("ed_keys_index_words") > w0 and v.get_option("ed_keys_index_words") >= 1000
        assert v.get_option("ed_keys_index_live") == 1 and v.get_option("ed_keys_index_keys") == 500
        assert v.get_option("ed_keys_index_left_out") == 0
        assert np.array_equal(v.ed_keys_find(keys), np.arange(500, dtype=np.uint32))
        for dslot in (0, 1):
            assert np.array_equal(dev_find(v, keys, dslot=dslot), np.arange(500, dtype=np.uint32))
            got, delta = run_by_key(v, items, dslot=dslot)
            assert has(delta, HIT) and np.array_equal(got, want), dslot
        v.ed_keys_reset()                                              # everything misses, and nothing launches
        l0 = v.get_option("ed_keys_index_launches")
        assert v.get_option("ed_keys_index_live") == 1 and v.get_option("ed_keys_index_keys") == 0
        assert np.all(v.ed_keys_find(keys) == NONE)
        for dslot in (0, 1):
            assert np.all(dev_find(v, keys, dslot=dslot) == NONE)
        assert v.get_option("ed_keys_index_launches") == l0
        perm = np.random.default_rng(0xEA).permutation(500)
        v.ed_keys_load(keys[perm])                                     # another order: the new slots
        inv = np.argsort(perm).astype(np.uint32)
        assert np.array_equal(v.ed_keys_find(keys), inv)
        for dslot in (0, 1):
            assert np.array_equal(dev_find(v, keys, dslot=dslot), inv)
            got, delta = run_by_key(v, items, dslot=dslot)
            assert has(delta, HIT) and np.array_equal(got, want), dslot


# ---------------------------------------------------------------- off, and a budget that refuses the table
def test_option_off_and_a_budget_too_small_for_the_index(world):
    items, want = world.batch(300)
    slots = np.array([world.slot_of[it[0]] for it in items], np.uint32)
    with gvm.Verifier([0]) as v:
        v.set_option("ed_keys_wide", 6)                                # an optional table, so the budget has a floor
        v.ed_keys_load(world.pub)                                      # off from the start: no index, "cannot tell"
        assert v.get_option("ed_keys_index_live") == 0 and v.get_option("ed_keys_index_keys") == 0
        assert v.get_option("ed_keys_index_words") == 0
        with pytest.raises(gvm.GpuVerifyError) as e:
            v.ed_keys_find(world.pub[:3])
        assert e.value.code == gvm.GV_EINVAL
        got, delta = run_by_key(v, items)
        assert has(delta, QUIET) and np.array_equal(got, want)
        v.set_option("ed_keys_index", 1)                               # a running arena keeps what it has: nothing
        assert v.get_option("ed_keys_index_live") == 0
        with pytest.raises(gvm.GpuVerifyError):
            v.ed_keys_find(world.pub[:3])
        got, delta = run_by_key(v, items)
        assert has(delta, QUIET) and np.array_equal(got, want)
        assert v.get_option("ed_keys_index_launches") == 0
        # a budget that holds what is allocated and not one byte more refuses the table
        held = v.get_option("hbm_optional_bytes")
        assert held >= 1 << 20
        v.ed_keys_reset()
        v.set_option("hbm_budget_mb", held >> 20)
        assert np.array_equal(v.ed_keys_load(world.pub), np.arange(len(world.keys)))     # GV_OK all the same
        assert v.get_option("ed_keys_index_live") == 0 and v.get_option("ed_keys_index_keys") == 0
        with pytest.raises(gvm.GpuVerifyError):
            v.ed_keys_find(world.pub[:3])
        got, delta = run_by_key(v, items)
        assert has(delta, QUIET) and np.array_equal(got, want)
        b = DevBatch(v, items, slots)
        try:
            assert np.array_equal(b.by_slot().bits(), want)
        finally:
            b.free()
        v.set_option("hbm_budget_mb", 0)                               # the budget lifted and the arena restarted
        v.ed_keys_reset()
        v.ed_keys_load(world.pub)
        assert v.get_option("ed_keys_index_live") == 1 and v.get_option("ed_keys_index_keys") == len(world.keys)
        got, delta = run_by_key(v, items)
        assert has(delta, HIT) and np.array_equal(got, want)


# ---------------------------------------------------------------- find -> keyed verify, chained on one stream
@pytest.fixture(scope="module")
def chain_sets():
    """Two sets of 4,000 items over the same 200 keys in which every item has another key."""
    rng = random.Random(0xEB)
    nk, base, reps = 200, 400, 10
    seeds = {}
    for _ in range(nk):
        s = rng.randbytes(32)
        seeds[OSSL.public_key(s)] = s
    keys = list(seeds)
    who = {"A": [i % nk for i in range(base)], "B": [(7 * i + 3) % nk for i in range(base)]}
    assert all(a != b for a, b in zip(who["A"], who["B"]))
    sets = {}
    for name, w in who.items():
        items = signed_items(rng, keys, seeds, w, bad=0.3)
        want = oracle(items)
        assert 0.5 < want.mean() < 0.9
        sets[name] = (items * reps, np.tile(want, reps))
    return keys, sets


@pytest.mark.parametrize("own_stream", [False, True])
def test_find_output_feeds_the_keyed_call_without_a_host_sync(chain_sets, own_stream):
    """find(A), keyed(A), find(B), keyed(B), ... enqueued back to back through
    ONE slot buffer, no synchronise in between: a keyed call that read the
    buffer before its own lookup wrote it would see the other set's (valid)
    slots and get valid signatures wrong."""
    keys, sets = chain_sets
    n = 4000
    assert n > ED_LAT_MAX
    with gvm.Verifier([0]) as v:
        start(v)
        v.ed_keys_load(arr32(keys))
        st = v.stream_create() if own_stream else None
        order = ["A", "B"] * 3
        batches = [DevBatch(v, sets[name][0]) for name in order]
        d_slots = v.dev_alloc(4 * n)
        try:
            for b in batches:
                b._fill()
            v.dev_sync()
            l0 = v.get_option("ed_keys_index_launches")
            for b in batches:                                          # no copy and no sync from here on
                v.dev_ed_keys_find(0, n, b.ptr[0], d_slots, stream=st)
                b.by_slot(st, d_slots=d_slots, fill=False)
            assert v.get_option("ed_keys_index_launches") - l0 == len(order)
            for k, (name, b) in enumerate(zip(order, batches)):
                got = b.bits(st)
                bad = np.nonzero(got != sets[name][1])[0]
                assert bad.size == 0, (k, name, bad[:10])
        finally:
            for b in batches:
                b.free()
            v.dev_free(d_slots)
            if st:
                v.stream_destroy(st)
