"""GPU tests of the wide ed25519 key arena (option "ed_keys_wide": radix-2^6 /
radix-2^8 combs of -A beside the radix-16 tables), its readback
gv_ed_keys_wide_point and the device-resident keyed entry point
gv_dev_verify_ed25519_msgs_keyed (include/gpuverify.h).

Expectations come from outside the code under test: oracle/ed25519_ref.py
(verdicts and table entries), hashlib for h = SHA-512(R || A || M) mod L, and
the unkeyed gv_verify_ed25519_msgs over each item's raw key."""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest

import ed_openssl as OSSL
import gpuverify as gvm
from oracle import ed25519_ref as E

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ED_LAT_MAX = 2048                       # the option's default (gv_runtime.cpp)
NW = {4: 64, 6: 43, 8: 32}
NO_SLOT = 8                             # the fixture loads slots 0..7: slot 8 never holds a key
SENTINEL = 0xA5A5A5A5A5A5A5A5


def arr32(keys):
    return np.array([np.frombuffer(k, np.uint8) for k in keys]).reshape(-1, 32)


def sigs(items):
    return np.array([np.frombuffer(s, np.uint8) for s in items]).reshape(-1, 64)


def flip(msg, rng):
    if not msg:
        return b"\x01"
    b = bytearray(msg)
    b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
    return bytes(b)


class World:
    """The 8-key fixture and a pool of items over its slots with their verdicts."""

    def __init__(self):
        g = json.load(open(os.path.join(GOLD, "ed25519_vectors.json")))["categories"]
        self.g = g
        rng = random.Random(0xED8)
        gold_valid = list(dict.fromkeys(bytes.fromhex(v["pub"]) for v in g["valid"]))
        self.seed = {}

        def ossl_key():
            s = rng.randbytes(32)
            p = OSSL.public_key(s)
            self.seed[p] = s
            return p

        rejected = bytes.fromhex(g["pub_not_on_curve"][0]["pub"])
        small = {bytes.fromhex(v["pub"]) for v in g["small_order"]}
        r_id = bytes.fromhex(g["r_identity"][0]["pub"])       # the R' = identity vector's key, when it is a small-order one
        small_key = r_id if r_id in small else sorted(small)[0]
        noncanon = next(bytes.fromhex(v["pub"]) for v in sorted(g["pub_noncanonical"], key=lambda v: not v["ok"])
                        if E.decode_point(bytes.fromhex(v["pub"])) is not None)
        # three ordinary keys, a rejected one, a small-order one, a non-canonical-y one, two more ordinary ones
        self.keys = [gold_valid[0], gold_valid[1], ossl_key(), rejected, small_key, noncanon, gold_valid[2], ossl_key()]
        assert len(set(self.keys)) == 8
        assert E.decode_point(rejected) is None
        assert E.point_mul(8, E.decode_point(small_key)) == E.IDENT
        assert int.from_bytes(noncanon, "little") & ((1 << 255) - 1) >= E.P
        self.pub = arr32(self.keys)
        self.seeded = [i for i, k in enumerate(self.keys) if k in self.seed]
        where = {k: i for i, k in enumerate(self.keys)}

        # the golden rejection classes (and the accepted vectors beside them): on the key's own slot when the
        # fixture holds it, else tiled over the slots
        items = []
        self.classes = ("s_ge_l", "s_eq_l", "s_high_bits", "r_noncanonical", "r_identity", "mixed_order",
                        "valid", "wrong_msg", "bad_r", "bad_s", "small_order", "pub_noncanonical")
        own = {c: 0 for c in self.classes}
        for c in self.classes:
            for v in g[c]:
                pub, msg, sig = (bytes.fromhex(v[k]) for k in ("pub", "msg", "sig"))
                if pub in where:
                    own[c] += 1
                items.append((where.get(pub, len(items) % 8), msg, sig))
        for c in ("s_ge_l", "s_high_bits", "r_noncanonical", "valid"):     # these classes do reach their own keys
            assert own[c] > 0, c
        # 512 random items of the seeded keys: valid, flipped, on another slot
        for i in range(512):
            k = self.seeded[i % len(self.seeded)]
            msg = rng.randbytes(rng.randrange(0, 420))
            sig = OSSL.sign(self.seed[self.keys[k]], msg)
            r = rng.random()
            if r < 0.15:
                b = bytearray(sig)
                b[rng.randrange(64)] ^= 1 << rng.randrange(8)
                sig = bytes(b)
            elif r < 0.3:
                msg = flip(msg, rng)
            elif r < 0.45:
                k = rng.randrange(8)
            items.append((k, msg, sig))
        # items that name slot 8 (valid signatures of a loaded key)
        for i in range(24):
            items.append((NO_SLOT, items[-1 - 3 * i][1], items[-1 - 3 * i][2]))
        order = list(range(len(items)))
        rng.shuffle(order)
        self.items = [items[i] for i in order]
        self.want = np.array([s < 8 and E.verify(self.keys[s], m, sg) for s, m, sg in self.items])
        assert 0.2 < self.want.mean() < 0.8

    def batch(self, n):
        """n items: the pool tiled (slots u32, sig, msgs, verdicts)."""
        idx = [i % len(self.items) for i in range(n)]
        return (np.array([self.items[i][0] for i in idx], np.uint32), sigs([self.items[i][2] for i in idx]),
                [self.items[i][1] for i in idx], self.want[idx])


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture(scope="module")
def vers(world):
    """One context per ed_keys_wide value with the fixture loaded from slot 0."""
    out = {}
    for rb in (0, 6, 8):
        v = gvm.Verifier([0])
        v.set_option("ed_keys_wide", rb)
        assert list(v.ed_keys_load(world.pub)) == list(range(8))
        assert v.get_option("ed_keys_wide") == rb
        assert v.get_option("ed_kw_rb") == rb and v.get_option("ed_kw_keys") == (8 if rb else 0)
        out[rb] = v
    yield out
    for v in out.values():
        v.close()


class DevBatch:
    """A batch in device memory of one device slot and its bitmap (one guard word behind it)."""

    def __init__(self, v, slots, sig, msgs, dslot=0):
        blob, off, ln = gvm.pack_msgs(msgs)
        self.v, self.n, self.dslot = v, len(slots), dslot
        self.words = (self.n + 63) // 64
        self.ptr = []
        for a in (np.ascontiguousarray(slots, np.uint32), np.ascontiguousarray(sig, np.uint8), blob, off, ln):
            p = v.dev_alloc(max(a.nbytes, 16) + 16, dslot)
            v.dev_upload(p, a, dslot)
            self.ptr.append(p)
        self.d_bits = v.dev_alloc(8 * (self.words + 1), dslot)

    def enqueue(self, stream=None, ptr=None, n=None):
        self.v.dev_upload(self.d_bits, np.full(self.words + 1, SENTINEL, np.uint64), self.dslot)
        p = ptr or self.ptr
        return self.v._L.gv_dev_verify_ed25519_msgs_keyed(
            self.v._ctx, self.dslot, self.n if n is None else n, *[ctypes.c_void_p(x) for x in p],
            ctypes.c_void_p(self.d_bits), ctypes.c_void_p(stream or 0))

    def words_back(self, stream=None):
        if stream:
            self.v.stream_sync(stream, self.dslot)
        else:
            self.v.dev_sync(self.dslot)
        w = np.zeros(self.words + 1, np.uint64)
        self.v.dev_download(w, self.d_bits, self.dslot)
        return w

    def bits(self, stream=None):
        w = self.words_back(stream)
        assert w[-1] == SENTINEL, "wrote past ceil(n / 64) words"
        b = np.unpackbits(w[:-1].view(np.uint8), bitorder="little")
        assert not b[self.n:].any(), "unused high bits of the last word"
        return b[:self.n].astype(bool)

    def run(self, stream=None):
        assert self.enqueue(stream) == gvm.GV_OK
        return self.bits(stream)

    def free(self):
        for p in self.ptr + [self.d_bits]:
            self.v.dev_free(p, self.dslot)


def host_keyed(v, slots, sig, msgs, lat_max=ED_LAT_MAX):
    v.set_option("ed_lat_max", lat_max)
    try:
        return v.verify_batch_ed25519_keyed(slots, sig, msgs).astype(bool)
    finally:
        v.set_option("ed_lat_max", ED_LAT_MAX)


def dev_keyed(v, slots, sig, msgs, lat_max=ED_LAT_MAX, stream=None, dslot=0):
    b = DevBatch(v, slots, sig, msgs, dslot)
    v.set_option("ed_lat_max", lat_max)
    try:
        return b.run(stream)
    finally:
        v.set_option("ed_lat_max", ED_LAT_MAX)
        b.free()


def wide_points(rb):
    nw, ne = NW[rb], 1 << (rb - 1)
    return [(w, j) for w in (0, 1, nw - 2, nw - 1) for j in (1, 2, ne - 1, ne)]


# ------------------------------------------------------------------ 1. tables
@pytest.mark.parametrize("rb", [6, 8])
def test_wide_tables_equal_the_oracle(vers, world, rb):
    v = vers[rb]
    nw, ne = NW[rb], 1 << (rb - 1)
    sl = np.arange(9, dtype=np.uint32)                       # slot 8 is not loaded
    neg = [None if E.decode_point(k) is None else E.point_neg(E.decode_point(k)) for k in world.keys]
    for w, j in wide_points(rb):
        enc, ok = v.ed_keys_wide_point(sl, w, j)
        for s in range(8):
            if neg[s] is None:
                assert ok[s] == 0 and not enc[s].any(), (s, w, j)
            else:
                assert ok[s] == 1 and bytes(enc[s]) == E.encode_point(E.point_mul(j << (rb * w), neg[s])), (s, w, j)
        assert ok[8] == 0 and not enc[8].any()
    L, ctx = v._L, v._ctx
    one, enc, ok = np.zeros(1, np.uint32), np.zeros((1, 32), np.uint8), np.zeros(1, np.uint8)
    p = [x.ctypes.data_as(ctypes.c_void_p) for x in (one, enc, ok)]
    for w, j in ((nw, 1), (0, 0), (0, ne + 1)):
        assert L.gv_ed_keys_wide_point(ctx, 1, p[0], w, j, p[1], p[2]) == gvm.GV_EINVAL, (w, j)
    assert L.gv_ed_keys_wide_point(ctx, 1, p[0], nw - 1, ne, p[1], p[2]) == gvm.GV_OK
    # the radix-16 readback is untouched by the wide arena
    e16, p16, ok16 = v.ed_keys_point(sl[:8], 63, 8)
    e0, p0, ok0 = vers[0].ed_keys_point(sl[:8], 63, 8)
    assert np.array_equal(e16, e0) and np.array_equal(p16, world.pub) and np.array_equal(ok16, ok0)


def test_no_wide_arena_without_the_option(vers):
    v = vers[0]
    assert v.get_option("ed_kw_rb") == 0 and v.get_option("ed_kw_keys") == 0
    with pytest.raises(gvm.GpuVerifyError) as e:
        v.ed_keys_wide_point(np.array([0], np.uint32), 0, 1)
    assert e.value.code == gvm.GV_EINVAL


# ------------------------------------------- 2. every digit of every window
def recode(h, rb):
    nw, ne = NW[rb], 1 << (rb - 1)
    out, cin = [], 0
    for w in range(nw):
        d = ((h >> (rb * w)) & ((1 << rb) - 1)) + cin
        cin = 0
        if w < nw - 1 and d >= ne:
            d -= 1 << rb
            cin = 1
        out.append(d)
    assert sum(d << (rb * w) for w, d in enumerate(out)) == h
    return out


@pytest.fixture(scope="module")
def digit_items(world):
    """4,096 valid signatures of one ordinary key, messages of 0..420 bytes, and each item's h."""
    rng = random.Random(0xD161)
    slot = world.seeded[0]
    key = world.keys[slot]
    msgs = [rng.randbytes(rng.randrange(0, 421)) for _ in range(4096)]
    sg = [OSSL.sign(world.seed[key], m) for m in msgs]
    hs = [int.from_bytes(hashlib.sha512(s[:32] + key + m).digest(), "little") % E.L for s, m in zip(sg, msgs)]
    bad = [flip(m, rng) for m in msgs]
    return np.full(4096, slot, np.uint32), sigs(sg), msgs, bad, hs


@pytest.mark.parametrize("rb", [6, 8])
def test_every_digit_of_every_window(vers, digit_items, rb):
    v = vers[rb]
    slots, sg, msgs, bad, hs = digit_items
    nw, ne = NW[rb], 1 << (rb - 1)
    seen = [set() for _ in range(nw)]
    for h in hs:
        for w, d in enumerate(recode(h, rb)):
            seen[w].add(d)
    for w in range(nw - 1):                                  # the reachable digits are all covered
        assert seen[w] == set(range(-ne, ne)), (w, sorted(set(range(-ne, ne)) - seen[w]))
    assert seen[nw - 1] == set(range(17 if rb == 8 else 2)), sorted(seen[nw - 1])
    before = v.get_option("ed_keyed_wide")
    assert host_keyed(v, slots, sg, msgs).all()
    assert v.get_option("ed_keyed_wide") > before
    before = v.get_option("ed_keyed_wide")
    assert dev_keyed(v, slots, sg, msgs).all()
    assert v.get_option("ed_keyed_wide") == before + 1
    assert not host_keyed(v, slots, sg, bad).any()
    assert not dev_keyed(v, slots, sg, bad).any()


# --------------------------------------------- 3. parity of the entry point
@pytest.fixture(scope="module")
def unkeyed(vers, world):
    """gv_verify_ed25519_msgs over each pool item's raw key (slot 8: no key, false)."""
    slots, sg, msgs, want = world.batch(len(world.items))
    raw = np.ascontiguousarray(world.pub[np.minimum(slots, 7)])
    got = vers[0].verify_batch_ed25519(raw, sg, msgs).astype(bool)
    got[slots >= 8] = False
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2049])
@pytest.mark.parametrize("rb", [0, 6, 8])
def test_device_resident_parity(vers, world, unkeyed, rb, n):
    v = vers[rb]
    slots, sg, msgs, want = world.batch(n)
    assert np.array_equal(want, unkeyed[[i % len(world.items) for i in range(n)]])
    b = DevBatch(v, slots, sg, msgs)
    st = v.stream_create()
    wide0 = v.get_option("ed_keyed_wide")
    try:
        for lat_max in (0, ED_LAT_MAX):                      # k_ed_keyed serves every n; the default routing
            v.set_option("ed_lat_max", lat_max)
            host = v.verify_batch_ed25519_keyed(slots, sg, msgs).astype(bool)
            assert np.array_equal(host, want), (lat_max, np.nonzero(host != want)[0][:10])
            for srt in (1, 0):
                for b16 in (1, 0):
                    v.set_option("sort_keys", srt)
                    v.set_option("ed_btab16", b16)
                    for stream in (st, None):
                        got = b.run(stream)
                        bad = np.nonzero(got != want)[0]
                        assert bad.size == 0, (lat_max, srt, b16, bool(stream), bad[:10], slots[bad[:10]])
    finally:
        v.set_option("ed_lat_max", ED_LAT_MAX)
        v.set_option("sort_keys", 1)
        v.set_option("ed_btab16", 1)
        v.stream_destroy(st)
        b.free()
    assert (v.get_option("ed_keyed_wide") > wide0) == (rb != 0)


# ------------------------------------------------------------ 4. validation
def test_validation_leaves_the_bitmap_alone(vers, world):
    v = vers[8]
    slots, sg, msgs, want = world.batch(100)
    b = DevBatch(v, slots, sg, msgs)
    try:
        d_slot, d_sig, d_blob, d_off, d_len = b.ptr
        for what, ptr in (("sig + 8", [d_slot, d_sig + 8, d_blob, d_off, d_len]),
                          ("slot + 2", [d_slot + 2, d_sig, d_blob, d_off, d_len]),
                          ("off null", [d_slot, d_sig, d_blob, 0, d_len]),
                          ("len null", [d_slot, d_sig, d_blob, d_off, 0]),
                          ("slot null", [0, d_sig, d_blob, d_off, d_len]),
                          ("sig null", [d_slot, 0, d_blob, d_off, d_len])):
            assert b.enqueue(ptr=ptr) == gvm.GV_EINVAL, what
            assert (b.words_back() == SENTINEL).all(), what
        L, ctx, vp = v._L, v._ctx, ctypes.c_void_p
        assert L.gv_dev_verify_ed25519_msgs_keyed(ctx, 0, 100, vp(d_slot), vp(d_sig), vp(d_blob), vp(d_off), vp(d_len),
                                                  None, None) == gvm.GV_EINVAL
        assert L.gv_dev_verify_ed25519_msgs_keyed(ctx, 1, 100, vp(d_slot), vp(d_sig), vp(d_blob), vp(d_off), vp(d_len),
                                                  vp(b.d_bits), None) == gvm.GV_ENODEV
        assert b.enqueue(n=0) == gvm.GV_OK                   # n = 0: nothing written
        assert (b.words_back() == SENTINEL).all()
        assert L.gv_dev_verify_ed25519_msgs_keyed(ctx, 0, 0, None, None, None, None, None, None, None) == gvm.GV_OK
        assert np.array_equal(b.run(), want)
    finally:
        b.free()


def test_empty_arena_gives_zero_bits(world):
    with gvm.Verifier([0]) as v:
        v.set_option("ed_keys_wide", 8)
        slots, sg, msgs, want = world.batch(130)
        for lat_max in (ED_LAT_MAX, 0):                      # never loaded: no arena memory at all
            assert not dev_keyed(v, slots, sg, msgs, lat_max).any()
        v.ed_keys_load(world.pub)
        assert np.array_equal(dev_keyed(v, slots, sg, msgs, 0), want)
        v.ed_keys_reset()
        assert v.get_option("ed_kw_keys") == 0 and v.get_option("ed_kw_rb") == 0
        for lat_max in (ED_LAT_MAX, 0):
            assert not dev_keyed(v, slots, sg, msgs, lat_max).any()
            assert not host_keyed(v, slots, sg, msgs, lat_max).any()


# --------------------------------------------------------------- 5. replace
@pytest.mark.parametrize("rb", [6, 8])
def test_replace_rebuilds_the_wide_tables(world, rb):
    rng = random.Random(0x5E + rb)
    rejected = world.keys[3]
    s_new = [rng.randbytes(32) for _ in range(2)]
    p_new = [OSSL.public_key(s) for s in s_new]
    # slot 0: ordinary -> rejected; slot 3: rejected -> ordinary; slot 7: ordinary -> ordinary
    rep = np.array([0, 3, 7], np.uint32)
    new = [rejected, p_new[0], p_new[1]]
    final = list(world.keys)
    for s, k in zip(rep, new):
        final[int(s)] = k
    sl8 = np.arange(8, dtype=np.uint32)
    with gvm.Verifier([0]) as fresh:
        fresh.set_option("ed_keys_wide", rb)
        fresh.ed_keys_load(arr32(final))
        want_pts = {wj: fresh.ed_keys_wide_point(sl8, *wj) for wj in wide_points(rb)}
        want16 = fresh.ed_keys_point(sl8, 63, 8)
    # signatures of the old key of slot 7, and of the new keys of slots 3 and 7
    old7 = world.seed[world.keys[7]]
    msgs = [rng.randbytes(40 + i) for i in range(6)]
    items = [(7, msgs[0], OSSL.sign(old7, msgs[0])), (7, msgs[1], OSSL.sign(old7, msgs[1])),
             (3, msgs[2], OSSL.sign(s_new[0], msgs[2])), (7, msgs[3], OSSL.sign(s_new[1], msgs[3])),
             (0, msgs[4], OSSL.sign(s_new[1], msgs[4])), (2, msgs[5], OSSL.sign(world.seed[world.keys[2]], msgs[5]))]
    n = 16384                                               # past ed_lat_max: k_ed_keyed on the wide tables
    idx = [i % len(items) for i in range(n)]
    slots = np.array([items[i][0] for i in idx], np.uint32)
    sg, ms = sigs([items[i][2] for i in idx]), [items[i][1] for i in idx]
    before = np.array([E.verify(world.keys[s], m, x) for s, m, x in items])[idx]
    after = np.array([E.verify(final[s], m, x) for s, m, x in items])[idx]
    assert list(before[:6]) == [True, True, False, False, False, True]
    assert list(after[:6]) == [False, False, True, True, False, True]
    with gvm.Verifier([0]) as v:
        v.set_option("ed_keys_wide", rb)
        v.ed_keys_load(world.pub)
        b = DevBatch(v, slots, sg, ms)
        st = v.stream_create()
        try:
            assert np.array_equal(b.run(st), before)
            # ordering: a batch enqueued on a caller stream, the replacement at once, no sync between
            assert b.enqueue(st) == gvm.GV_OK
            v.ed_keys_replace(rep, arr32(new))
            assert np.array_equal(b.bits(st), before), "the enqueued batch saw replaced keys"
            assert v.get_option("ed_kw_keys") == 8 and v.get_option("ed_kw_rb") == rb
            for wj, (enc, ok) in want_pts.items():
                got_enc, got_ok = v.ed_keys_wide_point(sl8, *wj)
                assert np.array_equal(got_enc, enc) and np.array_equal(got_ok, ok), wj
            for x, y in zip(v.ed_keys_point(sl8, 63, 8), want16):
                assert np.array_equal(x, y)
            w0 = v.get_option("ed_keyed_wide")
            assert np.array_equal(b.run(st), after)
            assert np.array_equal(b.run(None), after)
            assert v.get_option("ed_keyed_wide") == w0 + 2
            assert np.array_equal(host_keyed(v, slots, sg, ms), after)
            assert np.array_equal(host_keyed(v, slots[:600], sg[:600], ms[:600]), after[:600])       # k_ed_lat_sl
            assert np.array_equal(dev_keyed(v, slots[:600], sg[:600], ms[:600]), after[:600])
        finally:
            v.stream_destroy(st)
            b.free()


# ------------------------------------------------- 6. growth, refusal, reset
@pytest.fixture(scope="module")
def many(world):
    """300 ordinary keys and one signed item per key."""
    rng = random.Random(0x300)
    seeds = [rng.randbytes(32) for _ in range(300)]
    pubs = [OSSL.public_key(s) for s in seeds]
    msgs = [rng.randbytes(rng.randrange(0, 80)) for _ in seeds]
    sg = sigs([OSSL.sign(s, m) for s, m in zip(seeds, msgs)])
    # a third of the items on their neighbour's slot: false
    slots = np.arange(300, dtype=np.uint32)
    slots[::3] = (slots[::3] + 1) % 300
    want = slots == np.arange(300)
    return arr32(pubs), slots, sg, msgs, want


@pytest.mark.parametrize("rb", [6, 8])
def test_growth_moves_the_wide_entries(many, rb):
    pub, slots, sg, msgs, want = many
    nw, ne = NW[rb], 1 << (rb - 1)
    with gvm.Verifier([0]) as v:
        v.set_option("ed_keys_wide", rb)
        v.ed_keys_load(pub[:200])
        assert v.get_option("ed_kw_keys") == 200
        first = np.arange(200, dtype=np.uint32)
        pts = [(0, 1), (nw - 1, 1), (nw // 2, ne)]
        old = [v.ed_keys_wide_point(first, *wj) for wj in pts]
        v.ed_keys_load(pub[200:])                            # past the 256-slot first allocation
        assert v.get_option("ed_kw_keys") == 300 and v.get_option("ed_kw_rb") == rb and v.ed_keys_count == 300
        for wj, (enc, ok) in zip(pts, old):
            got_enc, got_ok = v.ed_keys_wide_point(first, *wj)
            assert np.array_equal(got_enc, enc) and np.array_equal(got_ok, ok) and ok.all(), wj
        a = E.point_neg(E.decode_point(bytes(pub[299])))
        enc, ok = v.ed_keys_wide_point(np.array([299, 300], np.uint32), nw - 1, 1)
        assert ok[0] == 1 and bytes(enc[0]) == E.encode_point(E.point_mul(1 << (rb * (nw - 1)), a))
        assert ok[1] == 0 and not enc[1].any()
        w0 = v.get_option("ed_keyed_wide")
        assert np.array_equal(dev_keyed(v, slots, sg, msgs, 0), want)
        assert np.array_equal(host_keyed(v, slots, sg, msgs, 0), want)
        assert v.get_option("ed_keyed_wide") == w0 + 2


def test_refused_growth_stops_the_wide_tables_until_reset(world, many):
    pub, slots, sg, msgs, want = many
    with gvm.Verifier([0]) as v:
        v.set_option("ed_keys_wide", 8)
        v.set_option("ed_keys_wide_mb", 200)                 # 256 slots of 576 KiB fit in 144 MiB, 512 do not
        assert v.get_option("ed_keys_wide_mb") == 200
        v.ed_keys_load(pub[:200])
        assert v.get_option("ed_kw_keys") == 200 and v.get_option("ed_kw_rb") == 8
        assert list(v.ed_keys_load(pub[200:280])) == list(range(200, 280))     # GV_OK: the growth is refused quietly
        assert v.get_option("ed_kw_keys") == 0 and v.get_option("ed_kw_rb") == 0 and v.ed_keys_count == 280
        with pytest.raises(gvm.GpuVerifyError):
            v.ed_keys_wide_point(np.array([0], np.uint32), 0, 1)
        w0 = v.get_option("ed_keyed_wide")
        sel = slots < 280
        sel &= np.arange(300) < 280
        for fn in (dev_keyed, host_keyed):                   # every slot on its radix-16 table
            assert np.array_equal(fn(v, slots[sel], sg[sel], [m for m, s in zip(msgs, sel) if s], 0), want[sel])
        assert v.get_option("ed_keyed_wide") == w0
        v.ed_keys_load(pub[280:])                            # a further load does not bring them back
        assert v.get_option("ed_kw_keys") == 0 and v.ed_keys_count == 300
        assert np.array_equal(dev_keyed(v, slots, sg, msgs, 0), want)
        assert v.get_option("ed_keyed_wide") == w0
        v.ed_keys_reset()
        v.ed_keys_load(world.pub)                            # from slot 0: the wide tables are back
        assert v.get_option("ed_kw_keys") == 8 and v.get_option("ed_kw_rb") == 8
        bs, bsg, bm, bw = world.batch(300)
        assert np.array_equal(dev_keyed(v, bs, bsg, bm, 0), bw)
        assert v.get_option("ed_keyed_wide") == w0 + 1


def test_option_takes_effect_from_slot_0(world, many):
    pub = many[0]
    with gvm.Verifier([0]) as v:
        L, ctx = v._L, v._ctx
        for bad in (7, 4, -1, 1, 9):
            assert L.gv_set_option(ctx, b"ed_keys_wide", bad) == gvm.GV_EINVAL
        assert L.gv_set_option(ctx, b"ed_keys_wide_mb", -1) == gvm.GV_EINVAL
        assert v.get_option("ed_keys_wide") == 0 and v.get_option("ed_keys_wide_mb") == 0
        v.set_option("ed_keys_wide", 8)
        v.ed_keys_load(world.pub)
        v.set_option("ed_keys_wide", 6)                      # mid-arena: nothing moves
        assert v.get_option("ed_kw_rb") == 8 and v.get_option("ed_kw_keys") == 8
        v.ed_keys_load(pub[:4])
        assert v.get_option("ed_kw_rb") == 8 and v.get_option("ed_kw_keys") == 12
        enc, ok = v.ed_keys_wide_point(np.array([9], np.uint32), 31, 128)      # still the radix-256 comb
        a = E.point_neg(E.decode_point(bytes(pub[1])))
        assert ok[0] == 1 and bytes(enc[0]) == E.encode_point(E.point_mul(128 << 248, a))
        bs, bsg, bm, bw = world.batch(200)
        w0 = v.get_option("ed_keyed_wide")
        assert np.array_equal(dev_keyed(v, bs, bsg, bm, 0), bw)
        assert v.get_option("ed_keyed_wide") == w0 + 1
        v.set_option("ed_keys_wide", 0)                      # 0 takes effect at once: the radix-16 tables serve
        assert np.array_equal(dev_keyed(v, bs, bsg, bm, 0), bw)
        assert v.get_option("ed_keyed_wide") == w0 + 1
        v.set_option("ed_keys_wide", 6)
        v.ed_keys_reset()
        v.ed_keys_load(world.pub)                            # the arena restarts: radix 64 now
        assert v.get_option("ed_kw_rb") == 6 and v.get_option("ed_kw_keys") == 8
        enc, ok = v.ed_keys_wide_point(np.array([1], np.uint32), 42, 1)
        a = E.point_neg(E.decode_point(world.keys[1]))
        assert ok[0] == 1 and bytes(enc[0]) == E.encode_point(E.point_mul(1 << 252, a))
        assert np.array_equal(dev_keyed(v, bs, bsg, bm, 0), bw)
        assert v.get_option("ed_keyed_wide") == w0 + 2


# ------------------------------------------- 7. two device slots of one GPU
@pytest.mark.parametrize("rb", [6, 8])
def test_two_device_slots(world, rb):
    rng = random.Random(0x2D + rb)
    seed = rng.randbytes(32)
    newkey = OSSL.public_key(seed)
    slots, sg, msgs, want = world.batch(2300)
    msg = b"a replaced slot on both device slots"
    s2, g2, m2 = np.array([5, 5, 2], np.uint32), sigs([OSSL.sign(seed, msg)] * 3), [msg, msg + b".", msg]
    with gvm.Verifier([0, 0]) as v:
        assert v.num_devices == 2
        v.set_option("ed_keys_wide", rb)
        v.ed_keys_load(world.pub)
        for d in (0, 1):
            for lat_max in (0, ED_LAT_MAX):
                assert np.array_equal(dev_keyed(v, slots, sg, msgs, lat_max, dslot=d), want), (d, lat_max)
            assert not dev_keyed(v, s2, g2, m2, 0, dslot=d).any()
        w0 = v.get_option("ed_keyed_wide")
        v.ed_keys_replace(np.array([5], np.uint32), arr32([newkey]))
        for d in (0, 1):
            st = v.stream_create(d)
            try:
                assert list(dev_keyed(v, s2, g2, m2, 0, stream=st, dslot=d)) == [True, False, False], d
            finally:
                v.stream_destroy(st, d)
        assert v.get_option("ed_keyed_wide") == w0 + 2
        assert list(host_keyed(v, s2, g2, m2, 0)) == [True, False, False]
