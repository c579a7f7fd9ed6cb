"""GPU tests of gv_ed_keys_replace and gv_ed_keys_point (include/gpuverify.h):
after a replacement the slot behaves on every ed25519 keyed route as if the
new key had been loaded into it, and nothing else about the arena moves.

Expectations come from outside the code under test: oracle/ed25519_ref.py for
the items on golden keys or golden signatures (non-canonical y, small order,
keys FromBytes rejects), OpenSSL for the rest, and the unkeyed
gv_verify_ed25519_msgs over each item's effective key."""
import ctypes
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

NK = 300
FIXED = [0, 1, 63, 64, 65, 255, 256, 299]       # wave / block edges of the slots and the last slot
# ed25519 keyed routes: k_ed_lat_sl; k_ed_keyed in slot order and in item order; the raw keys
ROUTES = {
    "lat_sl": {"ed_lat_max": 2048, "sort_keys": 1, "ed_keyed": 1},
    "keyed_sorted": {"ed_lat_max": 0, "sort_keys": 1, "ed_keyed": 1},
    "keyed_unsorted": {"ed_lat_max": 0, "sort_keys": 0, "ed_keyed": 1},
    "raw_keys": {"ed_lat_max": 0, "sort_keys": 1, "ed_keyed": 0},
}
POINTS = [(w, j) for w in (0, 1, 31, 63) for j in (1, 2, 8)]


def arr32(keys):
    return np.array([np.frombuffer(k, np.uint8) for k in keys]).reshape(-1, 32)


def sigs(items):
    return np.array([np.frombuffer(s, np.uint8) for s in items]).reshape(-1, 64)


class World:
    """300 loaded keys (30 of them golden: non-canonical y, small order, keys
    FromBytes rejects), a replacement of 70 slots, 601 items over all slots
    and their verdicts before and after the replacement."""

    def __init__(self):
        g = json.load(open(os.path.join(GOLD, "ed25519_vectors.json")))["categories"]
        self.vec = {}                                 # golden key -> one of its vectors (msg, sig), an accepted one first
        by_cat = {}
        for cat in ("pub_noncanonical", "small_order", "pub_not_on_curve"):
            for v in sorted(g[cat], key=lambda v: not v["ok"]):
                pub = bytes.fromhex(v["pub"])
                if pub not in self.vec:
                    self.vec[pub] = (bytes.fromhex(v["msg"]), bytes.fromhex(v["sig"]))
                    by_cat.setdefault(cat, []).append(pub)
        # the last key of each class is kept for the replacement
        new_gold = {cat: by_cat[cat].pop() for cat in by_cat}
        gold = (by_cat["pub_noncanonical"][:12] + by_cat["small_order"][:8] + by_cat["pub_not_on_curve"][:10])
        assert 24 <= len(gold) <= 30
        self.gold = set(self.vec)
        assert sum(E.decode_point(p) is None for p in gold) >= 5    # rejected keys among the loaded ones

        rng = random.Random(0xED25)
        nrng = np.random.default_rng(0xED26)
        self.seed = {}                                # OpenSSL key -> its seed

        def ossl_key():
            s = rng.randbytes(32)
            p = OSSL.public_key(s)
            self.seed[p] = s
            return p

        keys0 = [ossl_key() for _ in range(NK)]
        for pos, p in zip(nrng.choice(NK, len(gold), replace=False), gold):
            keys0[int(pos)] = p
        self.keys0 = keys0
        rest = np.setdiff1d(np.arange(NK), FIXED)
        self.rep = np.concatenate([FIXED, nrng.choice(rest, 62, replace=False)]).astype(np.uint32)
        nrng.shuffle(self.rep)                        # unsorted
        assert len(self.rep) == 70 and len(set(self.rep.tolist())) == 70 and list(self.rep) != sorted(self.rep)
        untouched = [s for s in range(NK) if s not in set(self.rep.tolist()) and keys0[s] in self.seed]
        self.twin = untouched[len(untouched) // 2]    # a resident key, its slot untouched
        new = [ossl_key() for _ in range(70)]
        self.i_rejected, self.i_noncanon, self.i_small, self.i_twin = 66, 67, 68, 69
        new[66] = new_gold["pub_not_on_curve"]
        new[67] = new_gold["pub_noncanonical"]
        new[68] = new_gold["small_order"]
        new[69] = keys0[self.twin]
        assert E.decode_point(new[66]) is None and E.decode_point(new[67]) is not None
        assert int.from_bytes(new[67], "little") & ((1 << 255) - 1) >= E.P       # y not reduced
        assert E.point_mul(8, E.decode_point(new[68])) == E.IDENT
        self.new = new
        final = list(keys0)
        for s, p in zip(self.rep, new):
            final[int(s)] = p
        self.final = final
        self.pub0, self.new_pub, self.final_pub = arr32(keys0), arr32(new), arr32(final)

        n = 601
        self.slots = (np.arange(n) % NK).astype(np.uint32)
        where = {int(s): k for k, s in enumerate(self.rep)}
        self.on_new, self.on_old = np.zeros(n, bool), np.zeros(n, bool)
        self.msgs, sg, self.from_gold = [], [], []
        for i, s in enumerate(self.slots.tolist()):
            key = keys0[s]
            if s in where:
                if (i // NK) % 2 == 0:
                    key = new[where[s]]
                    self.on_new[i] = True
                else:
                    self.on_old[i] = True
            if key in self.seed:
                msg = rng.randbytes(rng.randrange(0, 200))
                sig = OSSL.sign(self.seed[key], msg)
            else:
                msg, sig = self.vec[key]
            if rng.random() < 0.2:                    # a share has flipped bits
                if rng.random() < 0.5 or not msg:
                    b = bytearray(sig)
                    b[rng.randrange(64)] ^= 1 << rng.randrange(8)
                    sig = bytes(b)
                else:
                    b = bytearray(msg)
                    b[rng.randrange(len(msg))] ^= 1 << rng.randrange(8)
                    msg = bytes(b)
            self.msgs.append(msg)
            sg.append(sig)
            self.from_gold.append(key not in self.seed)
        self.sig = sigs(sg)
        self.before = self.expect(keys0)
        self.after = self.expect(final)
        # the replacement is visible in the verdicts, in both directions
        assert self.after[self.on_new].sum() > 40 and self.before[self.on_new].sum() <= 3
        assert self.before[self.on_old].sum() > 40 and self.after[self.on_old].sum() <= 3
        other = ~(self.on_new | self.on_old)
        assert np.array_equal(self.before[other], self.after[other]) and 0 < self.after[other].mean() < 1

    def verdict(self, pub, msg, sig, from_gold):
        if pub in self.gold or from_gold:
            return E.verify(pub, msg, sig)
        return OSSL.verify(pub, msg, sig)

    def expect(self, keys):
        return np.array([self.verdict(keys[s], m, bytes(sg), fg)
                         for s, m, sg, fg in zip(self.slots.tolist(), self.msgs, self.sig, self.from_gold)])


@pytest.fixture(scope="module")
def world():
    return World()


def on_route(ver, name, slots, sig, msgs):
    for k, v in ROUTES[name].items():
        ver.set_option(k, v)
    try:
        return ver.verify_batch_ed25519_keyed(slots, sig, msgs).astype(bool)
    finally:
        for k, v in ROUTES["lat_sl"].items():
            ver.set_option(k, v)


def check_routes(ver, world, want, what):
    for name in ROUTES:
        got = on_route(ver, name, world.slots, world.sig, world.msgs)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (what, name, bad[:10], world.slots[bad[:10]])


def all_points(ver, n=NK):
    sl = np.arange(n, dtype=np.uint32)
    return {wj: ver.ed_keys_point(sl, *wj) for wj in POINTS}


@pytest.fixture(scope="module")
def loaded_from_scratch(world):
    """ed_keys_point of a second Verifier that loaded the final key list."""
    with gvm.Verifier([0]) as v:
        v.ed_keys_load(world.final_pub)
        return all_points(v)


@pytest.fixture(scope="module", params=[1, 0], ids=["split", "one_lane"])
def replaced(request, world):
    """A Verifier with the 300 keys loaded, checked on every route, and the 70
    slots replaced, by the split key build or by the one-lane kernel."""
    v = gvm.Verifier([0])
    assert list(v.ed_keys_load(world.pub0)) == list(range(NK))
    check_routes(v, world, world.before, "before")
    state = (v.ed_keys_count, v.ed_keys_generation)
    r0 = v.get_option("ed_keys_replaced")
    v.set_option("ed_keys_split", request.param)
    v.ed_keys_replace(world.rep, world.new_pub)
    v.set_option("ed_keys_split", 1)
    assert (v.ed_keys_count, v.ed_keys_generation) == state and state[0] == NK
    assert v.get_option("ed_keys_replaced") == r0 + 70
    yield v
    v.close()


def test_unkeyed_entry_point_agrees_with_the_expectation(replaced, world):
    for keys, want in ((world.pub0, world.before), (world.final_pub, world.after)):
        got = replaced.verify_batch_ed25519(np.ascontiguousarray(keys[world.slots]), world.sig, world.msgs)
        assert np.array_equal(got.astype(bool), want)


def test_replaced_slots_verify_on_every_route(replaced, world):
    check_routes(replaced, world, world.after, "after")


def test_points_equal_a_load_from_scratch(replaced, world, loaded_from_scratch):
    got = all_points(replaced)
    for wj in POINTS:
        for a, b, what in zip(got[wj], loaded_from_scratch[wj], ("enc", "pub", "ok")):
            assert np.array_equal(a, b), (wj, what, np.nonzero((a != b).reshape(NK, -1).any(axis=1))[0][:10])
    enc, pub, ok = got[(0, 1)]
    assert np.array_equal(pub, world.final_pub)
    assert np.array_equal(ok.astype(bool), np.array([E.decode_point(p) is not None for p in world.final]))


def test_points_equal_the_oracle(replaced, world):
    rep = set(world.rep.tolist())
    sample = sorted(rep) + [s for s in range(NK) if s not in rep][::23]
    assert len(sample) >= 80 and any(world.final[s] in world.gold for s in sample)
    got = all_points(replaced)
    for s in sample:
        a = E.decode_point(world.final[s])
        for (w, j) in POINTS:
            enc, pub, ok = (x[s] for x in got[(w, j)])
            assert bytes(pub) == world.final[s]
            if a is None:
                assert ok == 0 and not enc.any(), (s, w, j)
            else:
                want = E.encode_point(E.point_mul(j * 16 ** w, E.point_neg(a)))
                assert ok == 1 and bytes(enc) == want, (s, w, j)


def test_point_past_the_count_and_bad_window(replaced, world):
    enc, pub, ok = replaced.ed_keys_point(np.array([world.twin, NK, NK + 7, 0xFFFFFFFF], np.uint32), 5, 3)
    assert ok[0] == 1 and enc[0].any() and pub[0].any()
    assert not enc[1:].any() and not pub[1:].any() and not ok[1:].any()
    for w, j in ((64, 1), (0, 0), (0, 9)):
        with pytest.raises(gvm.GpuVerifyError):
            replaced.ed_keys_point(np.array([0], np.uint32), w, j)


def test_rejected_then_good_key(replaced, world):
    slot = int(world.rep[world.i_rejected])
    idx = np.nonzero(world.slots == slot)[0]
    for name in ROUTES:
        assert not on_route(replaced, name, world.slots[idx], world.sig[idx], [world.msgs[i] for i in idx]).any()
    rng = random.Random(slot)
    seed = rng.randbytes(32)
    pub = OSSL.public_key(seed)
    r0 = replaced.get_option("ed_keys_replaced")
    replaced.ed_keys_replace(np.array([slot], np.uint32), arr32([pub]))
    try:
        assert replaced.get_option("ed_keys_replaced") == r0 + 1 and replaced.ed_keys_count == NK
        msg = b"a good key in a slot that held a rejected one"
        good, bad = OSSL.sign(seed, msg), OSSL.sign(seed, msg + b".")
        assert OSSL.verify(pub, msg, good) and not OSSL.verify(pub, msg, bad)
        for name in ROUTES:
            got = on_route(replaced, name, np.array([slot, slot], np.uint32), sigs([good, bad]), [msg, msg])
            assert list(got) == [True, False], name
    finally:                                           # the world's final key list again
        replaced.ed_keys_replace(np.array([slot], np.uint32), arr32([world.new[world.i_rejected]]))
    check_routes(replaced, world, world.after, "rejected key back")


def test_validation_changes_nothing(replaced, world):
    v = replaced
    L, ctx = v._L, v._ctx
    state, r0 = (v.ed_keys_count, v.ed_keys_generation), v.get_option("ed_keys_replaced")
    two = np.ascontiguousarray(world.pub0[:2])

    def call(slots, pub=two):
        s = np.array(slots, np.uint32)
        return L.gv_ed_keys_replace(ctx, len(s), s.ctypes.data_as(ctypes.c_void_p),
                                    pub.ctypes.data_as(ctypes.c_void_p))

    def unchanged():
        assert np.array_equal(v.verify_batch_ed25519_keyed(world.slots, world.sig, world.msgs).astype(bool),
                              world.after)
        assert (v.ed_keys_count, v.ed_keys_generation) == state and v.get_option("ed_keys_replaced") == r0

    assert call([5, 5]) == gvm.GV_EINVAL                              # a slot twice
    unchanged()
    assert call([5, v.ed_keys_count]) == gvm.GV_EINVAL                # the first slot that is not loaded
    unchanged()
    s = np.array([5, 6], np.uint32)
    assert L.gv_ed_keys_replace(ctx, 2, None, two.ctypes.data_as(ctypes.c_void_p)) == gvm.GV_EINVAL
    assert L.gv_ed_keys_replace(ctx, 2, s.ctypes.data_as(ctypes.c_void_p), None) == gvm.GV_EINVAL
    unchanged()
    assert L.gv_ed_keys_replace(ctx, 0, None, None) == gvm.GV_OK
    v.ed_keys_replace(np.zeros(0, np.uint32), np.zeros((0, 32), np.uint8))
    unchanged()
    with pytest.raises(gvm.GpuVerifyError):
        v.ed_keys_replace(np.array([5, 5], np.uint32), two)
    unchanged()


@pytest.mark.parametrize("split", [1, 0])
def test_one_slot_all_slots_growth_and_reset(world, loaded_from_scratch, split):
    """A list of one slot; a list of all 300; a load afterwards grows the arena
    and the replaced slots keep their keys; after a reset no slot is loaded."""
    rng = random.Random(0x300 + split)
    with gvm.Verifier([0]) as v:
        v.ed_keys_load(world.pub0)
        gen = v.ed_keys_generation
        v.set_option("ed_keys_split", split)
        one = int(world.rep[3])
        v.ed_keys_replace(np.array([one], np.uint32), world.new_pub[3:4])
        enc, pub, ok = v.ed_keys_point(np.arange(NK, dtype=np.uint32), 31, 8)
        want = world.pub0.copy()
        want[one] = world.new_pub[3]
        assert np.array_equal(pub, want)
        for x, y in zip((enc, pub, ok), loaded_from_scratch[(31, 8)]):
            assert np.array_equal(x[one], y[one])
        untouched = np.setdiff1d(np.arange(NK), world.rep)
        assert np.array_equal(enc[untouched], loaded_from_scratch[(31, 8)][0][untouched])
        perm = np.random.default_rng(split).permutation(NK).astype(np.uint32)
        v.ed_keys_replace(perm, np.ascontiguousarray(world.final_pub[perm]))
        assert v.get_option("ed_keys_replaced") == 1 + NK and v.ed_keys_count == NK and v.ed_keys_generation == gen
        for wj in ((0, 1), (63, 8)):
            for x, y in zip(v.ed_keys_point(np.arange(NK, dtype=np.uint32), *wj), loaded_from_scratch[wj]):
                assert np.array_equal(x, y), wj
        check_routes(v, world, world.after, "all slots")
        # growth: the arena is reallocated and copied, the replaced slots keep their new keys
        more = [rng.randbytes(32) for _ in range(NK)]
        more_pub = [OSSL.public_key(s) for s in more]
        assert list(v.ed_keys_load(arr32(more_pub))) == list(range(NK, 2 * NK))
        assert v.ed_keys_count == 2 * NK
        check_routes(v, world, world.after, "after growth")
        msgs = [rng.randbytes(30) for _ in more]
        sg = sigs([OSSL.sign(s, m) for s, m in zip(more, msgs)])
        for name in ROUTES:
            assert on_route(v, name, np.arange(NK, 2 * NK, dtype=np.uint32), sg, msgs).all(), name
        for x, y in zip(v.ed_keys_point(np.arange(NK, dtype=np.uint32), 1, 2), loaded_from_scratch[(1, 2)]):
            assert np.array_equal(x, y)
        # reset: no slot is loaded, so no slot can be replaced
        v.ed_keys_reset()
        none = v.verify_batch_ed25519_keyed(world.slots, world.sig, world.msgs)
        assert not none.any()
        r0 = v.get_option("ed_keys_replaced")
        for sl in (0, 5, NK - 1):
            with pytest.raises(gvm.GpuVerifyError):
                v.ed_keys_replace(np.array([sl], np.uint32), world.new_pub[:1])
        assert v.get_option("ed_keys_replaced") == r0 and v.ed_keys_count == 0
        assert np.array_equal(v.verify_batch_ed25519_keyed(world.slots, world.sig, world.msgs), none)
        enc, pub, ok = v.ed_keys_point(np.arange(4, dtype=np.uint32))
        assert not enc.any() and not pub.any() and not ok.any()
