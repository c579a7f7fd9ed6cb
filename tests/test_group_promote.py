"""The grouped route's layout promotion (gv_set_option "group_promote";
DESIGN section 4.1k): a scratch set whose keys recur rebuilds its key tables
once in the kg layout of the option's NG groups and runs k_ecmult_kn<5, NG>
from then on; a batch of new keys sends it back to k4's layout.  Device calls
on the context stream alternate the two scratch sets, each with its own cache,
history and flag, so every scenario runs in pairs of calls.

Shapes are tests/test_group_reuse.py's: 16,384 items (above lat_max, at
group_min) over 512-1,700 distinct keys, an arena of 3,328 rows.
"group_promote_min" is set to 0 and "group_promote" explicitly, so every case
holds whatever defaults ship.  Verdicts are checked on every call against
construction, and on 2,000-item samples against the C oracle."""
import numpy as np
import pytest

import bench
import gpuverify as gvm
import special_cases as SC
from golden_io import load_digest_vectors
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 16_384
NG = 9                                       # the layout of the cases that are not run per layout
P_BYTES = (2**256 - 2**32 - 977).to_bytes(32, "big")


def key_ids(pub):
    """The set of distinct keys of a batch that k_dedupe gives an id (prefix 02 / 03 and x < p)."""
    rows = {bytes(r) for r in np.unique(pub, axis=0)}
    return {r for r in rows if r[0] in (2, 3) and r[1:] < P_BYTES}


class DevBatch:
    """A batch resident on device 0, with one bitmap per call in flight."""

    def __init__(self, ver, pub, sig, dig, exp, calls=8):
        self.ver, self.n, self.exp = ver, len(exp), exp
        self.U = len(key_ids(pub))
        self.d = [ver.dev_alloc(a.nbytes) for a in (pub, sig, dig)]
        for p, a in zip(self.d, (pub, sig, dig)):
            ver.dev_upload(p, np.ascontiguousarray(a))
        self.words = (self.n + 63) // 64
        self.bits = [ver.dev_alloc(self.words * 8) for _ in range(calls)]

    def run(self, calls=2):
        """`calls` pipelined calls; per call (keys built, keys reused, groups per key), then every bitmap checked."""
        v, out = self.ver, []
        for k in range(calls):
            h0, b0 = v.get_option("group_reuse_hit"), v.get_option("group_reuse_built")
            v.dev_verify_digests(0, self.n, self.d[0], self.d[1], self.d[2], self.bits[k])
            out.append((v.get_option("group_reuse_built") - b0, v.get_option("group_reuse_hit") - h0,
                        v.get_option("group_layout")))
        v.dev_sync()
        for k in range(calls):
            got = np.zeros(self.words, np.uint64)
            v.dev_download(got, self.bits[k])
            assert np.array_equal(bench.unpack_bits(got, self.n), self.exp), f"call {k}"
        return out

    def free(self):
        for p in self.d + self.bits:
            self.ver.dev_free(p)


def cold(b, ng=4):
    return (b.U, 0, ng)


def warm(b, ng=4):
    return (0, b.U, ng)


def promoted_in_eight(b, ng):
    """The same batch eight times from a cold context: per set cold, warm, warm on k4, then the promoting rebuild."""
    return [cold(b)] * 2 + [warm(b)] * 4 + [cold(b, ng)] * 2


def open_ver(ng):
    v = gvm.Verifier([0])
    assert v.get_option("group_reuse") == 1 and v.get_option("kg") == 0
    assert v.get_option("group_promote_min") == 262_144
    v.set_option("group_promote_min", 0)
    v.set_option("group_promote", ng)
    assert v.get_option("group_promote") == ng
    return v


@pytest.fixture()
def ver():
    v = open_ver(NG)
    yield v
    v.close()


@pytest.fixture(scope="module")
def mixed():
    """16,384 items over 1,024 keys, a tenth adversarial (random-x keys among them: ids of their own), with
    the special cases (point at infinity, x in [n, p), forced u1 / u2, small keys, digest edges) and every
    golden rejection class written over random positions; the oracle agrees with construction on a
    2,000-item sample that holds them all."""
    pub, sig, dig, exp = bench.make_digest_workload(N, 0xA1, 1024, 0.1, 16)
    rng = np.random.default_rng(21)
    sp, ss, sd, se, kinds = SC.make(np.random.default_rng(22), 3)
    gp, gs, gd, gok, classes = load_digest_vectors()
    assert {"high_s", "wrong_msg", "parity_flip", "bad_prefix"} <= set(classes)
    ap, as_, ad, ae = (np.concatenate(p) for p in ((sp, gp), (ss, gs), (sd, gd), (se, gok)))
    pos = rng.choice(N, len(ae), replace=False)
    pub[pos], sig[pos], dig[pos], exp[pos] = ap, as_, ad, ae
    idx = np.union1d(pos, rng.choice(N, 2000 - len(pos), replace=False))
    assert np.array_equal(O.verify_digests(pub[idx], sig[idx], dig[idx], threads=16), exp[idx])
    assert 512 <= len(key_ids(pub)) <= 1700
    return pub, sig, dig, exp


@pytest.fixture(scope="module")
def fresh():
    """16,384 valid items over 1,500 keys that `mixed` does not hold."""
    pub, sig, dig, exp = bench.make_digest_workload(N, 0xA2, 1500, 0.0, 16)
    idx = np.random.default_rng(23).choice(N, 2000, replace=False)
    assert np.array_equal(O.verify_digests(pub[idx], sig[idx], dig[idx], threads=16), exp[idx])
    return pub, sig, dig, exp


@pytest.mark.parametrize("ng", [6, 7, 9])
def test_same_batch_eight_times(mixed, ng):
    v = open_ver(ng)
    try:
        b = DevBatch(v, *mixed)
        assert b.run(8) == promoted_in_eight(b, ng)
        assert v.get_option("group_promoted") == 2 and v.get_option("group_demoted") == 0
        assert v.get_option("group_reuse_reset") == 2          # the promoting calls' flushes
        g0 = v.group_stats()
        assert b.run(4) == [warm(b, ng)] * 4                   # nothing is built after the promoting call
        g1 = v.group_stats()
        assert g1[0] - g0[0] == 4 and g1[1] == g0[1]
        r = v.route_stats()
        assert r["kg"] == 6 and r["k4f"] == 6
        assert v.get_option("group_promoted") == 2 and v.get_option("kg") == 0
        b.free()
    finally:
        v.close()


def test_rejected_keys_stay_rejected_across_the_rebuild(ver):
    """Goldens (every rejection class, infinity, x in [n, p), exceptional adds) tiled and shuffled."""
    gp, gs, gd, gok, _ = load_digest_vectors()
    reps = -(-N // len(gok))
    perm = np.random.default_rng(24).permutation(reps * len(gok))[:N]
    pub, sig, dig = (np.tile(a, (reps, 1))[perm] for a in (gp, gs, gd))
    exp = np.tile(gok, reps)[perm]
    b = DevBatch(ver, pub, sig, dig, exp, calls=12)
    assert b.U < len(np.unique(pub, axis=0))                   # some keys have no id: they get no row
    assert b.run(12) == promoted_in_eight(b, NG) + [warm(b, NG)] * 4
    b.free()


def test_new_keys_demote_and_repeats_promote_again(ver, mixed, fresh):
    a, b = DevBatch(ver, *mixed), DevBatch(ver, *fresh)
    assert a.run(8) == promoted_in_eight(a, NG)
    mem = ver.get_option("hbm_optional_bytes")
    rows = ver.get_option("group_reuse_rows")
    assert b.run(1) == [cold(b)]                               # every key missed: flushed, built on k4's layout
    assert ver.get_option("group_demoted") == 1
    assert b.run(1) == [cold(b)]                               # ... and the other set
    assert ver.get_option("group_demoted") == 2
    assert b.run(6) == [warm(b)] * 4 + [cold(b, NG)] * 2
    assert ver.get_option("group_promoted") == 4 and ver.get_option("group_demoted") == 2
    assert b.run(2) == [warm(b, NG)] * 2
    assert ver.get_option("hbm_optional_bytes") == mem         # no arena was freed or allocated on the way
    assert ver.get_option("group_reuse_rows") == rows
    a.free()
    b.free()


def test_overflow_flush_stays_promoted(ver):
    """Windows of 1,600 keys sliding by 400 over one 3,600-key pool (item i: key i % 3,600): each batch brings
    400 new keys (2.4 % of its items, below every layout's break-even) until the 3,328 rows no longer hold them."""
    keys, step, width = 3600, 400, 1600
    pub, sig, dig, exp = bench.make_digest_workload(keys * 11, 0xA3, keys, 0.0, 16)
    k = np.arange(keys * 11) % keys
    wins = []
    for t in range(6):
        ix = np.nonzero((k >= t * step) & (k < t * step + width))[0][:N]
        assert len(ix) == N
        wins.append(DevBatch(ver, pub[ix], sig[ix], dig[ix], exp[ix]))
        assert wins[-1].U == width
    ix = np.random.default_rng(25).choice(len(exp), 2000, replace=False)
    assert np.array_equal(O.verify_digests(pub[ix], sig[ix], dig[ix], threads=16), exp[ix])
    assert wins[0].run(8) == promoted_in_eight(wins[0], NG)
    for w in wins[1:5]:                                        # 2,000 ... 3,200 rows in use
        assert w.run(2) == [(step, width - step, NG)] * 2
    assert ver.get_option("group_reuse_reset") == 2            # the promoting calls' flushes
    assert ver.get_option("group_reuse_rows") == 3328
    assert wins[5].run(2) == [cold(wins[5], NG)] * 2           # 3,600 rows: flushed, all built from row 0, still kg
    assert ver.get_option("group_reuse_reset") == 4            # once more per set
    assert wins[5].run(2) == [warm(wins[5], NG)] * 2
    assert ver.get_option("group_promoted") == 2 and ver.get_option("group_demoted") == 0
    for w in wins:
        w.free()


def test_option_off_is_the_parent(ver, mixed):
    ver.set_option("group_promote", 0)
    b = DevBatch(ver, *mixed)
    assert b.run(8) == [cold(b)] * 2 + [warm(b)] * 6
    assert ver.get_option("group_promoted") == 0 and ver.get_option("group_demoted") == 0
    assert ver.get_option("group_reuse_reset") == 0
    # k_group_put's two launches per cold call, k_group_find and k_group_map per warm one
    assert ver.get_option("group_reuse_launches") == 2 * 2 + 6 * 2
    r = ver.route_stats()
    assert r["k4f"] == 8 and r["kg"] == 0
    b.free()


def test_explicit_kg_makes_promotion_inert(ver, mixed):
    ver.set_option("kg", 6)
    b = DevBatch(ver, *mixed)
    assert b.run(8) == [cold(b, 6)] * 2 + [warm(b, 6)] * 6
    assert ver.get_option("group_promoted") == 0
    assert ver.route_stats()["kg"] == 8
    b.free()


def test_budget_without_room_for_the_kg_arena_stays_on_k4(ver, mixed):
    b = DevBatch(ver, *mixed)
    # an arena of 3,328 rows is 16.8 MiB in k4's layout and 37.6 MiB in the 9-group one: 34-35 MiB past
    # the G tables hold both sets' k4 arenas and no 9-group arena, neither up front nor beside a k4 one
    mem0 = ver.get_option("hbm_optional_bytes")
    ver.set_option("hbm_budget_mb", (mem0 >> 20) + 35)
    assert b.run(2) == [cold(b)] * 2                           # both sets' arenas, k4-sized
    mem = ver.get_option("hbm_optional_bytes")
    assert 33 << 20 < mem - mem0 < 34 << 20
    assert b.run(6) == [warm(b)] * 6                           # the promotion is refused: no error, same tables
    assert ver.get_option("group_promoted") == 0
    assert ver.get_option("hbm_optional_bytes") == mem
    ver.set_option("hbm_budget_mb", 0)                         # no budget again, but not a quiescing option:
    assert b.run(2) == [warm(b)] * 2                           # the refused sets do not try again
    ver.set_option("keys_wide", ver.get_option("keys_wide"))   # a quiescing option: cold caches, a new attempt
    assert b.run(8) == promoted_in_eight(b, NG)                # (this promotion allocates the 9-group arenas)
    assert ver.get_option("group_promoted") == 2
    assert ver.get_option("hbm_optional_bytes") - mem0 > 75 << 20
    b.free()


def test_quiescing_option_keeps_a_promoted_set_promoted(ver, mixed):
    b = DevBatch(ver, *mixed)
    assert b.run(8) == promoted_in_eight(b, NG)
    ver.set_option("keys_wide", ver.get_option("keys_wide"))   # drops every set's cache
    assert b.run(4) == [cold(b, NG)] * 2 + [warm(b, NG)] * 2   # rebuilt cold, directly in the kg layout
    assert ver.get_option("group_promoted") == 2 and ver.get_option("group_demoted") == 0
    ver.set_option("group_reuse", 1)                           # an option that chooses the schedule: back to k4
    assert b.run(2) == [cold(b)] * 2
    assert ver.get_option("group_demoted") == 0                # (cleared, not demoted)
    b.free()


def test_batch_below_group_promote_min_never_promotes(ver, mixed):
    ver.set_option("group_promote_min", N + 1)
    b = DevBatch(ver, *mixed)
    assert b.run(8) == [cold(b)] * 2 + [warm(b)] * 6
    assert ver.get_option("group_promoted") == 0
    ver.set_option("group_promote_min", N)                     # not a quiescing option: the history stands
    assert b.run(2) == [cold(b, NG)] * 2
    assert ver.get_option("group_promoted") == 2
    b.free()
