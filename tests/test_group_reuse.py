"""The grouped route's per-set key-table cache (gv_set_option "group_reuse";
DESIGN section 4.1k): a scratch set keeps the tables of the keys it has built,
and a later batch on that set builds only the keys it has not seen
(k_group_find / k_group_put / k_group_map over the set's arena).  Device
calls on the context stream alternate the two scratch sets, each with a cache
of its own, so every scenario runs in pairs of calls.

Shapes: 16,384 items (above lat_max, at group_min) over 512-1,700 distinct
keys: the smallest grouped batch; its arena has 3,328 rows, so three disjoint
1,500-key batches overflow it.  The counters are the library's
("group_reuse_hit" / "_built" / "_reset" / "_launches"); the distinct keys of
a batch are counted here from its bytes, by k_dedupe's rule (prefix 02 / 03
and x < p: any other key gets no id, no row and a false verdict)."""
import numpy as np
import pytest

import bench
import gpuverify as gvm
from golden_io import load_digest_vectors
from oracle import oracle as O

pytestmark = pytest.mark.gpu

N = 16_384
P_BYTES = bytes.fromhex("FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2F")


def key_ids(pub):
    """The set of distinct keys of a batch that k_dedupe gives an id."""
    rows = {bytes(r) for r in np.unique(pub, axis=0)}
    return {r for r in rows if r[0] in (2, 3) and r[1:] < P_BYTES}


class DevBatch:
    """A batch resident on device 0, with one bitmap per call in flight."""

    def __init__(self, ver, pub, sig, dig, exp, calls=4):
        self.ver, self.n, self.exp = ver, len(exp), exp
        self.ids = key_ids(pub)
        self.d = [ver.dev_alloc(a.nbytes) for a in (pub, sig, dig)]
        for p, a in zip(self.d, (pub, sig, dig)):
            ver.dev_upload(p, np.ascontiguousarray(a))
        self.words = (self.n + 63) // 64
        self.bits = [ver.dev_alloc(self.words * 8) for _ in range(calls)]

    def run(self, calls=2):
        """`calls` pipelined calls; per call (keys built, keys reused), then every bitmap checked."""
        v, out = self.ver, []
        for k in range(calls):
            h0, b0 = v.get_option("group_reuse_hit"), v.get_option("group_reuse_built")
            v.dev_verify_digests(0, self.n, self.d[0], self.d[1], self.d[2], self.bits[k])
            out.append((v.get_option("group_reuse_built") - b0, v.get_option("group_reuse_hit") - h0))
        v.dev_sync()
        for k in range(calls):
            got = np.zeros(self.words, np.uint64)
            v.dev_download(got, self.bits[k])
            assert np.array_equal(bench.unpack_bits(got, self.n), self.exp), f"call {k}"
        return out

    def free(self):
        for p in self.d + self.bits:
            self.ver.dev_free(p)


@pytest.fixture()
def ver():
    v = gvm.Verifier([0])
    assert v.get_option("group_reuse") == 1
    yield v
    v.close()


@pytest.fixture(scope="module")
def base():
    """16,384 items over 1,024 keys, a quarter adversarial (random-x keys among them: ids of their own)."""
    return bench.make_digest_workload(N, 0x91, 1024, 0.25, 16)


def test_same_batch_four_times(ver, base):
    pub, sig, dig, exp = base
    idx = np.random.default_rng(11).choice(N, 2000, replace=False)
    assert np.array_equal(O.verify_digests(pub[idx], sig[idx], dig[idx], threads=16), exp[idx])
    b = DevBatch(ver, pub, sig, dig, exp)
    U = len(b.ids)
    assert 1024 <= U <= N // 5
    g0 = ver.group_stats()
    assert b.run(4) == [(U, 0), (U, 0), (0, U), (0, U)]       # cold, cold, warm, warm
    g1 = ver.group_stats()
    assert g1[0] - g0[0] == 4 and g1[1] - g0[1] == 2 * U       # the second number: keys whose tables were built
    assert ver.get_option("group_reuse_reset") == 0
    assert ver.route_stats()["k4f" if gvm.Verifier.KG_DEFAULT == 0 else "kg"] == 4
    b.free()


def test_partial_overlap(ver):
    """Key sets X (keys 0..1023) and Y (keys 512..1535) of one 1,536-key workload, 16,384 items each."""
    pub, sig, dig, exp = bench.make_digest_workload(24_576, 0x92, 1536, 0.1, 16)
    k = np.arange(24_576) % 1536
    ix, iy = np.nonzero(k < 1024)[0], np.nonzero(k >= 512)[0]
    assert len(ix) == N and len(iy) == N
    X = DevBatch(ver, pub[ix], sig[ix], dig[ix], exp[ix])
    Y = DevBatch(ver, pub[iy], sig[iy], dig[iy], exp[iy])
    idx = np.random.default_rng(12).choice(N, 2000, replace=False)
    assert np.array_equal(O.verify_digests(pub[iy][idx], sig[iy][idx], dig[iy][idx], threads=16), exp[iy][idx])
    new_y, both = len(Y.ids - X.ids), len(Y.ids & X.ids)
    assert both >= 512 and new_y >= 512
    assert X.run(2) == [(len(X.ids), 0)] * 2
    assert len(X.ids | Y.ids) <= ver.get_option("group_reuse_rows")   # both fit: no flush below
    assert Y.run(2) == [(new_y, both)] * 2                     # only the keys X did not bring
    assert X.run(2) == [(0, len(X.ids))] * 2
    assert Y.run(2) == [(0, len(Y.ids))] * 2
    assert ver.get_option("group_reuse_reset") == 0
    X.free()
    Y.free()


def test_rejected_keys_are_cached_as_rejected(ver):
    """Goldens (every rejection class, infinity, x in [n, p), exceptional adds) tiled and shuffled."""
    gp, gs, gd, gok, _ = load_digest_vectors()
    reps = -(-N // len(gok))
    perm = np.random.default_rng(13).permutation(reps * len(gok))
    pub, sig, dig = (np.tile(a, (reps, 1))[perm] for a in (gp, gs, gd))
    exp = np.tile(gok, reps)[perm]
    b = DevBatch(ver, pub, sig, dig, exp, calls=6)
    U = len(b.ids)
    assert U < len(np.unique(pub, axis=0))                     # some keys have no id: they get no row
    assert b.run(6) == [(U, 0)] * 2 + [(0, U)] * 4             # three times per set, the same verdicts each time
    b.free()


def test_overflow_flushes_then_refills(ver):
    """Disjoint 1,500-key batches: two fill the arena's rows, the third does not fit."""
    sets = [DevBatch(ver, *bench.make_digest_workload(N, 0x93 + i, 1500, 0.0, 16), calls=2) for i in range(3)]
    assert sets[0].run(2) == [(1500, 0)] * 2
    rows = ver.get_option("group_reuse_rows")                  # the arena's row capacity, allocated by the first call
    assert 3000 <= rows < 4500
    assert sets[1].run(2) == [(1500, 0)] * 2
    assert ver.get_option("group_reuse_reset") == 0
    assert sets[2].run(2) == [(1500, 0)] * 2                   # 3,000 + 1,500 rows: flushed, all built from row 0
    assert ver.get_option("group_reuse_reset") == 2            # once per set
    assert sets[2].run(2) == [(0, 1500)] * 2                   # ... and entered again: a full hit
    assert sets[0].run(2) == [(1500, 0)] * 2                   # the flushed keys are gone (3,000 rows in use)
    assert ver.get_option("group_reuse_reset") == 2
    for s in sets:
        s.free()


def test_layout_change_starts_cold(ver, base):
    b = DevBatch(ver, *base)
    U = len(b.ids)
    assert b.run(4) == [(U, 0)] * 2 + [(0, U)] * 2
    for key, val, route in (("kg", 6, "kg"), ("kg", 0, "k4f"), ("k6", 1, "k6"), ("k6", 0, "k4f")):
        ver.set_option(key, val)
        r0 = ver.route_stats()[route]
        assert b.run(4) == [(U, 0)] * 2 + [(0, U)] * 2, (key, val)   # the first call on each set builds all its keys
        assert ver.route_stats()[route] - r0 == 4, (key, val)
    b.free()


def test_option_off_launches_nothing(ver, base):
    b = DevBatch(ver, *base)
    U = len(b.ids)
    ver.set_option("group_reuse", 0)
    assert ver.get_option("group_reuse") == 0
    g0 = ver.group_stats()
    assert b.run(4) == [(0, 0)] * 4
    g1 = ver.group_stats()
    assert g1[0] - g0[0] == 4 and g1[1] - g0[1] == 4 * U       # every call builds every key
    assert ver.get_option("group_reuse_launches") == 0
    ver.set_option("group_reuse", 1)
    assert b.run(4) == [(U, 0)] * 2 + [(0, U)] * 2
    assert ver.get_option("group_reuse_launches") > 0
    ver.set_option("group_reuse", 0)                           # switched off again: the rows are rebuilt from 0
    l0 = ver.get_option("group_reuse_launches")
    assert b.run(2) == [(0, 0)] * 2
    assert ver.get_option("group_reuse_launches") == l0
    ver.set_option("group_reuse", 1)
    assert b.run(2) == [(U, 0)] * 2                            # ... so the cache starts cold
    b.free()


def test_unique_key_batch_between_grouped_calls(ver, base):
    b = DevBatch(ver, *base)
    u = DevBatch(ver, *bench.make_digest_workload(N, 0x97, N, 0.1, 16))
    U = len(b.ids)
    assert b.run(2) == [(U, 0)] * 2
    g0, r0 = ver.group_stats()[0], ver.route_stats()
    assert u.run(2) == [(0, 0)] * 2                            # the pub33 pipeline, on both sets
    r1 = ver.route_stats()
    assert ver.group_stats()[0] == g0
    assert (r1["pub33"] + r1["item_f"]) - (r0["pub33"] + r0["item_f"]) == 2
    assert b.run(2) == [(0, U)] * 2                            # the cache was left as it was
    b.free()
    u.free()
