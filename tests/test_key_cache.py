"""GPU tests of the account pubkey cache (gv_keys_load + keyed verifies,
SURVEY.md §8f-2): a keyed verify must give exactly the verdict of the pub33
path -- hence of the oracle -- for the key loaded into the slot, including keys
ParsePubKey rejects and slots that were never loaded."""
import numpy as np
import pytest

import gpuverify as gvm
from golden_io import load_digest_vectors, load_msg_vectors
from oracle import oracle as O
from test_gpu_parity import PATHS, make_random_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    yield v
    v.close()


# (lat_max, sliced, keys_k6, keys_wide, lat_kw): the PATHS schedules (rows: pub33
# only) with the resident arena's wide-window tables (small batches:
# k_verify_lat16_kw), plus the sliced kernel on the kn tables (lat_kw 0) and on
# the k4 tables, and the throughput ladders on the k6 tables and the two-window layout
KEYED_PATHS = {**{p: (v[0], v[1], 1, 2, 1) for p, v in PATHS.items() if p != "latency_rows"},
               "latency_kn_arena": (1 << 30, 1, 1, 2, 0),
               "latency_k4_arena": (1 << 30, 1, 0, 0, 1), "throughput_k6_arena": (0, 1, 1, 0, 1),
               "throughput_wide_two": (0, 1, 1, 1, 1)}


@pytest.fixture(params=sorted(KEYED_PATHS))
def path(request, ver):
    """Keyed batches take the fused small-batch kernel up to lat_max
    (k_verify_lat16_kw on the arena's one-window wide tables,
    k_verify_lat16_kn on its kn tables with lat_kw 0, k_verify_lat16_sl on its
    k4 tables with keys_k6 0, or k_verify_lat16 with lat_sliced 0), the
    throughput pipeline above it: every schedule is checked."""
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


def keyed_inputs(ver, pub):
    """Load the distinct keys of `pub` (in first-seen order) and map items to slots."""
    uniq, first, inv = np.unique(pub, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    slots = ver.keys_load(uniq[order])
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return slots[rank[inv.reshape(-1)]]


def test_golden_vectors_keyed(ver, path):
    ver.keys_reset()
    pub, sig, dig, ok, cats = load_digest_vectors()
    got = ver.verify_batch_digests_keyed(keyed_inputs(ver, pub), sig, dig)
    bad = [(i, cats[i], int(ok[i])) for i in range(len(ok)) if got[i] != ok[i]]
    assert not bad, bad[:20]
    pub, sig, msgs, ok, cats = load_msg_vectors()
    got = ver.verify_batch_msgs_keyed(keyed_inputs(ver, pub), sig, msgs)
    bad = [(i, cats[i], int(ok[i])) for i in range(len(ok)) if got[i] != ok[i]]
    assert not bad, bad[:20]


def test_adversarial_keyed_equals_oracle_and_pub_path(ver, path):
    ver.keys_reset()
    pub, sig, dig = make_random_batch(20000, seed=0xCA, adversarial=0.25, nkeys=301)
    want = O.verify_digests(pub, sig, dig, threads=16)
    slots = keyed_inputs(ver, pub)
    got = ver.verify_batch_digests_keyed(slots, sig, dig)
    assert np.array_equal(got, want)
    assert np.array_equal(got, ver.verify_batch_digests(pub, sig, dig))


@pytest.mark.parametrize("n", [1, 17, 255, 256, 257, 3000])
def test_ragged_keyed_and_unloaded_slots(ver, n, path):
    ver.keys_reset()
    pub, sig, dig = make_random_batch(n, seed=1000 + n, adversarial=0.3, nkeys=5)
    want = O.verify_digests(pub, sig, dig, threads=8)
    slots = keyed_inputs(ver, pub)
    assert np.array_equal(ver.verify_batch_digests_keyed(slots, sig, dig), want)
    # a slot that was never loaded is false, whatever the signature
    bad = slots.copy()
    bad[::3] = ver.keys_count + np.arange(len(bad[::3]), dtype=np.uint32)
    exp = want.copy()
    exp[::3] = 0
    assert np.array_equal(ver.verify_batch_digests_keyed(bad, sig, dig), exp)


def _special_msg_items(n, seed):
    """n message items, one key each, e = SHA-256 of the message: item 0 sums
    to the point at infinity (d = -e / r), item 1 has R.x = n + delta with
    r = n + delta ("x_in_n_p_rbig": reject), item 2 the same R with r = delta
    (accept), item 3 a valid signature over a message with one bit flipped
    afterwards; the rest valid.  n == 1: `seed` picks which of the four."""
    import random

    import special_cases as S
    rng = random.Random(seed)
    items = []

    def add(pub, r, s, msg):
        items.append((np.frombuffer(pub, np.uint8), np.frombuffer(S._b32(r) + S._b32(s), np.uint8), msg))

    for i in ([seed % 4] if n == 1 else range(n)):
        msg = rng.randbytes(rng.randrange(1, 300))
        e = int.from_bytes(O.sha256(msg), "big")
        if i == 0:                                              # infinity
            r = rng.randrange(1, S.N)
            add(S.R.compress(S._mul(-e * pow(r, S.N - 2, S.N))), r, rng.randrange(1, 2**62), msg)
        elif i in (1, 2):                                       # R.x in [n, p)
            Q = None
            while Q is None:
                delta = rng.choice(S._deltas())
                s = rng.randrange(1, S.HALF_N)
                Q = S._recover(S._lift(S.N + delta, rng.randrange(2)), delta, s, e)
            add(S.R.compress(Q), S.N + delta if i == 1 else delta, s, msg)
        else:
            priv = rng.randrange(1, S.N).to_bytes(32, "big")
            sig = O.sign(priv, O.sha256(msg))
            if i == 3:                                          # wrong message
                msg = bytes([msg[0] ^ 1]) + msg[1:]
            items.append((np.frombuffer(O.pubkey(priv), np.uint8), np.frombuffer(bytes(sig), np.uint8), msg))
    pub, sig, msgs = (np.array([it[0] for it in items]), np.array([it[1] for it in items]), [it[2] for it in items])
    want = np.array([O.verify_bytes(bytes(p), m, bytes(s)) for p, s, m in zip(pub, sig, msgs)], np.uint8)
    return pub, sig, msgs, want


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("arena", ["kn", "k4"])
def test_keyed_messages_staged_bitmap_kn_and_k4(ver, arena, n):
    """k_verify_lat16_kn (lat_kw 0) and k_verify_lat16_sl (keys_k6 0, keys_wide
    0) on the message path with bitmap verdicts (lat_zero_copy 0: staged input,
    the kernel sets bits): the point at infinity, R.x in [n, p) with r = R.x
    (reject) and r = R.x - n (accept), a wrong message, against the oracle."""
    ver.keys_reset()
    for k, v in ({"lat_kw": 0} if arena == "kn" else {"keys_k6": 0, "keys_wide": 0}).items():
        ver.set_option(k, v)
    ver.set_option("lat_zero_copy", 0)
    try:
        for seed in (range(4) if n == 1 else [n]):              # n == 1: each special item as its own batch
            pub, sig, msgs, want = _special_msg_items(n, seed)
            if n > 1:
                assert list(want[:4]) == [0, 0, 1, 0] and want[4:].all()
            slots = ver.keys_load(pub)
            before = ver.route_stats()["lat_keyed"]
            assert np.array_equal(ver.verify_batch_msgs_keyed(slots, sig, msgs), want)
            assert ver.route_stats()["lat_keyed"] == before + 1
    finally:
        ver.set_option("lat_zero_copy", 1)
        ver.set_option("lat_kw", 1)
        ver.set_option("keys_k6", 1)
        ver.set_option("keys_wide", 2)
        ver.keys_reset()


def test_arena_growth_keeps_earlier_slots(ver):
    """Many loads grow the arena (re-allocation + copy); earlier slots stay valid."""
    ver.keys_reset()
    pub, sig, dig = make_random_batch(6000, seed=31, adversarial=0.2, nkeys=6000)
    want = O.verify_digests(pub, sig, dig, threads=16)
    slots = np.concatenate([ver.keys_load(pub[i:i + 1500]) for i in range(0, 6000, 1500)])
    assert ver.keys_count == 6000 and np.array_equal(slots, np.arange(6000))
    assert np.array_equal(ver.verify_batch_digests_keyed(slots, sig, dig), want)


def test_device_resident_keyed(ver):
    ver.keys_reset()
    n = 5000
    pub, sig, dig = make_random_batch(n, seed=41, adversarial=0.25, nkeys=97)
    want = O.verify_digests(pub, sig, dig, threads=16)
    slots = keyed_inputs(ver, pub)
    bufs = [ver.dev_alloc(a.nbytes) for a in (slots, sig, dig)]
    d_bits = ver.dev_alloc(((n + 63) // 64) * 8)
    try:
        for p, a in zip(bufs, (slots, sig, dig)):
            ver.dev_upload(p, a)
        ver.dev_verify_digests_keyed(0, n, bufs[0], bufs[1], bufs[2], d_bits)
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        ver.dev_download(bits, d_bits)
    finally:
        for p in bufs + [d_bits]:
            ver.dev_free(p)
    got = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n]
    assert np.array_equal(got, want)


def test_keyed_two_device_slots():
    pub, sig, dig = make_random_batch(3001, seed=78, adversarial=0.25, nkeys=13)
    want = O.verify_digests(pub, sig, dig, threads=16)
    with gvm.Verifier([0, 0]) as v2:
        slots = keyed_inputs(v2, pub)
        assert np.array_equal(v2.verify_batch_digests_keyed(slots, sig, dig), want)
