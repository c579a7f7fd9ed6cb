"""The resident key arena's narrow wide-window tables and the layout chain
(include/gpuverify.h "keys_wide", "keys_wide_qw", "keys_wide_mb").

The arena holds each key's wide-window tables in one of four layouts, in order
of falling memory per key: A (11-bit windows, one per group), B (11-bit, two
per group), C (9-bit, one) and D (9-bit, two).  gv_keys_load starts at the
first layout its options allow and moves the whole arena down the list when a
growth is refused; only a refusal of D leaves keyed batches on the 6-bit kn
tables.  Every layout must give the oracle's verdicts."""
import numpy as np
import pytest

import bench
import gpuverify as gvm
import special_cases as SC
from oracle import oracle as O
from oracle import secp_ref as R

gpu = pytest.mark.gpu

N, LAM = R.N, R.LAMBDA
DEFAULTS = {"keys_wide": 2, "keys_wide_qw": 0, "keys_wide_mb": 0, "keys_k6": 1}


@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    yield v
    v.close()


@pytest.fixture
def defaults(ver):
    yield
    for k, val in DEFAULTS.items():
        ver.set_option(k, val)
    ver.keys_reset()


def routes_of(ver, fn):
    r0 = ver.route_stats()
    out = fn()
    r1 = ver.route_stats()
    return out, {k: r1[k] - r0[k] for k in r1 if r1[k] != r0[k]}


def first_seen(pub):
    """The distinct keys of pub in first-seen order, and each item's index into them."""
    uniq, first, inv = np.unique(pub, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return uniq[order], rank[inv.reshape(-1)]


# ---- forced u2 = r / s on the edges of the 9-bit windows
def forced_u2_values():
    """A u2 below 2^127 splits to k1 = u2, k2 = 0, and LAM u2 to the other GLV
    half: digit +-256 (the last table entry), carry chains through all 15
    windows, the top window, and the two-window group boundaries of layout D."""
    w9 = [0x100, 0x1FF, 0x100 << 9, 2**126 - 1,
          sum(0x100 << (9 * w) for w in range(14)),               # 0x100 in every 9-bit window: 126 bits
          sum(0x1FF << (9 * w) for w in range(1, 14, 2)),         # 0x1FF in every other window: 126 bits
          sum(0x1FF << (9 * w) for w in range(0, 14, 2))]         # ... and in the windows between
    assert all(v < 2**127 for v in w9) and w9[4].bit_length() == 126 and w9[5].bit_length() == 126
    return [u for v in w9 for u in (v, LAM * v % N)]


def forced_u2_cases():
    rows = []
    for qi, dq in enumerate((1, 2, N - 1)):                        # Q = G, 2G, -G
        Q = SC._mul(dq)
        for ui, u2 in enumerate(forced_u2_values()):
            out = SC._sig_for_uv(0x3039 + 97 * ui + qi, u2, Q)
            assert out is not None, (dq, hex(u2))
            r, s, e = out
            rows.append((R.compress(Q), SC._b32(r) + SC._b32(s), SC._b32(e)))
    pub, sig, dig = (np.array([np.frombuffer(row[i], np.uint8) for row in rows]) for i in range(3))
    return pub, sig, dig, np.ones(len(rows), np.uint8)


@pytest.fixture(scope="module")
def narrow_batch():
    """(pub, sig, dig, by-construction verdicts, oracle verdicts): random items
    on 512 keys with a quarter adversarial, the special-case kinds, and the
    forced u2 cases."""
    parts = [bench.make_digest_workload(20_000, 0x9B, 512, 0.25, 16),
             SC.make(np.random.default_rng(0x9C), 64)[:4],
             forced_u2_cases()]
    pub, sig, dig, exp = (np.ascontiguousarray(np.concatenate([p[i] for p in parts])) for i in range(4))
    perm = np.random.default_rng(0x9D).permutation(len(exp))
    pub, sig, dig, exp = pub[perm], sig[perm], dig[perm], exp[perm].astype(np.uint8)
    want = O.verify_digests(pub, sig, dig, threads=16)
    return pub, sig, dig, exp, want


@gpu
@pytest.mark.parametrize("keys_wide, route, ng", [(2, "kw", 15), (1, "kw2", 8)])
def test_forced_narrow_layouts_match_the_oracle(ver, defaults, narrow_batch, keys_wide, route, ng):
    pub, sig, dig, exp, want = narrow_batch
    assert np.array_equal(want, exp)                               # the oracle agrees with the constructions
    ver.keys_reset()
    ver.set_option("keys_wide_qw", 9)                              # GV_EINVAL without the narrow table set
    ver.set_option("keys_wide", keys_wide)
    keys, idx = first_seen(pub)
    slots = ver.keys_load(keys)[idx].astype(np.uint32)
    assert ver.get_option("kw_arena_qw") == 9 and ver.get_option("kw_arena_ng") == ng
    got, routes = routes_of(ver, lambda: ver.verify_batch_digests_keyed(slots, sig, dig))
    assert routes.get(route, 0) >= 1, routes
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:10], want[bad[:10]])
    ver.set_option("keys_wide", 0)                                 # the kn tables of the same slots
    got6, routes = routes_of(ver, lambda: ver.verify_batch_digests_keyed(slots, sig, dig))
    assert routes.get("kn", 0) >= 1, routes
    assert np.array_equal(got6, got)


# ---- the chain A -> B -> C -> D -> kn, driven by "keys_wide_mb"
MIB = 1 << 20


def slot_bytes(qw, ng):
    """Bytes per key of the qw-bit layout of ng groups: per group 2^(qw - 1)
    entries of 64 B and 32 B of parked Z (gv_runtime.cpp key_wide_slot_bytes)."""
    return ng * ((1 << (qw - 1)) * 64 + 32)


LAYOUTS = [(11, 12), (11, 6), (9, 15), (9, 8)]                     # A, B, C, D: (kw_arena_qw, kw_arena_ng)


def round_up(x, m):
    return (x + m - 1) // m * m


def model_chain(limit, loads, key_cap, only_qw=0):
    """The arena's (layout index or None, capacity) after loading `loads` keys
    in turn from slot 0 under "keys_wide" 2 and a byte limit: the growth rule of
    ensure_keys_wide (doubling up to key_cap, never below 4,096 slots, rounded
    to 256; an arena rebuilt in another layout starts from capacity 0) and the
    chain of gv_keys_load."""
    allowed = [i for i, (qw, _) in enumerate(LAYOUTS) if not only_qw or qw == only_qw]
    li, cap, used = allowed[0], 0, 0

    def grown(cap, need):
        if need <= cap:
            return cap
        grow = need if cap >= key_cap else min(2 * cap, max(need, key_cap))
        return round_up(max(need, grow, 4096), 256)

    for n in loads:
        need = used + n
        new = grown(cap, need)
        while new * slot_bytes(*LAYOUTS[li]) > limit:
            nxt = [i for i in allowed if i > li]
            if not nxt:
                return None, 0
            li, new = nxt[0], grown(0, need)
        cap, used = new, need
    return li, cap


def chain_limits(key_cap):
    """Byte limits after which 3,000 + 3,000 keys end in layout C, in layout D
    and on the kn tables, from the slot sizes and the growth rule: a relayout
    allocates round_up(6,000, 256) = 6,144 slots, a plain growth 2 x 4,096."""
    sA, sB, sC, sD = (slot_bytes(*l) for l in LAYOUTS)
    # C: the first load fits B (4,096 slots) but not A; B's growth to 8,192 is refused, C at 6,144 fits
    lim_c = (max(4096 * sB, 6144 * sC) + min(4096 * sA, 8192 * sB)) // 2
    # D: the first load fits C but not B; C's growth to 8,192 is refused, D at 6,144 fits
    lim_d = (max(4096 * sC, 6144 * sD) + min(4096 * sB, 8192 * sC)) // 2
    # none: the first load fits D but not C; D's growth to 8,192 is refused
    lim_0 = (4096 * sD + min(4096 * sC, 8192 * sD)) // 2
    lims = [round_up(x, MIB) for x in (lim_c, lim_d, lim_0)]
    assert [model_chain(x, [3000, 3000], key_cap)[0] for x in lims] == [2, 3, None], lims
    return lims


def test_chain_limits_are_those_of_the_worked_example():
    lims = [x // MIB for x in chain_limits(1 << 22)]
    assert 1537 <= lims[0] < 3073 and 962 <= lims[1] < 1537 and 514 <= lims[2] < 962, lims


@pytest.fixture(scope="module")
def chain_batch():
    """6,000 distinct keys (the first seen of a batch a quarter adversarial:
    some are keys ParsePubKey rejects) and the batch's items on them."""
    pub, sig, dig, exp = bench.make_digest_workload(30_000, 0x9E, 6000, 0.25, 16)
    keys, idx = first_seen(pub)
    on = idx < 6000
    assert len(keys) >= 6000 and on.sum() > 20_000
    pub, sig, dig, idx = (np.ascontiguousarray(a[on]) for a in (pub, sig, dig, idx))
    want = O.verify_digests(pub, sig, dig, threads=16)
    assert 0 < want.mean() < 1
    return keys[:6000], idx, sig, dig, want


@gpu
@pytest.mark.parametrize("end", ["C", "D", "none"])
def test_chain_moves_down_the_layouts(ver, defaults, chain_batch, end):
    keys, idx, sig, dig, want = chain_batch
    key_cap = ver.get_option("key_cap")
    limit = chain_limits(key_cap)["C D none".split().index(end)]
    li_end, _ = model_chain(limit, [3000, 3000], key_cap)
    li_first, _ = model_chain(limit, [3000], key_cap)
    ver.keys_reset()
    ver.set_option("keys_wide", 2)
    ver.set_option("keys_wide_qw", 0)
    ver.set_option("keys_wide_mb", limit // MIB)
    a = ver.keys_load(keys[:3000])
    assert (ver.get_option("kw_arena_qw"), ver.get_option("kw_arena_ng")) == LAYOUTS[li_first]
    b = ver.keys_load(keys[3000:])                                  # past 4,096 slots: the growth is refused
    layout = LAYOUTS[li_end] if li_end is not None else (0, 0)
    assert (ver.get_option("kw_arena_qw"), ver.get_option("kw_arena_ng")) == layout
    assert layout == {"C": (9, 15), "D": (9, 8), "none": (0, 0)}[end]
    slots = np.concatenate([a, b]).astype(np.uint32)[idx]           # items on keys of both loads
    assert (idx < 3000).any() and (idx >= 3000).any()
    got, routes = routes_of(ver, lambda: ver.verify_batch_digests_keyed(slots, sig, dig))
    assert routes.get({"C": "kw", "D": "kw2", "none": "kn"}[end], 0) >= 1, routes
    assert np.array_equal(got, want)
    # an arena started from slot 0 is back at the first layout the limit allows
    ver.keys_reset()
    c = ver.keys_load(keys[3000:]).astype(np.uint32)
    assert (ver.get_option("kw_arena_qw"), ver.get_option("kw_arena_ng")) == LAYOUTS[li_first]
    sub = np.tile(np.nonzero(idx >= 3000)[0], 2)                    # twice: past the small-batch bound
    assert len(sub) > gvm.LAT_MAX_KEYED_DEFAULT
    got, routes = routes_of(ver, lambda: ver.verify_batch_digests_keyed(c[idx[sub] - 3000], sig[sub], dig[sub]))
    assert routes.get("kw" if LAYOUTS[li_first][1] in (12, 15) else "kw2", 0) >= 1, routes
    assert np.array_equal(got, want[sub])


@gpu
def test_width_11_only_ends_on_the_kn_tables(ver, defaults, chain_batch):
    """"keys_wide_qw" 11 under the smallest limit: layouts A and B are refused
    and the 9-bit layouts are not tried."""
    keys, idx, sig, dig, want = chain_batch
    key_cap = ver.get_option("key_cap")
    limit = chain_limits(key_cap)[2]
    assert model_chain(limit, [3000], key_cap, only_qw=11)[0] is None
    assert model_chain(limit, [3000], key_cap)[0] == 3             # ... which layout D would have held
    ver.keys_reset()
    ver.set_option("keys_wide", 2)
    ver.set_option("keys_wide_qw", 11)
    ver.set_option("keys_wide_mb", limit // MIB)
    a = ver.keys_load(keys[:3000])
    assert ver.get_option("kw_arena_qw") == 0 and ver.get_option("kw_arena_ng") == 0
    b = ver.keys_load(keys[3000:])
    assert ver.get_option("kw_arena_qw") == 0 and ver.get_option("kw_arena_ng") == 0
    slots = np.concatenate([a, b]).astype(np.uint32)[idx]
    got, routes = routes_of(ver, lambda: ver.verify_batch_digests_keyed(slots, sig, dig))
    assert routes.get("kn", 0) >= 1 and not routes.get("kw", 0) and not routes.get("kw2", 0), routes
    assert np.array_equal(got, want)


@gpu
def test_small_keyed_batch_on_a_narrow_arena(ver, defaults, narrow_batch):
    """64 items against a 9-bit arena: the small-batch kernel on the kn tables
    (k_verify_lat16_kw reads 11-bit tables only)."""
    pub, sig, dig, exp, want = narrow_batch
    ver.keys_reset()
    ver.set_option("keys_wide_qw", 9)
    ver.set_option("keys_wide", 2)
    keys, idx = first_seen(pub)
    slots = ver.keys_load(keys)[idx].astype(np.uint32)
    assert ver.get_option("kw_arena_qw") == 9
    sel = np.concatenate([np.nonzero(want == 0)[0][:24], np.nonzero(want == 1)[0][:40]])
    assert len(sel) == 64
    got, routes = routes_of(ver, lambda: ver.verify_batch_digests_keyed(slots[sel], sig[sel], dig[sel]))
    assert routes.get("lat_keyed", 0) >= 1 and not routes.get("kw", 0), routes
    assert np.array_equal(got, want[sel])
