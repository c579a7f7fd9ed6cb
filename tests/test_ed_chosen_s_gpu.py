"""The [s]B half of every ed25519 verdict on the GPU, at the edges of S and on
every comb-table entry a valid S can name (tests/ed_chosen_s.py; the same
items pass the CPU build of the device source in test_ed_chosen_s_host.py).

SMALL -- the edge values of S under the identity key and their twins, the
torsion-key items (their [h](-A) is not the identity) and the radix-256
sweeps with twins -- runs on every route with its own recoding of S:
k_ed_lat_unc, the throughput kernels and k_ed_keyed<4> with [s]B from either
table, k_ed_lat_sl, the wide arenas (k_ed_keyed<6>, <8>) and the grouped
route with radix-64 and radix-16 key combs.

BIG -- the radix-2^16 sweeps: entry (w, j) of btab16 for every j <= 2^15 in
every window below the top with each sign, every top-window entry an S < L
can name, and a rejected twin per item, 204,808 items -- runs on every route
that reads btab16, followed by the `plus` sweep with "ed_btab16" 0.

Every comparison is exact.  Each run also asserts the counters that show
where it ran (route_stats "ed_lat", group_stats, "ed_keyed_wide", "ed_kw_rb")
and "ed_btab16_live": the runtime adds [s]B from the radix-256 table when the
radix-2^16 one could not be built, with the same verdicts, so only that value
tells that btab16 was read at all."""
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest

import ed_chosen_s as C
import gpuverify as gvm

pytestmark = pytest.mark.gpu
ALL = 1 << 30
DEFAULTS = {"ed_unc_lat_max": 2048, "ed_lat_max": 2048, "ed_group": 1, "ed_group_min": 196608, "ed_group_r64": 1,
            "ed_btab16": 1}


@pytest.fixture(scope="module")
def sets():
    e, s8, s16 = C.edge_items(), C.sweeps(8), C.sweeps(16)
    small = C.concat("small", [e, C.twins(e), C.torsion_items()]
                     + [x for k in C.SWEEPS for x in (s8[k], C.twins(s8[k]))])
    big = C.concat("big", [x for k in C.SWEEPS for x in (s16[k], C.twins(s16[k]))])
    top = C.concat("top", [s16["top"], C.twins(s16["top"])])
    assert len(small) >= 256 and len(big) == 2 * (3 * 32769 + 4097)
    assert 0 < small.want.mean() < 1 and big.want.mean() == 0.5
    return SimpleNamespace(small=small, big=big, plus=s16["plus"], top=top)


@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    yield v
    v.close()


@pytest.fixture(scope="module", params=[6, 8])
def wide(request):
    """a context whose ed25519 arena holds wide comb tables: the option is set before the first load"""
    v = gvm.Verifier([0])
    v.set_option("ed_keys_wide", request.param)
    yield v, request.param
    v.close()


@contextmanager
def options(v, **kv):
    try:
        for k, x in kv.items():
            v.set_option(k, x)
        yield
    finally:
        for k in kv:
            v.set_option(k, DEFAULTS[k])


# ------------------------------------------------------------ entry points
def slots_of(v, items):
    """the arena slot of every item's key; a key is loaded once per context"""
    have = vars(v).setdefault("_chosen_s_slots", {})
    uniq, inv = np.unique(items.pub, axis=0, return_inverse=True)
    new = [u for u in uniq if bytes(u) not in have]
    if new:
        for u, s in zip(new, v.ed_keys_load(np.array(new, np.uint8).reshape(-1, 32))):
            have[bytes(u)] = int(s)
    return np.array([have[bytes(u)] for u in uniq], np.uint32)[inv.reshape(-1)]


def host_unkeyed(v, items):
    return v.verify_batch_ed25519(items.pub, items.sig, items.msg_arg())


def host_keyed(v, items):
    return v.verify_batch_ed25519_keyed(slots_of(v, items), items.sig, items.msg_arg())


def dev_keyed(v, items):
    """gv_dev_verify_ed25519_msgs_keyed: device-resident inputs, accept bitmap"""
    n = len(items)
    if items.msgs is None:
        blob, off, ln = np.zeros(256, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    else:
        blob, off, ln = gvm.pack_msgs(items.msgs)
    arrs = [np.ascontiguousarray(a) for a in (slots_of(v, items), items.sig, blob, off, ln)]
    nw = (n + 63) // 64
    ptrs = [v.dev_alloc(max(a.nbytes, 256)) for a in arrs] + [v.dev_alloc(nw * 8)]
    try:
        for p, a in zip(ptrs, arrs):
            v.dev_upload(p, a)
        v.dev_verify_ed25519_keyed(0, n, *ptrs)
        v.dev_sync()
        bits = np.zeros(nw, np.uint64)
        v.dev_download(bits, ptrs[-1])
    finally:
        for p in ptrs:
            v.dev_free(p)
    return np.unpackbits(bits.view(np.uint8), bitorder="little")[:n]


# ---------------------------------------------------------------- checking
def counters(v):
    return {"ed_lat": v.route_stats()["ed_lat"], "grouped": v.group_stats()[0], "wide": v.get_option("ed_keyed_wide"),
            "rb": v.get_option("ed_kw_rb"), "live": v.get_option("ed_btab16_live")}


def isolate(call, v, items, i):
    """For item i of a radix-2^16 sweep: the single-digit values of its j on the
    same route, and which (w, digit) fail there."""
    if not items.label[i].startswith("r16 "):
        return ""
    j = int(items.label[i].split("j=")[1].split()[0])
    probes, labels = C.single_digit_probes(j)
    got = call(v, probes)
    return f"; single-digit probes failing as (w, digit): {[lb for lb, g in zip(labels, got) if g != 1] or 'none'}"


def run(what, call, v, items, *, ed_lat=0, grouped=0, wide=False, rb=0, reads16=True, bits=16):
    """one call on a route: the counters say it ran where it should, every verdict is the expected one"""
    before = counters(v)
    got = call(v, items)
    after = counters(v)
    assert after["ed_lat"] - before["ed_lat"] == ed_lat, (what, before, after)
    assert after["grouped"] - before["grouped"] == grouped, (what, before, after)
    assert (after["wide"] > before["wide"]) == wide, (what, before, after)
    assert after["rb"] == rb, (what, after)
    if reads16:
        assert after["live"] == 1, f"{what}: the radix-2^16 table of B was not built: [s]B came from the radix-256 table"
    else:
        assert after["live"] == before["live"], (what, before, after)
    assert got.shape == items.want.shape
    bad = np.nonzero(got != items.want)[0]
    if bad.size:
        i = int(bad[0])
        pytest.fail(f"{what}: {bad.size} of {len(items)} verdicts wrong; first: got {int(got[i])} for "
                    f"{items.describe(i, bits)}; then {[items.label[k] for k in bad[1:5]]}" + isolate(call, v, items, i))
    return got


# route name -> (entry point, options, what run() expects); b16: [s]B from btab16 (1) or the radix-256 table (0)
def unkeyed_routes(b16=1):
    return {
        "throughput": (host_unkeyed, dict(ed_unc_lat_max=0, ed_group=0, ed_btab16=b16), dict(reads16=bool(b16))),
        "grouped_r64": (host_unkeyed, dict(ed_unc_lat_max=0, ed_group=1, ed_group_min=256, ed_group_r64=1, ed_btab16=b16),
                        dict(grouped=1, reads16=bool(b16))),
        "grouped_r16": (host_unkeyed, dict(ed_unc_lat_max=0, ed_group=1, ed_group_min=256, ed_group_r64=0, ed_btab16=b16),
                        dict(grouped=1, reads16=bool(b16))),
    }


def keyed_routes(b16=1):
    return {
        "keyed4": (host_keyed, dict(ed_lat_max=0, ed_btab16=b16), dict(reads16=bool(b16))),
        "keyed4_dev": (dev_keyed, dict(ed_lat_max=0, ed_btab16=b16), dict(reads16=bool(b16))),
    }


# ------------------------------------------------------------------- SMALL
def test_small_k_ed_lat_unc(ver, sets):
    with options(ver, ed_unc_lat_max=ALL):
        run("k_ed_lat_unc", host_unkeyed, ver, sets.small, ed_lat=1, reads16=False, bits=8)


def test_small_k_ed_lat_sl(ver, sets):
    with options(ver, ed_lat_max=ALL):
        run("k_ed_lat_sl", host_keyed, ver, sets.small, reads16=False, bits=8)


@pytest.mark.parametrize("b16", [1, 0])
@pytest.mark.parametrize("route", ["throughput", "grouped_r64", "grouped_r16", "keyed4", "keyed4_dev"])
def test_small_per_lane_routes(ver, sets, route, b16):
    call, opts, expect = {**unkeyed_routes(b16), **keyed_routes(b16)}[route]
    with options(ver, **opts):
        run(f"{route} ed_btab16={b16}", call, ver, sets.small, bits=16 if b16 else 8, **expect)


@pytest.mark.parametrize("b16", [1, 0])
def test_small_wide_arena(wide, sets, b16):
    v, rb = wide
    with options(v, ed_lat_max=0, ed_btab16=b16):
        run(f"k_ed_keyed<{rb}> ed_btab16={b16}", host_keyed, v, sets.small, wide=True, rb=rb, reads16=bool(b16),
            bits=16 if b16 else 8)
    with options(v, ed_lat_max=ALL):                          # the sliced kernel of the same context: radix-16 tables
        run(f"k_ed_lat_sl beside a radix-2^{rb} arena", host_keyed, v, sets.small, rb=rb, reads16=False, bits=8)


# --------------------------------------------------------------------- BIG
def big_then_plus_without_btab16(what, v, sets, routes_of, route, **more):
    call, opts, expect = routes_of(1)[route]
    with options(v, **opts):
        got = run(f"{what}", call, v, sets.big, **{**expect, **more})
    assert v.get_option("ed_btab16_live") == 1
    call, opts, expect = routes_of(0)[route]
    with options(v, **opts):
        again = run(f"{what}, plus sweep with ed_btab16=0", call, v, sets.plus, **{**expect, **more})
    assert np.array_equal(again, got[:len(sets.plus)])       # big starts with the plus sweep
    assert v.get_option("ed_btab16_live") == 1


@pytest.mark.parametrize("route", ["throughput", "grouped_r64", "grouped_r16"])
def test_big_sweeps_unkeyed(ver, sets, route):
    big_then_plus_without_btab16(route, ver, sets, unkeyed_routes, route)


@pytest.mark.parametrize("route", ["keyed4", "keyed4_dev"])
def test_big_sweeps_keyed(ver, sets, route):
    big_then_plus_without_btab16(route, ver, sets, keyed_routes, route)


def test_big_sweeps_wide_arena(wide, sets):
    v, rb = wide
    big_then_plus_without_btab16(f"k_ed_keyed<{rb}>", v, sets, keyed_routes, "keyed4", wide=True, rb=rb)


# -------------------------------------------------- build-then-read ordering
def test_first_keyed_call_of_a_context_builds_the_table_it_reads(sets):
    """The first call that wants btab16 builds it inside that call; the top
    sweep (every top-window entry, with twins) is that call."""
    v = gvm.Verifier([0])
    try:
        assert v.get_option("ed_btab16_live") == 0
        slots_of(v, sets.top)                                 # loading keys does not build it
        assert v.get_option("ed_btab16_live") == 0
        with options(v, ed_lat_max=0):
            before = counters(v)
            got = host_keyed(v, sets.top)
        assert v.get_option("ed_btab16_live") == 1
        assert counters(v)["wide"] == before["wide"] and counters(v)["rb"] == 0
        bad = np.nonzero(got != sets.top.want)[0]
        assert bad.size == 0, (bad.size, [sets.top.describe(int(i)) for i in bad[:4]])
    finally:
        v.close()
