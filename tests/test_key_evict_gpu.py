"""GPU test of the host mirror's clock eviction (gvh_set_key_resident) over the
real library: the churn workload of tests/evict_workload.py -- signers rotating
over 2,000 accounts against an arena kept at 512 slots -- must give the codes,
logs and final accounts of a run without eviction and of tests/ante_ref.py,
on the keyed routes, with the arena never past its resident size."""
import pytest

import evict_workload as W
import gpuverify as gvm
import gvhost

pytestmark = pytest.mark.gpu

KEYED = ("keyed125", "k4", "lat_keyed", "k4f", "kn", "kw", "kw2")       # schedules reading the key arena
UNKEYED = ("pub33", "lat", "item_f", "k6", "kg")                       # schedules taking pub33 items


@pytest.fixture(scope="module")
def load():
    accts, blocks, parts, _ = W.workload()
    codes, ref = W.reference_codes(accts, blocks, parts)
    return accts, blocks, codes, ref


def run(accts, blocks, resident):
    """Deliver the blocks one by one; per block the results, the route counters
    that moved, and the arena's count and generation after it."""
    with gvm.Verifier([0]) as v:
        app = gvhost.HostApp(v, chain_id=W.CHAIN, height=W.HEIGHT)
        try:
            app.set_keyed(True, 64)
            app.set_key_resident(resident)
            assert app.key_stats()[0] == resident
            for addr, num, seq, pub in accts:
                app.set_account(addr, num, seq, pub)
            out = []
            for txs in blocks:
                r0 = v.route_stats()
                rc, res = app.deliver_block(txs)
                assert rc == 0
                r1 = v.route_stats()
                out.append((res, {k: r1[k] - r0[k] for k in r1 if r1[k] != r0[k]}, v.keys_count,
                            v.keys_generation()))
            final = {addr: app.get_account(addr) for addr, _, _, _ in accts}
            return out, final, app.key_stats()
        finally:
            app.close()


def test_churn_with_eviction_equals_plain_run_and_reference(load):
    accts, blocks, codes, ref = load
    on, final_on, (resident, replaced, resets) = run(accts, blocks, W.RESIDENT)
    off, final_off, stats_off = run(accts, blocks, 0)
    assert stats_off == (0, 0, 0)
    assert [r for res, _, _, _ in on for r in res] == [r for res, _, _, _ in off for r in res]   # codes, logs, gas
    assert [r["code"] for res, _, _, _ in on for r in res] == codes
    assert 0 < codes.count(0) < len(codes)
    assert final_on == final_off
    for addr, acc in final_on.items():
        assert (acc["number"], acc["sequence"], acc["pub"]) == (
            ref.accounts[addr].number, ref.accounts[addr].sequence, ref.accounts[addr].pub)
    # the arena stays at its resident size and is never started over
    assert resident == W.RESIDENT and replaced > 0 and resets == 0
    assert all(count <= W.RESIDENT for _, _, count, _ in on) and on[-1][2] == W.RESIDENT
    assert len({gen for _, _, _, gen in on}) == 1
    assert off[-2][2] > W.RESIDENT                                     # ... which the plain run passes
    # keyed routes for the churn blocks (the first loads, the later ones replace) ...
    for _, routes, _, _ in on[:-1]:
        assert sum(routes.get(k, 0) for k in KEYED) >= 1 and not any(routes.get(k, 0) for k in UNKEYED), routes
    # ... and the pub33 route for the block whose fresh keys outnumber every evictable slot
    routes = on[-1][1]
    assert sum(routes.get(k, 0) for k in UNKEYED) >= 1 and not any(routes.get(k, 0) for k in KEYED), routes
