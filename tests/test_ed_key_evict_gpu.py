"""GPU test of the host mirror's clock eviction over the ed25519 key arena
(gvh_set_ed_key_resident) on the real library: 12 chains of 40 validators
whose trusted commits arrive round-robin against an arena kept at 128 slots
must give the results of a run without eviction and of tests/commit_ref.py,
on the keyed route, with the arena never past its resident size and never
started over."""
import numpy as np
import pytest

import gpuverify as gvm
import gvhost
from test_ibc_commits import COMMIT, Chain, _signer, flip, ref

pytestmark = pytest.mark.gpu

CHAINS, VALS, RESIDENT, ROUNDS = 12, 40, 128, 3


@pytest.fixture(scope="module")
def calls():
    """Per call one trusted commit, the chains round-robin; every fifth commit
    has a signature with a flipped bit.  The last call carries four chains."""
    wl = _signer()
    rng = np.random.default_rng(0xE71C)
    chains = [Chain(wl, rng, VALS, chain_id="ibc-%d" % c) for c in range(CHAINS)]
    out = []
    for k in range(ROUNDS * CHAINS):
        ch = chains[k % CHAINS]
        s = ch.commit(100 + k, [COMMIT] * VALS)
        if k % 5 == 0:
            s = flip(s, int(rng.integers(VALS)))
        out.append([{"vals": ch.vals, "sigs": s, "keys_trusted": True}])
    # 160 keys: more than a resident size of 128 can evict; none of them resident when it comes
    out.append([{"vals": chains[c].vals, "sigs": chains[c].commit(900 + c, [COMMIT] * VALS), "keys_trusted": True}
                for c in (0, 1, 2, 3)])
    return out


def run(calls, resident):
    """Per call: the results, the ed_lat route counter's move (uncached small
    batches), the arena's count and generation, and the replaced counter."""
    with gvm.Verifier([0]) as v:
        app = gvhost.HostApp(v, chain_id="ibc-chain", height=1)
        try:
            app.set_ed_key_resident(resident)
            assert app.ed_key_stats() == (resident, 0, 0)
            out = []
            for cs in calls:
                r0 = v.route_stats()["ed_lat"]
                got = app.verify_commits(cs)
                out.append((got, v.route_stats()["ed_lat"] - r0, v.ed_keys_count, v.ed_keys_generation,
                            app.ed_key_stats()[1]))
            return out, app.ed_key_stats(), v.get_option("ed_keys_replaced")
        finally:
            app.close()


def test_round_robin_commits_with_eviction_equal_plain_run_and_reference(calls):
    on, (resident, replaced, resets), lib_replaced = run(calls, RESIDENT)
    off, stats_off, lib_off = run(calls, 0)
    assert stats_off == (0, 0, 0) and lib_off == 0
    assert [got for got, *_ in on] == [got for got, *_ in off]
    kinds = [g[0] for got, *_ in on for g in got]
    assert kinds.count("wrong_sig") == len(range(0, ROUNDS * CHAINS, 5)) and set(kinds) == {"ok", "wrong_sig"}
    for k in (0, 3, 4, 5, 17, 35, len(calls) - 1):                      # pure-Python ed25519 is slow: spot checks
        assert on[k][0] == [ref(d) for d in calls[k]], k
    # the arena stays at its resident size and is never started over
    assert resident == RESIDENT and replaced > 0 and resets == 0 and lib_replaced == replaced
    assert all(count <= RESIDENT for _, _, count, _, _ in on) and on[-1][2] == RESIDENT
    assert len({gen for _, _, _, gen, _ in on}) == 1
    assert off[-1][2] == CHAINS * VALS                                   # ... which the plain run passes
    # every chain's set is evicted before its turn comes again: each later call replaces its 40 keys
    assert on[2][4] == 0 and on[3][4] == 4 * VALS - RESIDENT and on[4][4] == on[3][4] + VALS
    # keyed route for every single-commit call, eviction on or off ...
    assert all(moved == 0 for _, moved, _, _, _ in on[:-1] + off)
    # ... and the last call, whose 160 fresh keys outnumber the evictable slots, runs unkeyed and changes nothing
    assert on[-1][1] >= 1 and on[-1][2] == on[-2][2] and on[-1][4] == on[-2][4] == replaced


def test_changing_the_resident_size_starts_the_arena_over(calls):
    with gvm.Verifier([0]) as v:
        app = gvhost.HostApp(v, chain_id="ibc-chain", height=1)
        try:
            app.verify_commits(calls[0])
            assert v.ed_keys_count == VALS
            gen = v.ed_keys_generation
            app.set_ed_key_resident(64)
            assert v.ed_keys_count == 0 and v.ed_keys_generation == gen + 1
            for cs in calls[:3]:
                got = app.verify_commits(cs)
                assert [g[0] for g in got] == [ref(d)[0] for d in cs]
            # 40 loaded; 24 loaded and 16 replaced; 40 replaced
            assert v.ed_keys_count == 64 and app.ed_key_stats() == (64, 3 * VALS - 64, 0)
            assert v.ed_keys_generation == gen + 1
        finally:
            app.close()
