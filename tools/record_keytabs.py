#!/usr/bin/env python3
"""Record what a libgpuverify.so's key table sets hold and charge along one
sequence of loads, growths and grouped calls (needs a GPU):

    python tools/record_keytabs.py PATH/libgpuverify.so [OUT.json]

writes tests/golden/keytabs_parent.json (or OUT.json).  The fixture in the
tree was recorded from the library of the commit before the runtime's key
arenas moved onto one table-set type (KeyTabs, csrc/gv_keytabs.h);
tests/test_keytabs_gpu.py replays the sequence (run() below) on the current
library and requires every recorded number again.

The sequence, with the state (state()) recorded after each step:
  A  a context; 300 keys loaded (the arenas' floor capacity, 4,096 slots);
     4,000 more (4,096 -> 8,192 slots, the loaded prefix copied: k4, kn and
     wide tables); a keyed call of 16,384 items and one of 1,024
  B  a context with keys_wide1_cap = 4,096; the same two loads (the wide arena
     moves to its next layout and is rebuilt from keys read back); the two
     keyed calls; two pub33 device calls of 16,384 items over 1,024 keys (a
     grouped arena on both scratch sets); group_promote 9, group_promote_min
     0 and eight more (setting the option drops the sets' caches, so per set
     a cold call, two warm ones and the promoting rebuild in an arena of the
     promoted layout); gv_keys_reset and 300 keys

Every verifying call's verdicts are compared with the construction's, and
after each growth hook(v, step) runs (the test reads table entries there)."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "cosmos-sdk-rootchain_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N = 16_384
N_SMALL = 1_024
FIRST, MORE = 300, 4_000
OPTIONS = ("hbm_optional_bytes", "group_layout", "group_reuse_rows", "group_promoted", "group_demoted",
           "group_reuse_built", "group_reuse_hit", "kw_arena_qw", "kw_arena_ng", "keys_index_words")


class Workload:
    """4,300 keys with their private keys, keyed items signed by their slot's key (a tenth with a flipped digest
    bit: verdict 0), and a pub33 batch over 1,024 keys; verdicts by construction."""

    def __init__(self):
        import bench
        from oracle import oracle as O
        rng = np.random.default_rng(0xC7)
        priv = rng.integers(0, 256, size=(FIRST + MORE, 32), dtype=np.uint8)
        priv[:, 0] &= 0x7F
        priv[:, 31] |= 1
        self.pub = O.pubkey_batch(priv, threads=16)
        self.keyed = {}
        for n in (N, N_SMALL):
            slots = rng.integers(0, FIRST + MORE, n).astype(np.uint32)
            slots[:FIRST] = rng.permutation(FIRST)[:min(n, FIRST)]     # the copied prefix, every slot of it
            dig = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
            sig = O.sign_batch(np.ascontiguousarray(priv[slots]), dig, threads=16)
            exp = np.ones(n, np.uint8)
            bad = rng.choice(n, n // 10, replace=False)
            dig[bad, 7] ^= 1
            exp[bad] = 0
            self.keyed[n] = (slots, sig, dig, exp)
        self.grouped = bench.make_digest_workload(N, 0xC8, 1024, 0.1, 16)
        self.unpack_bits = bench.unpack_bits


def state(v):
    rec = {k: v.get_option(k) for k in OPTIONS}
    rec["routes"] = v.route_stats()
    return rec


def run(open_verifier, w, hook=None):
    """The sequence on contexts from open_verifier(); returns [[step name, state], ...]."""
    out = []

    def step(v, name):
        out.append([name, state(v)])
        if hook and name.endswith("grown"):
            hook(v, name)

    def loads(v, tag):
        assert np.array_equal(v.keys_load(w.pub[:FIRST]), np.arange(FIRST))
        step(v, tag + " floor")
        assert np.array_equal(v.keys_load(w.pub[FIRST:]), np.arange(FIRST, FIRST + MORE))
        step(v, tag + " grown")
        for n in (N, N_SMALL):
            slots, sig, dig, exp = w.keyed[n]
            assert np.array_equal(v.verify_batch_digests_keyed(slots, sig, dig), exp), f"{tag}: keyed call of {n}"
            step(v, f"{tag} keyed {n}")

    with open_verifier() as v:
        step(v, "A open")
        loads(v, "A")
    with open_verifier() as v:
        v.set_option("keys_wide1_cap", 4096)
        step(v, "B open")
        loads(v, "B")
        pub, sig, dig, exp = w.grouped
        d = [v.dev_alloc(a.nbytes) for a in (pub, sig, dig)]
        for p, a in zip(d, (pub, sig, dig)):
            v.dev_upload(p, np.ascontiguousarray(a))
        words = (N + 63) // 64
        bits = v.dev_alloc(words * 8)
        for call in range(10):
            if call == 2:
                v.set_option("group_promote_min", 0)
                v.set_option("group_promote", 9)
            v.dev_verify_digests(0, N, d[0], d[1], d[2], bits)
            v.dev_sync()
            got = np.zeros(words, np.uint64)
            v.dev_download(got, bits)
            assert np.array_equal(w.unpack_bits(got, N), exp), f"grouped call {call}"
            step(v, f"B grouped {call}")
        for p in d + [bits]:
            v.dev_free(p)
        v.keys_reset()
        step(v, "B reset")
        assert np.array_equal(v.keys_load(w.pub[:FIRST]), np.arange(FIRST))
        step(v, "B reloaded")
    return out


def main(argv):
    if not argv:
        print(__doc__)
        return 2
    import gpuverify
    gpuverify.load(os.path.abspath(argv[0]))
    out = argv[1] if len(argv) > 1 else os.path.join(REPO, "tests", "golden", "keytabs_parent.json")
    steps = run(lambda: gpuverify.Verifier([0]), Workload())
    with open(out, "w") as f:
        json.dump({"steps": steps}, f, sort_keys=True, indent=1)
        f.write("\n")
    print(f"wrote {out}: {len(steps)} steps")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
