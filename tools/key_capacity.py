#!/usr/bin/env python3
"""Rate and layout of the resident key arena at a given number of keys.

Loads --keys distinct secp256k1 keys with gv_keys_load (in --load-chunk pieces:
the arena grows by doubling as on a node; 0 = one load) under the given
"keys_wide" / "keys_wide_qw" / "keys_wide_mb" options, then verifies a
device-resident keyed digest batch of --n items taken round-robin over the
keys, and prints one JSON line: the layout the arena took ("kw_arena_qw",
"kw_arena_ng"; both 0: no wide tables), the route the batch ran on,
gv_keys_count, the verdict mismatches against the workload's by-construction
verdicts (valid signatures, every 8th over a changed digest), and verifies/s.

Timing as bench.py's timed loop: --warmup calls, a device synchronise, then
--steps pipelined calls between two host clock reads, the second after a
device synchronise.  --repeat runs the timed loop that many times on the same
arena (the spread of one build on one device).  One process, one GPU.

--churn R --resident N: the arena as a cache.  Loads N keys, then per step
(--churn-steps) replaces the R residents loaded longest ago with R keys not
seen before (gv_keys_replace) and verifies --steps device-resident keyed
batches of --n items over the current residents.  Prints verifies/s (the median
over the steps), the layout after the churn, and keys/s of gv_keys_replace
beside keys/s of gv_keys_load for the same R keys into fresh slots of a second
context (reset before each load, its arena already at capacity: the same
kernels over the same chunks, without growth).

  python tools/key_capacity.py --keys 65536 --qw 11
  python tools/key_capacity.py --keys 500000 --qw 0 --load-chunk 65536
  python tools/key_capacity.py --churn 4096 --resident 65536
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "cosmos-sdk-rootchain_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench                      # noqa: E402
import gpuverify as gvm           # noqa: E402


def get_or(ver, key, default):
    """An option a library without the layout chain does not know."""
    try:
        return ver.get_option(key)
    except gvm.GpuVerifyError:
        return default


def churn(args):
    n, nres, R, S = args.n, args.resident, args.churn, args.churn_steps
    K = nres + R * S                                   # every key the run ever loads
    if K > n:
        raise SystemExit("--n must be at least --resident + --churn * --churn-steps")
    t0 = time.perf_counter()
    pub, sig, dig, exp = bench.make_digest_workload(n, args.seed, K, 0.0, args.threads)   # item i: key i % K
    dig[::8, 31] ^= 1
    exp[::8] = 0
    item_key = np.arange(n) % K
    keys = np.ascontiguousarray(pub[:K])
    t_work = time.perf_counter() - t0
    ver, ver2 = gvm.Verifier([0]), gvm.Verifier([0])
    try:
        for v in (ver, ver2):
            v.set_option("keys_wide", args.wide)
            v.set_option("keys_wide_qw", args.qw)
            v.set_option("keys_wide_mb", args.mb)
            v.keys_reset()
        slot_of = np.full(K, -1, np.int64)             # key -> slot, -1: not resident
        slot_of[:nres] = ver.keys_load(keys[:nres])
        ver2.keys_load(keys[:R])                       # the second context's arena at capacity before it is timed
        layout0 = (ver.get_option("kw_arena_qw"), ver.get_option("kw_arena_ng"))
        nw = (n + 63) // 64
        d_slots, d_sig, d_dig = (ver.dev_alloc(a) for a in (4 * n, 64 * n, 32 * n))
        d_bits = ver.dev_alloc(nw * 8)
        rates, t_rep, t_load, mism = [], [], [], 0
        r0 = ver.route_stats()
        for s in range(S):
            old = np.arange(s * R, (s + 1) * R) % K    # loaded longest ago
            new = np.arange(nres + s * R, nres + (s + 1) * R)
            victims = np.ascontiguousarray(slot_of[old], np.uint32)
            t0 = time.perf_counter()
            ver.keys_replace(victims, keys[new])
            t_rep.append(time.perf_counter() - t0)
            slot_of[new], slot_of[old] = victims, -1
            ver2.keys_reset()
            t0 = time.perf_counter()
            ver2.keys_load(keys[new])
            t_load.append(time.perf_counter() - t0)
            idx = np.resize(np.nonzero(slot_of[item_key] >= 0)[0], n)   # items on residents, repeated to n
            for ptr, a in ((d_slots, slot_of[item_key[idx]].astype(np.uint32)), (d_sig, sig[idx]), (d_dig, dig[idx])):
                ver.dev_upload(ptr, np.ascontiguousarray(a))
            for _ in range(args.warmup):
                ver.dev_verify_digests_keyed(0, n, d_slots, d_sig, d_dig, d_bits)
            ver.dev_sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ver.dev_verify_digests_keyed(0, n, d_slots, d_sig, d_dig, d_bits)
            ver.dev_sync()
            rates.append(n * args.steps / (time.perf_counter() - t0))
            bits = np.zeros(nw, np.uint64)
            ver.dev_download(bits, d_bits)
            mism += int(np.count_nonzero(bench.unpack_bits(bits, n) != exp[idx]))
        r1 = ver.route_stats()
        routes = {k: r1[k] - r0[k] for k in r1 if r1[k] != r0[k]}
        rep, load = R / float(np.median(t_rep)), R / float(np.median(t_load))
        out = {"resident": nres, "churn": R, "churn_steps": S, "items": n, "keys_wide": args.wide,
               "keys_wide_qw": args.qw, "keys_wide_mb": args.mb, "layout_before": layout0,
               "kw_arena_qw": ver.get_option("kw_arena_qw"), "kw_arena_ng": ver.get_option("kw_arena_ng"),
               "route": max(routes, key=routes.get) if routes else None, "routes": routes,
               "keys_count": ver.keys_count, "keys_replaced": ver.get_option("keys_replaced"), "mismatches": mism,
               "value": round(float(np.median(rates)), 1), "unit": "verifies/s", "rates": [round(r, 1) for r in rates],
               "replace_keys_per_s": round(rep, 1), "load_keys_per_s": round(load, 1),
               "replace_over_load": round(rep / load, 3), "steps": args.steps, "warmup": args.warmup,
               "workload_s": round(t_work, 1)}
        for ptr in (d_slots, d_sig, d_dig, d_bits):
            ver.dev_free(ptr)
    finally:
        ver.close()
        ver2.close()
    print(json.dumps(out), flush=True)
    return 1 if out["mismatches"] else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keys", type=int, default=0, help="distinct keys to load")
    ap.add_argument("--churn", type=int, default=0, help="keys replaced per step (with --resident)")
    ap.add_argument("--resident", type=int, default=0, help="resident keys of the churn run")
    ap.add_argument("--churn-steps", type=int, default=8, help="replacement steps of the churn run")
    ap.add_argument("--qw", type=int, default=0, help='"keys_wide_qw": 0 (the chain), 11 or 9')
    ap.add_argument("--wide", type=int, default=2, help='"keys_wide": 2, 1 or 0')
    ap.add_argument("--mb", type=int, default=0, help='"keys_wide_mb" (0: no limit)')
    ap.add_argument("--n", type=int, default=1 << 20, help="items per batch")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=1, help="timed loops on the same arena")
    ap.add_argument("--load-chunk", type=int, default=0, help="keys per gv_keys_load call (0: all at once)")
    ap.add_argument("--seed", type=int, default=0xCA9)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the workload generator")
    ap.add_argument("--legacy", action="store_true",
                    help="a library without keys_wide_qw / keys_wide_mb: set neither (comparison runs)")
    args = ap.parse_args()
    if args.churn or args.resident:
        if args.churn < 1 or args.resident < args.churn:
            ap.error("--churn R --resident N with 1 <= R <= N")
        return churn(args)
    if args.keys < 1 or args.keys > args.n:
        ap.error("--keys must be in 1..--n (every key is used by an item)")

    n, nkeys = args.n, args.keys
    t0 = time.perf_counter()
    # item i is signed by key i % nkeys (no adversarial items: pub[:nkeys] are the
    # distinct keys); every 8th digest then gets a flipped bit, so both verdicts occur
    pub, sig, dig, exp = bench.make_digest_workload(n, args.seed, nkeys, 0.0, args.threads)
    assert np.array_equal(pub, pub[np.arange(n) % nkeys])
    dig[::8, 31] ^= 1
    exp[::8] = 0
    t_work = time.perf_counter() - t0

    ver = gvm.Verifier([0])
    try:
        ver.set_option("keys_wide", args.wide)
        if not args.legacy:
            ver.set_option("keys_wide_qw", args.qw)
            ver.set_option("keys_wide_mb", args.mb)
        ver.keys_reset()
        step = args.load_chunk or nkeys
        t0 = time.perf_counter()
        slots_k = np.concatenate([ver.keys_load(np.ascontiguousarray(pub[c:min(c + step, nkeys)]))
                                  for c in range(0, nkeys, step)])
        t_load = time.perf_counter() - t0
        slots = np.ascontiguousarray(slots_k[np.arange(n) % nkeys], np.uint32)
        nw = (n + 63) // 64
        d_slots, d_sig, d_dig = (ver.dev_alloc(a.nbytes) for a in (slots, sig, dig))
        d_bits = ver.dev_alloc(nw * 8)
        for ptr, a in ((d_slots, slots), (d_sig, sig), (d_dig, dig)):
            ver.dev_upload(ptr, a)

        def call():
            ver.dev_verify_digests_keyed(0, n, d_slots, d_sig, d_dig, d_bits)

        r0 = ver.route_stats()
        for _ in range(args.warmup):
            call()
        ver.dev_sync()
        rates = []
        for _ in range(args.repeat):
            ver.dev_sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                call()
            ver.dev_sync()
            rates.append(n * args.steps / (time.perf_counter() - t0))
        r1 = ver.route_stats()
        bits = np.zeros(nw, np.uint64)
        ver.dev_download(bits, d_bits)
        got = bench.unpack_bits(bits, n)
        routes = {k: r1[k] - r0[k] for k in r1 if r1[k] != r0[k]}
        out = {"keys": nkeys, "items": n, "keys_wide": args.wide, "keys_wide_qw": args.qw, "keys_wide_mb": args.mb,
               "load_chunk": args.load_chunk, "kw_arena_qw": get_or(ver, "kw_arena_qw", None),
               "kw_arena_ng": get_or(ver, "kw_arena_ng", None), "route": max(routes, key=routes.get) if routes else None,
               "routes": routes, "keys_count": ver.keys_count, "mismatches": int(np.count_nonzero(got != exp)),
               "value": round(float(np.median(rates)), 1), "unit": "verifies/s",
               "rates": [round(r, 1) for r in rates], "steps": args.steps, "warmup": args.warmup,
               "keys_load_s": round(t_load, 3), "workload_s": round(t_work, 1)}
        for ptr in (d_slots, d_sig, d_dig, d_bits):
            ver.dev_free(ptr)
        ver.keys_reset()
    finally:
        ver.close()
    print(json.dumps(out), flush=True)
    return 1 if out["mismatches"] else 0


if __name__ == "__main__":
    sys.exit(main())
