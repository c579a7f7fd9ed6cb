#!/usr/bin/env python3
"""Grouped-route throughput against the share of keys that successive batches
have in common (option "group_reuse").

The headline bench verifies one batch over and over, so with the key-table
cache every timed step is a full hit.  Here the batches differ: each is 1M
signatures over 65,536 keys (16 per key, round-robin as in bench.py), and
batch t + 1 keeps a random `share` of batch t's keys and takes the rest from
a pool, least recently used first.  The pool is five batches' worth of keys
(327,680): a set's arena holds 209,920 rows and a set sees every other batch,
so at share 0 a key comes back only after its rows were flushed -- the line
that pays find, put and the periodic flush for nothing.

All batches are device-resident before the clock starts; `warm` batches run
first, the next `steps` are timed.  One JSON line per share.  GV_LIB picks
the library (a parent build has no "group_reuse_*" counters: null).

usage: group_reuse_rate.py [--pool FILE] [--label NAME] [--shares 0,50,90,100] [--warm 4] [--steps 12]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cosmos-sdk-rootchain_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import bench  # noqa: E402
import gpuverify as gvm  # noqa: E402

KEYS, PER_KEY, WINDOWS = 65_536, 16, 5


def load_pool(path, threads):
    """pub, sig, dig of WINDOWS * KEYS keys, PER_KEY valid signatures each (item i: key i % keys)."""
    if path and os.path.exists(path):
        z = np.load(path)
        return z["pub"], z["sig"], z["dig"]
    nk = WINDOWS * KEYS
    pub, sig, dig, exp = bench.make_digest_workload(nk * PER_KEY, 0x6E05E, nk, 0.0, threads)
    assert exp.all()
    if path:
        np.savez(path, pub=pub, sig=sig, dig=dig)
    return pub, sig, dig


def key_lists(share, count, rng):
    """`count` batches' key lists: each keeps share of the one before, the rest least recently used."""
    nk = WINDOWS * KEYS
    last = np.full(nk, -1, np.int64)
    cur = np.arange(KEYS)
    out = []
    for t in range(count):
        if t:
            keep = rng.choice(cur, int(round(share * KEYS)), replace=False)
            free = np.ones(nk, bool)
            free[cur] = False
            cand = np.nonzero(free)[0]
            cand = cand[np.argsort(last[cand] + rng.random(len(cand)), kind="stable")]
            cur = np.concatenate([keep, cand[:KEYS - len(keep)]])
            rng.shuffle(cur)
        last[cur] = t
        out.append(cur.copy())
    return out


def stat(ver, key):
    try:
        return ver.get_option(key)
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", help="npz file holding the signed pool (written when missing)")
    ap.add_argument("--shares", default="0,50,90,100")
    ap.add_argument("--label", default="", help="copied into every line (which library ran)")
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--threads", type=int, default=bench.host_cores()["effective"] or 1)
    args = ap.parse_args()
    pub, sig, dig = load_pool(args.pool, args.threads)
    nk, n = WINDOWS * KEYS, KEYS * PER_KEY
    words = (n + 63) // 64
    rng = np.random.default_rng(0x5A)
    count = args.warm + args.steps
    for pct in (int(s) for s in args.shares.split(",")):
        with gvm.Verifier([0]) as ver:                     # a context of its own: cold caches for every share
            bufs = [[ver.dev_alloc(n * w) for w in (33, 64, 32)] for _ in range(count)]
            d_bits = ver.dev_alloc(words * 8)
            lists = key_lists(pct / 100.0, count, rng)
            for ks, d in zip(lists, bufs):
                items = (ks[None, :] + nk * np.arange(PER_KEY)[:, None]).ravel()
                for p, a in zip(d, (pub, sig, dig)):
                    ver.dev_upload(p, np.ascontiguousarray(a[items]))
            seen = [len(np.intersect1d(lists[t], lists[t - 1])) / KEYS for t in range(1, count)]
            run = lambda d: ver.dev_verify_digests(0, n, d[0], d[1], d[2], d_bits)  # noqa: E731
            for d in bufs[:args.warm]:
                run(d)
            ver.dev_sync()
            c0 = [stat(ver, "group_reuse_" + k) for k in ("hit", "built", "reset")]
            g0 = ver.group_stats()
            t0 = time.perf_counter()
            for d in bufs[args.warm:]:
                run(d)
            ver.dev_sync()
            dt = time.perf_counter() - t0
            c1 = [stat(ver, "group_reuse_" + k) for k in ("hit", "built", "reset")]
            g1 = ver.group_stats()
            bits = np.zeros(words, np.uint64)
            ver.dev_download(bits, d_bits)
            ok = int(bench.unpack_bits(bits, n).sum())
            delta = [None if a is None else b - a for a, b in zip(c0, c1)]
            print(json.dumps({"share_pct": pct, "share_seen": round(float(np.mean(seen)), 4),
                              "verifies_per_s": round(n * args.steps / dt, 1),
                              "ms_per_batch": round(dt / args.steps * 1e3, 4), "steps": args.steps,
                              "grouped_batches": g1[0] - g0[0], "keys_built": g1[1] - g0[1],
                              "reuse_hit": delta[0], "reuse_built": delta[1], "reuse_reset": delta[2],
                              "last_batch_valid": ok, "label": args.label}), flush=True)
            assert ok == n, "every signature of the pool is valid"
            for p in [q for d in bufs for q in d] + [d_bits]:
                ver.dev_free(p)


if __name__ == "__main__":
    main()
