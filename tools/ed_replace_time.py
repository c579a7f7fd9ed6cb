#!/usr/bin/env python3
"""Time of gv_ed_keys_replace beside gv_ed_keys_load on one device.

Two contexts on one build.  The first holds an arena of --arena (4,096) loaded
ed25519 keys; per n in --sizes a step replaces n of its slots (drawn afresh,
distinct) with n keys not seen before.  The second is reset before every load
and loads the same n keys into slots 0..n-1 of its empty arena, which is
allocated at --arena slots beforehand: no growth, so both calls run the same
kernels over the same n keys (the scratch allocation, the copies in, the key
build, the synchronise).  A third figure: gv_ed_keys_reset plus a reload of
all --arena keys, what a caller without replacement pays to change any slot.

Per n: --warmup untimed steps, then --runs steps; a step times one replace
and one load, each once, alternating, by the host clock around the call (both
end in a stream synchronise).  Medians, the 10th / 90th percentiles and the
ratio replace / load go out as one JSON line.  One process, one GPU.

  python tools/ed_replace_time.py
  python tools/ed_replace_time.py --sizes 1,40,150,4096 --runs 20 --split 0
"""
import argparse
import ctypes
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


def public_keys(n, seed):
    """n distinct OpenSSL ed25519 public keys (n x 32) from seeded private keys."""
    wl = bench.workload_lib()
    vp = ctypes.c_void_p
    wl.gvw_ed25519_sign.argtypes = [ctypes.c_size_t, ctypes.c_size_t, vp, vp, vp, vp, vp, vp, ctypes.c_int]
    sd = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    ln = np.ones(n, np.uint32)
    off = np.arange(n, dtype=np.uint64)
    blob = np.zeros(n, np.uint8)
    pub = np.zeros((n, 32), np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    assert wl.gvw_ed25519_sign(n, n, sd.ctypes.data, blob.ctypes.data, off.ctypes.data, ln.ctypes.data,
                               pub.ctypes.data, sig.ctypes.data, 8) == 0
    return pub


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def stats(ts):
    a = np.sort(np.array(ts))
    return {"p50_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4),
            "p90_ms": round(float(np.percentile(a, 90)), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena", type=int, default=4096)
    ap.add_argument("--sizes", default="1,40,150,4096")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--split", type=int, default=1, help='"ed_keys_split": 1 chain + table kernels, 0 one lane per key')
    ap.add_argument("--seed", type=int, default=0xED)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    if max(sizes) > args.arena:
        raise SystemExit("--sizes must not pass --arena")
    steps = args.warmup + args.runs
    resident = public_keys(args.arena, args.seed)
    rng = np.random.default_rng(args.seed + 1)
    out = {"arena": args.arena, "runs": args.runs, "warmup": args.warmup, "ed_keys_split": args.split, "sizes": {}}
    with gvm.Verifier([0]) as va, gvm.Verifier([0]) as vb:
        for v in (va, vb):
            v.set_option("ed_keys_split", args.split)
        va.ed_keys_load(resident)
        vb.ed_keys_load(resident)                     # the second arena at its full size, then empty
        vb.ed_keys_reset()
        gen = va.ed_keys_generation
        for n in sizes:
            fresh = public_keys(n * steps, args.seed + 2 + n).reshape(steps, n, 32)
            rep, load = [], []
            for k in range(steps):
                slots = rng.choice(args.arena, n, replace=False).astype(np.uint32)
                keys = np.ascontiguousarray(fresh[k])

                def do_replace():
                    va.ed_keys_replace(slots, keys)

                def do_load():
                    vb.ed_keys_load(keys)

                vb.ed_keys_reset()
                order = (do_replace, do_load) if k % 2 == 0 else (do_load, do_replace)
                t = {f: timed(f) for f in order}
                if k >= args.warmup:
                    rep.append(t[do_replace])
                    load.append(t[do_load])
                # the replaced slots hold the new keys (raw bytes read back from the device)
                if k == steps - 1:
                    assert np.array_equal(va.ed_keys_point(slots)[1], keys)
            r, ld = stats(rep), stats(load)
            out["sizes"][str(n)] = {"replace": r, "load": ld, "ratio": round(r["p50_ms"] / ld["p50_ms"], 3)}
        assert va.ed_keys_count == args.arena and va.ed_keys_generation == gen
        reload = []
        for k in range(steps):
            def do_reload():
                va.ed_keys_reset()
                va.ed_keys_load(resident)
            t = timed(do_reload)
            if k >= args.warmup:
                reload.append(t)
        out["reset_reload_all"] = stats(reload)
        out["ed_keys_replaced"] = va.get_option("ed_keys_replaced")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
