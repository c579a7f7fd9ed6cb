#!/usr/bin/env python3
"""What the key arena's pubkey index ("keys_index") buys a caller that stages
blocks on the GPU: device-resident digest batches of --n items over --keys keys
(C2's shape: 1M over 65,536), every key loaded, verified

  a  by gv_dev_verify_digests_keyed with the true slots      (the ceiling)
  b  by gv_dev_verify_digests with "keys_index" 1            (the new route)
  c  by gv_dev_verify_digests with "keys_index" 0            (today's route)
  d  as c, on a library built from the parent commit (--parent-lib)

--rounds (3) times, alternating: each round one fresh process on this commit's
library runs a, b, c in turn on one context, then one on the parent's runs d.
b counts as a gain only when its slowest run beats d's fastest (the boxes
spread +-3 %); c against d shows what the option costs while off.

Also reported, per process of this commit's library: gv_keys_load of all keys
and gv_keys_replace of --replace slots with the option off and on (arenas
already at capacity: the same kernels, no growth), and k_kidx_find's own time
over one batch from HIP events ("time_kernels", "keys_index_find_ns").

--miss M[,M...]: instead of the above, the same batch with M of its items
re-keyed to fresh keys that are NOT resident (valid signatures, at positions
spread evenly over the batch), per M and per process

  split  by gv_dev_verify_digests, "keys_index" 1, "keys_index_split" M
         (the resident items on the arena, the M others as a sub-batch)
  off    the same with "keys_index_split" 0: the whole batch falls through
         (on the parent's library: its only behaviour)

and, once per process, `resident`: the all-resident batch with "keys_index" 1.
The summary names the routes taken, the mismatches against construction and,
per M, whether split's slowest run beats the parent's fastest `off` by more
than the +-3 % box spread.

Timing as bench.py's timed loop: --warmup calls, a device synchronise, then
--steps pipelined calls between two host clock reads, the second after a
device synchronise.  One GPU.  Prints one JSON line per process and a summary.

  python tools/key_index_rate.py --parent-lib /path/to/parent/libgpuverify.so
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "cosmos-sdk-rootchain_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(ver, call, warmup, steps, n):
    for _ in range(warmup):
        call()
    ver.dev_sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    ver.dev_sync()
    return n * steps / (time.perf_counter() - t0)


def child(args):
    """One process, one context: a, b, c (this commit's library) or d (--legacy)."""
    import bench
    import gpuverify as gvm
    w = np.load(args.child)
    pub, sig, dig, exp = w["pub"], w["sig"], w["dig"], w["exp"]
    n, nkeys, R = len(exp), args.keys, args.replace
    keys = np.ascontiguousarray(pub[:nkeys])                 # item i: key i % nkeys
    out = {"lib": "parent" if args.legacy else "this", "items": n, "keys": nkeys}
    ver = gvm.Verifier([0])
    try:
        def load_and_replace(tag):
            ver.keys_reset()
            t0 = time.perf_counter()
            slots = ver.keys_load(keys)
            out["load_s_" + tag] = round(time.perf_counter() - t0, 4)
            victims = np.arange(R, dtype=np.uint32) * (nkeys // R)
            t0 = time.perf_counter()
            ver.keys_replace(victims, np.ascontiguousarray(keys[victims]))      # the same keys: verdicts unchanged
            out["replace_s_" + tag] = round(time.perf_counter() - t0, 4)
            return slots

        ver.keys_load(keys)                                   # untimed: the arenas reach their capacity
        slots_k = load_and_replace("index_off")
        if not args.legacy:
            ver.set_option("keys_index", 1)
            slots_k = load_and_replace("index_on")
            for k in ("live", "keys", "left_out", "words"):
                out["keys_index_" + k] = ver.get_option("keys_index_" + k)
        slots = np.ascontiguousarray(slots_k[np.arange(n) % nkeys], np.uint32)
        nw = (n + 63) // 64
        d_slots, d_pub, d_sig, d_dig = (ver.dev_alloc(a.nbytes) for a in (slots, pub, sig, dig))
        d_bits = ver.dev_alloc(nw * 8)
        for ptr, a in ((d_slots, slots), (d_pub, pub), (d_sig, sig), (d_dig, dig)):
            ver.dev_upload(ptr, a)

        def keyed():
            ver.dev_verify_digests_keyed(0, n, d_slots, d_sig, d_dig, d_bits)

        def plain():
            ver.dev_verify_digests(0, n, d_pub, d_sig, d_dig, d_bits)

        def run(name, call, index):
            if index is not None:
                ver.set_option("keys_index", index)
            r0 = ver.route_stats()
            rate = timed(ver, call, args.warmup, args.steps, n)
            r1 = ver.route_stats()
            bits = np.zeros(nw, np.uint64)
            ver.dev_download(bits, d_bits)
            out[name] = {"rate": round(rate, 1), "routes": {k: r1[k] - r0[k] for k in r1 if r1[k] != r0[k]},
                         "mismatches": int(np.count_nonzero(bench.unpack_bits(bits, n) != exp))}

        if args.legacy:
            run("d", plain, None)
        else:
            run("a", keyed, None)
            run("b", plain, 1)
            run("c", plain, 0)
            out["keys_index_hit"], out["keys_index_miss"] = (ver.get_option("keys_index_" + k) for k in ("hit", "miss"))
            # the lookup kernel alone, from HIP events (the timed stages serialise the pipeline: last)
            ver.set_option("keys_index", 1)
            ver.set_option("time_kernels", 1)
            ns = []
            for _ in range(5):
                plain()
                ver.dev_sync()
                ns.append(ver.get_option("keys_index_find_ns"))
            ver.set_option("time_kernels", 0)
            out["find_us"] = [round(v / 1000.0, 1) for v in ns]
        for ptr in (d_slots, d_pub, d_sig, d_dig, d_bits):
            ver.dev_free(ptr)
        ver.keys_reset()
    finally:
        ver.close()
    print(json.dumps(out), flush=True)
    return 1 if any(isinstance(v, dict) and v.get("mismatches") for v in out.values()) else 0


def spread(n, m):
    """m distinct positions spread evenly over n items."""
    return (np.arange(m, dtype=np.int64) * n) // m


def child_miss(args):
    """One process, one context: `resident`, then per M `split` and `off` (--legacy: `off` alone)."""
    import bench
    import gpuverify as gvm
    w = np.load(args.child)
    pub, sig, dig, exp = w["pub"], w["sig"], w["dig"], w["exp"]
    fpub, fsig, fdig = w["fpub"], w["fsig"], w["fdig"]
    n, nkeys = len(exp), args.keys
    out = {"lib": "parent" if args.legacy else "this", "items": n, "keys": nkeys}
    ver = gvm.Verifier([0])
    try:
        ver.set_option("keys_index", 1)
        ver.keys_load(np.ascontiguousarray(pub[:nkeys]))
        out["keys_index_live"] = ver.get_option("keys_index_live")
        out["keys_index_left_out"] = ver.get_option("keys_index_left_out")
        nw = (n + 63) // 64
        d_pub, d_sig, d_dig = (ver.dev_alloc(a.nbytes) for a in (pub, sig, dig))
        d_bits = ver.dev_alloc(nw * 8)

        def run(name, want, split):
            if split is not None:
                ver.set_option("keys_index_split", split)
            r0 = ver.route_stats()
            c0 = {k: ver.get_option("keys_index_" + k) for k in ("hit", "miss")}
            rate = timed(ver, lambda: ver.dev_verify_digests(0, n, d_pub, d_sig, d_dig, d_bits), args.warmup,
                         args.steps, n)
            r1 = ver.route_stats()
            bits = np.zeros(nw, np.uint64)
            ver.dev_download(bits, d_bits)
            out[name] = {"rate": round(rate, 1), "routes": {k: r1[k] - r0[k] for k in r1 if r1[k] != r0[k]},
                         "hit": ver.get_option("keys_index_hit") - c0["hit"],
                         "miss": ver.get_option("keys_index_miss") - c0["miss"],
                         "mismatches": int(np.count_nonzero(bench.unpack_bits(bits, n) != want))}

        for ptr, a in ((d_pub, pub), (d_sig, sig), (d_dig, dig)):
            ver.dev_upload(ptr, a)
        run("resident", exp, None)
        for m in args.miss_list:
            at = spread(n, m)
            p2, s2, g2, e2 = pub.copy(), sig.copy(), dig.copy(), exp.copy()
            p2[at], s2[at], g2[at], e2[at] = fpub[:m], fsig[:m], fdig[:m], 1
            for ptr, a in ((d_pub, p2), (d_sig, s2), (d_dig, g2)):
                ver.dev_upload(ptr, a)
            if not args.legacy:
                i0 = ver.get_option("keys_index_split_items")
                run("split_%d" % m, e2, m)
                out["split_%d" % m]["split_items"] = ver.get_option("keys_index_split_items") - i0
            run("off_%d" % m, e2, None if args.legacy else 0)
        for ptr in (d_pub, d_sig, d_dig, d_bits):
            ver.dev_free(ptr)
        ver.keys_reset()
    finally:
        ver.close()
    print(json.dumps(out), flush=True)
    return 1 if any(isinstance(v, dict) and v.get("mismatches") for v in out.values()) else 0


def summarise_miss(args, runs):
    this = [r for r in runs if r["lib"] == "this"]
    parent = [r for r in runs if r["lib"] == "parent"]
    rates = lambda rs, k: [r[k]["rate"] for r in rs if k in r]
    per_m = {}
    for m in args.miss_list:
        sp, off, par = rates(this, "split_%d" % m), rates(this, "off_%d" % m), rates(parent, "off_%d" % m)
        per_m[str(m)] = {"split": sp, "off": off, "parent": par,
                         "routes_split": next((r["split_%d" % m]["routes"] for r in this), None),
                         "routes_off": next((r["off_%d" % m]["routes"] for r in this), None),
                         "split_over_parent": round(float(np.median(sp) / np.median(par)), 4) if par else None,
                         "off_over_parent": round(float(np.median(off) / np.median(par)), 4) if par else None,
                         "split_over_resident": round(float(np.median(sp) / np.median(rates(this, "resident"))), 4),
                         # beats the fall-through by more than the +-3 % box spread
                         "split_beats_parent": bool(par and min(sp) > 1.03 * max(par))}
    res, pres = rates(this, "resident"), rates(parent, "resident")
    return {"items": args.n, "keys": args.keys, "steps": args.steps, "rounds": args.rounds, "unit": "verifies/s",
            "resident": res, "parent_resident": pres,
            "resident_over_parent": round(float(np.median(res) / np.median(pres)), 4) if pres else None,
            "miss": per_m,
            "mismatches": sum(v["mismatches"] for r in runs for v in r.values() if isinstance(v, dict))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default="", help="libgpuverify.so built from the parent commit (none: no d runs)")
    ap.add_argument("--n", type=int, default=1 << 20, help="items per batch")
    ap.add_argument("--keys", type=int, default=65536, help="distinct keys, all loaded")
    ap.add_argument("--replace", type=int, default=4096, help="slots per timed gv_keys_replace")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0xCA9)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the workload generator")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per process")
    ap.add_argument("--miss", default="", help="M[,M...]: batches with M non-resident items, split against fall-through")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)       # the workload file: run one process's part
    ap.add_argument("--legacy", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.keys < 1 or args.keys > args.n or not 1 <= args.replace <= args.keys:
        ap.error("1 <= --replace <= --keys <= --n")
    args.miss_list = [int(x) for x in args.miss.split(",") if x]
    if any(m < 1 or m > args.n for m in args.miss_list):
        ap.error("1 <= M <= --n")
    if args.child:
        return child_miss(args) if args.miss_list else child(args)

    import bench
    t0 = time.perf_counter()
    pub, sig, dig, exp = bench.make_digest_workload(args.n, args.seed, args.keys, 0.0, args.threads)
    dig[::8, 31] ^= 1                                          # both verdicts occur
    exp[::8] = 0
    tmp = tempfile.mkdtemp()
    wl = os.path.join(tmp, "workload.npz")
    extra = {}
    if args.miss_list:                                         # fresh keys (another seed) with valid signatures
        fpub, fsig, fdig, _ = bench.make_digest_workload(max(args.miss_list), args.seed + 1, max(args.miss_list), 0.0,
                                                         args.threads)
        resident = {k.tobytes() for k in pub[:args.keys]}
        assert not any(k.tobytes() in resident for k in fpub)
        extra = dict(fpub=fpub, fsig=fsig, fdig=fdig)
    np.savez(wl, pub=pub, sig=sig, dig=dig, exp=exp, **extra)
    t_work = time.perf_counter() - t0
    base = [sys.executable, os.path.abspath(__file__), "--child", wl, "--keys", str(args.keys), "--replace",
            str(args.replace), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    if args.miss_list:
        base += ["--miss", args.miss]
    runs, rc = [], 0
    try:
        for _ in range(args.rounds):
            for legacy in ([False, True] if args.parent_lib else [False]):
                env = dict(os.environ)
                if legacy:
                    env["GV_LIB"] = args.parent_lib
                else:
                    env.pop("GV_LIB", None)
                # a fresh child process per part: one that faults or hangs ends the whole run
                r = subprocess.run(base + (["--legacy"] if legacy else []), env=env, capture_output=True, text=True,
                                   timeout=args.timeout)
                sys.stderr.write(r.stderr[-2000:])
                if r.returncode not in (0, 1):
                    print(json.dumps({"error": "child exited %d" % r.returncode, "runs": runs}), flush=True)
                    return 2
                rc |= r.returncode
                line = r.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                runs.append(json.loads(line))
    finally:
        os.remove(wl)
        os.rmdir(tmp)
    if args.miss_list:
        print(json.dumps(summarise_miss(args, runs)), flush=True)
        return rc
    rates = {m: [r[m]["rate"] for r in runs if m in r] for m in "abcd"}
    this = [r for r in runs if r["lib"] == "this"]
    summary = {"items": args.n, "keys": args.keys, "steps": args.steps, "rounds": args.rounds, "unit": "verifies/s",
               "rates": rates, "routes": {m: next((r[m]["routes"] for r in runs if m in r), None) for m in "abcd"},
               "b_beats_d": bool(rates["b"] and rates["d"] and min(rates["b"]) > max(rates["d"])),
               "c_over_d": round(float(np.median(rates["c"]) / np.median(rates["d"])), 4) if rates["d"] else None,
               "b_over_a": round(float(np.median(rates["b"]) / np.median(rates["a"])), 4),
               "find_us": [r["find_us"] for r in this],
               "load_s": {t: [r["load_s_" + t] for r in this] for t in ("index_off", "index_on")},
               "replace_s": {t: [r["replace_s_" + t] for r in this] for t in ("index_off", "index_on")},
               "replace_slots": args.replace, "parent_load_s": [r["load_s_index_off"] for r in runs if r["lib"] == "parent"],
               "parent_replace_s": [r["replace_s_index_off"] for r in runs if r["lib"] == "parent"],
               "mismatches": sum(v["mismatches"] for r in runs for v in r.values() if isinstance(v, dict)),
               "workload_s": round(t_work, 1)}
    print(json.dumps(summary), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
