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
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)       # the workload file: run one process's part
    ap.add_argument("--legacy", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.keys < 1 or args.keys > args.n or not 1 <= args.replace <= args.keys:
        ap.error("1 <= --replace <= --keys <= --n")
    if args.child:
        return child(args)

    import bench
    t0 = time.perf_counter()
    pub, sig, dig, exp = bench.make_digest_workload(args.n, args.seed, args.keys, 0.0, args.threads)
    dig[::8, 31] ^= 1                                          # both verdicts occur
    exp[::8] = 0
    tmp = tempfile.mkdtemp()
    wl = os.path.join(tmp, "workload.npz")
    np.savez(wl, pub=pub, sig=sig, dig=dig, exp=exp)
    t_work = time.perf_counter() - t0
    base = [sys.executable, os.path.abspath(__file__), "--child", wl, "--keys", str(args.keys), "--replace",
            str(args.replace), "--steps", str(args.steps), "--warmup", str(args.warmup)]
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
