#!/usr/bin/env python3
"""What the ed25519 arena's pubkey index ("ed_keys_index") buys a caller that
stages commits on the GPU: device-resident pub32 batches of --n items (1M) over
--keys keys (4,096), messages of 300..399 bytes, 1/8 with a corrupted R byte
(DESIGN section 4.3d's workload), every key loaded, verified

  parent    by gv_dev_verify_ed25519_msgs on a library built from the parent
            commit (--parent-lib): the yardstick, its repeats give the spread
  off_first by the same call on this commit's library, "ed_keys_index" 0, as the
            first thing its process does: the parent's position
  off       the same after routed0 / keyed0 have run, over the loaded arena
  routed0   ... "ed_keys_index" 1, the radix-16 tables      (the new route)
  routed8   ... "ed_keys_index" 1, "ed_keys_wide" 8
  keyed0/8  by gv_dev_verify_ed25519_msgs_keyed with the caller's slots: the
            ceiling -- the gap to routed0/8 is the lookup and its host wait
  miss1     routed8's call with ONE item on a key that is not resident: the
            whole batch falls through, so the gap to `off` is a wasted lookup
  lat64     64 items, one call at a time with a device synchronise after each:
            p50 of --lat-calls calls, routed against "ed_keys_index" 0

--rounds (3) times, alternating: each round one fresh process on the parent's
library, then one on this commit's.  A gain is claimed only where the route's
slowest run beats the parent's fastest.

Timing as bench.py's timed loop: --warmup calls, a device synchronise, then
--steps (60) calls between two host clock reads, the second after a device
synchronise.  Verdicts are compared with the construction (OpenSSL-signed, the
corrupted items false) over every item of every run, and
oracle/ed25519_ref.py decides --oracle-items (256) items of the batch spread
evenly, which must agree with the construction.  One GPU.  Prints one JSON
line per process and a summary.

  python tools/ed_key_index_rate.py --parent-lib /path/to/parent/libgpuverify.so
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
for p in (REPO, os.path.join(REPO, "cosmos-sdk-rootchain_amd"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def child(args):
    """One process, one context: this commit's routes, or (--legacy) the parent's one."""
    import bench
    import gpuverify as gvm
    w = np.load(args.child)
    pub, sig, blob, off, lens, exp = (w[k] for k in ("pub", "sig", "blob", "off", "lens", "exp"))
    n = len(exp)
    nw = (n + 63) // 64
    uk, inv = np.unique(pub, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    out = {"lib": "parent" if args.legacy else "this", "items": n, "keys": int(len(uk))}
    ver = gvm.Verifier([0])
    try:
        d_pub, d_sig, d_blob, d_off, d_len = (ver.dev_alloc(a.nbytes) for a in (pub, sig, blob, off, lens))
        for ptr, a in ((d_pub, pub), (d_sig, sig), (d_blob, blob), (d_off, off), (d_len, lens)):
            ver.dev_upload(ptr, a)
        d_slots, d_bits = ver.dev_alloc(4 * n), ver.dev_alloc(8 * nw)

        def plain(m=n):
            ver.dev_verify_ed25519(0, m, d_pub, d_sig, d_blob, d_off, d_len, d_bits)

        def keyed(m=n):
            ver.dev_verify_ed25519_keyed(0, m, d_slots, d_sig, d_blob, d_off, d_len, d_bits)

        def counters():
            if args.legacy:
                return {}
            c = {k: ver.get_option("ed_keys_index_" + k) for k in ("hit", "miss", "launches")}
            c["grouped"], c["wide"] = ver.group_stats()[0], ver.get_option("ed_keyed_wide")
            return c

        def run(name, call, want=exp):
            c0 = counters()
            for _ in range(args.warmup):
                call()
            ver.dev_sync()
            t = time.perf_counter()
            for _ in range(args.steps):
                call()
            ver.dev_sync()
            rate = n * args.steps / (time.perf_counter() - t)
            c1 = counters()
            bits = np.zeros(nw, np.uint64)
            ver.dev_download(bits, d_bits)
            out[name] = {"rate": round(rate, 1), "moved": {k: c1[k] - c0[k] for k in c1},
                         "mismatches": int(np.count_nonzero(bench.unpack_bits(bits, n).astype(bool) != want))}

        def latency(name, call):
            for _ in range(10):
                call(64)
                ver.dev_sync()
            us = []
            for _ in range(args.lat_calls):
                t = time.perf_counter()
                call(64)
                ver.dev_sync()
                us.append((time.perf_counter() - t) * 1e6)
            bits = np.zeros(1, np.uint64)
            ver.dev_download(bits, d_bits)
            out[name] = {"p50_us": round(float(np.median(us)), 1), "p90_us": round(float(np.percentile(us, 90)), 1),
                         "mismatches": int(np.count_nonzero(bench.unpack_bits(bits, 64).astype(bool) != exp[:64]))}

        if args.legacy:
            run("parent", plain)
            latency("lat64_parent", plain)
        else:
            run("off_first", plain)                  # the parent's position: a fresh process, an empty arena, option off
            for wide in (0, 8):
                ver.ed_keys_reset()
                ver.set_option("ed_keys_wide", wide)
                ver.set_option("ed_keys_index", 1)
                t = time.perf_counter()
                slots = ver.ed_keys_load(uk)[inv].astype(np.uint32)
                out["load_s_%d" % wide] = round(time.perf_counter() - t, 4)
                ver.dev_upload(d_slots, slots)
                out["index_%d" % wide] = {k: ver.get_option("ed_keys_index_" + k)
                                          for k in ("live", "keys", "left_out", "words")}
                out["index_%d" % wide]["ed_kw_rb"] = ver.get_option("ed_kw_rb")
                run("routed%d" % wide, plain)
                run("keyed%d" % wide, keyed)
                if wide == 0:
                    latency("lat64_routed", plain)
                    ver.set_option("ed_keys_index", 0)
                    run("off", plain)
                    latency("lat64_off", plain)
            # one item on a key no slot holds (its signature no longer verifies)
            at = n // 2
            p2, e2 = pub.copy(), exp.copy()
            p2[at] = np.frombuffer(bytes(range(1, 33)), np.uint8)
            assert not (uk == p2[at]).all(axis=1).any()
            e2[at] = False
            ver.dev_upload(d_pub, p2)
            run("miss1", plain, e2)
            ver.dev_upload(d_pub, pub)
        for ptr in (d_pub, d_sig, d_blob, d_off, d_len, d_slots, d_bits):
            ver.dev_free(ptr)
        ver.ed_keys_reset()
    finally:
        ver.close()
    print(json.dumps(out), flush=True)
    return 1 if any(isinstance(v, dict) and v.get("mismatches") for v in out.values()) else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default="", help="libgpuverify.so built from the parent commit (none: no yardstick)")
    ap.add_argument("--n", type=int, default=1 << 20, help="items per batch")
    ap.add_argument("--keys", type=int, default=4096, help="distinct keys, all loaded")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lat-calls", type=int, default=200, help="timed 64-item calls per latency figure")
    ap.add_argument("--oracle-items", type=int, default=256, help="items the Python oracle decides")
    ap.add_argument("--seed", type=int, default=0xED)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the workload generator")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per process")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)       # the workload file: run one process's part
    ap.add_argument("--legacy", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.keys < 1 or args.keys > args.n or args.n < 64:
        ap.error("1 <= --keys <= --n, --n >= 64")
    if args.child:
        return child(args)

    import ed_key_capacity
    from oracle import ed25519_ref as E
    t0 = time.perf_counter()
    pub, sig, blob, off, lens, exp = ed_key_capacity.workload(args.n, args.keys, args.seed, args.threads)
    t_work = time.perf_counter() - t0
    oracle_bad = 0
    for i in (np.arange(args.oracle_items, dtype=np.int64) * args.n) // max(1, args.oracle_items):
        msg = bytes(blob[int(off[i]):int(off[i]) + int(lens[i])])
        oracle_bad += E.verify(bytes(pub[i]), msg, bytes(sig[i])) != bool(exp[i])
    tmp = tempfile.mkdtemp()
    wl = os.path.join(tmp, "workload.npz")
    np.savez(wl, pub=pub, sig=sig, blob=blob, off=off, lens=lens, exp=exp)
    base = [sys.executable, os.path.abspath(__file__), "--child", wl, "--steps", str(args.steps), "--warmup",
            str(args.warmup), "--lat-calls", str(args.lat_calls)]
    runs, rc = [], 0
    try:
        for _ in range(args.rounds):
            for legacy in ([True, False] if args.parent_lib else [False]):
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
    names = ("parent", "off_first", "off", "routed0", "keyed0", "routed8", "keyed8", "miss1")
    rates = {m: [r[m]["rate"] for r in runs if m in r] for m in names}
    med = {m: float(np.median(v)) for m, v in rates.items() if v}
    par = rates["parent"]

    def over(a, b):
        return round(med[a] / med[b], 4) if a in med and b in med else None

    lat = {m: [r[m]["p50_us"] for r in runs if m in r] for m in ("lat64_parent", "lat64_off", "lat64_routed")}
    summary = {"items": args.n, "keys": args.keys, "mean_msg_bytes": round(float(lens.mean()), 1), "steps": args.steps,
               "warmup": args.warmup, "rounds": args.rounds, "unit": "ed25519 verifies/s", "rates": rates,
               "parent_spread": round((max(par) - min(par)) / med["parent"], 4) if par else None,
               "off_first_inside_parent_spread": bool(par and all(min(par) <= x <= max(par) for x in rates["off_first"])),
               "off_inside_parent_spread": bool(par and all(min(par) <= x <= max(par) for x in rates["off"])),
               "off_first_over_parent": over("off_first", "parent"), "off_over_parent": over("off", "parent"),
               "routed0_over_parent": over("routed0", "parent"), "routed8_over_parent": over("routed8", "parent"),
               "routed0_beats_parent": bool(par and min(rates["routed0"]) > max(par)),
               "routed8_beats_parent": bool(par and min(rates["routed8"]) > max(par)),
               "routed0_over_keyed0": over("routed0", "keyed0"), "routed8_over_keyed8": over("routed8", "keyed8"),
               "miss1_over_off": over("miss1", "off"), "miss1_over_parent": over("miss1", "parent"),
               "lat64_p50_us": lat,
               "moved": {m: next((r[m]["moved"] for r in runs if m in r and r["lib"] == "this"), None) for m in names},
               "index": next(({k: r[k] for k in ("index_0", "index_8", "load_s_0", "load_s_8")}
                              for r in runs if r["lib"] == "this"), None),
               "mismatches": sum(v["mismatches"] for r in runs for v in r.values()
                                 if isinstance(v, dict) and "mismatches" in v),
               "oracle_items": args.oracle_items, "oracle_disagrees_with_construction": int(oracle_bad),
               "workload_s": round(t_work, 1)}
    print(json.dumps(summary), flush=True)
    return rc | (1 if oracle_bad else 0)


if __name__ == "__main__":
    sys.exit(main())
