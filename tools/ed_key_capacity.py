#!/usr/bin/env python3
"""Rate of device-resident keyed ed25519 batches per table radix of the arena.

One context on one GPU.  The bench's ed25519 shape: --n items (1M) over --keys
keys (4,096), messages of 300..399 bytes, 1/8 with a corrupted R byte, all in
device memory.  Per round (--rounds, alternating so the three share the box's
state) the arena is reset and reloaded under "ed_keys_wide" 0, 6 and 8 and
gv_dev_verify_ed25519_msgs_keyed is timed over the whole batch: --warmup
calls, a device synchronise, then --steps calls between two host clock reads,
the second after a device synchronise (the window is ~0.5 s at the default).
Beside each rate: the seconds of the gv_ed_keys_load of the --keys keys (wide
build included), the table bytes per key, "ed_kw_rb", the batches that ran
on wide tables and the verdict mismatches against construction.

The yardsticks the parent commit already has, same session, same buffers:
gv_verify_ed25519_msgs_keyed (host buffers, PCIe included, the radix-16
tables) and gv_dev_verify_ed25519_msgs (device-resident, in-batch key
grouping).  Prints one JSON line.

  python tools/ed_key_capacity.py
  python tools/ed_key_capacity.py --n 262144 --steps 100 --rounds 5
"""
import argparse
import ctypes as C
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

TABLE_BYTES = {0: 64 * 8 * 36 * 4, 6: 43 * 32 * 36 * 4, 8: 32 * 128 * 36 * 4}   # per key; 6 / 8 beside the radix-16 table


def workload(n, nkeys, seed, threads):
    """bench_extras.ed25519's batch: OpenSSL-signed items round-robin over nkeys seeds."""
    wl = bench.workload_lib()
    rng = np.random.default_rng(seed)
    lens = rng.integers(300, 400, size=n, dtype=np.uint32)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    blob = rng.integers(0, 256, size=int(lens.sum()), dtype=np.uint8)
    seeds = rng.integers(0, 256, size=(nkeys, 32), dtype=np.uint8)
    pub = np.zeros((n, 32), np.uint8)
    sig = np.zeros((n, 64), np.uint8)
    vp = C.c_void_p
    wl.gvw_ed25519_sign.argtypes = [C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, C.c_int]
    rc = wl.gvw_ed25519_sign(n, nkeys, seeds.ctypes.data, blob.ctypes.data, off.ctypes.data, lens.ctypes.data,
                             pub.ctypes.data, sig.ctypes.data, threads)
    assert rc == 0
    bad = rng.random(n) < 0.125
    sig[bad, 5] ^= 0x40                           # R no longer the encoding of [S]B - [h]A
    return pub, sig, blob, off, lens, ~bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 20, help="items per batch")
    ap.add_argument("--keys", type=int, default=4096, help="distinct keys")
    ap.add_argument("--steps", type=int, default=60, help="timed calls per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="rounds of ed_keys_wide 0 / 6 / 8")
    ap.add_argument("--host-steps", type=int, default=3, help="timed host-buffer calls (the PCIe-bound yardstick)")
    ap.add_argument("--seed", type=int, default=0xED)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the workload generator")
    args = ap.parse_args()
    n = args.n
    if args.keys < 1 or args.keys > n:
        ap.error("--keys must be in 1..--n")

    t0 = time.perf_counter()
    pub, sig, blob, off, lens, exp = workload(n, args.keys, args.seed, args.threads)
    uk, inv = np.unique(pub, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    t_work = time.perf_counter() - t0
    nw = (n + 63) // 64

    ver = gvm.Verifier([0])
    try:
        d_pub, d_sig, d_blob, d_off, d_len = (ver.dev_alloc(a.nbytes) for a in (pub, sig, blob, off, lens))
        for ptr, a in ((d_pub, pub), (d_sig, sig), (d_blob, blob), (d_off, off), (d_len, lens)):
            ver.dev_upload(ptr, a)
        d_slots, d_bits = ver.dev_alloc(4 * n), ver.dev_alloc(8 * nw)

        def timed(call, steps, warmup):
            for _ in range(warmup):
                call()
            ver.dev_sync()
            t = time.perf_counter()
            for _ in range(steps):
                call()
            ver.dev_sync()
            return n * steps / (time.perf_counter() - t)

        def mismatches():
            bits = np.zeros(nw, np.uint64)
            ver.dev_download(bits, d_bits)
            return int(np.count_nonzero(bench.unpack_bits(bits, n).astype(bool) != exp))

        rates = {0: [], 6: [], 8: []}
        loads = {0: [], 6: [], 8: []}
        info = {}
        for _ in range(args.rounds):
            for wide in (0, 6, 8):
                ver.set_option("ed_keys_wide", wide)
                ver.ed_keys_reset()
                t = time.perf_counter()
                slots = ver.ed_keys_load(uk)[inv].astype(np.uint32)
                loads[wide].append(time.perf_counter() - t)
                ver.dev_upload(d_slots, slots)
                w0 = ver.get_option("ed_keyed_wide")
                rates[wide].append(timed(lambda: ver.dev_verify_ed25519_keyed(0, n, d_slots, d_sig, d_blob, d_off, d_len,
                                                                              d_bits), args.steps, args.warmup))
                info[wide] = {"ed_kw_rb": ver.get_option("ed_kw_rb"), "ed_kw_keys": ver.get_option("ed_kw_keys"),
                              "wide_batches": ver.get_option("ed_keyed_wide") - w0, "mismatches": mismatches()}
        # the yardsticks: host buffers on the radix-16 tables, and the grouped device-resident route
        ver.set_option("ed_keys_wide", 0)
        ver.ed_keys_reset()
        slots = ver.ed_keys_load(uk)[inv].astype(np.uint32)
        host = ver.verify_batch_ed25519_keyed(slots, sig, (blob, off, lens))
        t = time.perf_counter()
        for _ in range(args.host_steps):
            ver.verify_batch_ed25519_keyed(slots, sig, (blob, off, lens))
        host_rate = n * args.host_steps / (time.perf_counter() - t)
        host_mism = int(np.count_nonzero(host.astype(bool) != exp))
        grouped = timed(lambda: ver.dev_verify_ed25519(0, n, d_pub, d_sig, d_blob, d_off, d_len, d_bits),
                        max(1, args.steps // 2), args.warmup)
        grouped_mism = mismatches()
        for ptr in (d_pub, d_sig, d_blob, d_off, d_len, d_slots, d_bits):
            ver.dev_free(ptr)
        ver.ed_keys_reset()
    finally:
        ver.close()

    med = {w: float(np.median(r)) for w, r in rates.items()}
    out = {"items": n, "keys": int(len(uk)), "mean_msg_bytes": round(float(lens.mean()), 1), "unit": "ed25519 verifies/s",
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "dev_keyed": {str(w): {"value": round(med[w], 1), "rates": [round(r, 1) for r in rates[w]],
                                  "vs_radix16": round(med[w] / med[0], 4),
                                  "load_s_per_%d_keys" % len(uk): round(float(np.median(loads[w])), 4),
                                  "loads_s": [round(x, 4) for x in loads[w]],
                                  "table_bytes_per_key": TABLE_BYTES[0] + (TABLE_BYTES[w] if w else 0), **info[w]}
                         for w in (0, 6, 8)},
           "host_keyed": {"value": round(host_rate, 1), "steps": args.host_steps, "mismatches": host_mism},
           "dev_grouped": {"value": round(grouped, 1), "steps": max(1, args.steps // 2), "mismatches": grouped_mism},
           "workload_s": round(t_work, 1)}
    print(json.dumps(out), flush=True)
    bad = host_mism + grouped_mism + sum(i["mismatches"] for i in info.values())
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
