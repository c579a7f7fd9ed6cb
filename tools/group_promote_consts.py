#!/usr/bin/env python3
"""The two constants behind the grouped route's layout promotion (option
"group_promote"): what a key costs more to build in a kg
layout than in k4's, and what an item saves on the kg ladder.

One C2 batch (1M signatures over 65,536 keys), device-resident, serialized
("pipeline_dev" 0) with kernel events on.  Per layout (option "kg": 0 = k4, then
the many-group layouts) the batch runs with "group_reuse" off -- every call
builds every key: the key stage's time with the build -- and with it on, warm:
the same stage without.  One JSON line per layout: the four stage times
[unpack+dedupe, s^-1 | key tables, prep, ladder] of both, the build's time per
key and the ladder's per item.  GV_LIB picks the library.

usage: group_promote_consts.py [--ngs 0,6,7,9] [--warm 3] [--steps 10] [--label NAME]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "cosmos-sdk-rootchain_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import bench  # noqa: E402
import gpuverify as gvm  # noqa: E402

N, KEYS = 1 << 20, 65_536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ngs", default="0,6,7,9")
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--label", default="")
    ap.add_argument("--threads", type=int, default=bench.host_cores()["effective"] or 1)
    args = ap.parse_args()
    pub, sig, dig, exp = bench.make_digest_workload(N, 0xC2, KEYS, 0.0, args.threads)
    words = (N + 63) // 64
    for ng in (int(s) for s in args.ngs.split(",")):
        with gvm.Verifier([0]) as ver:
            d = [ver.dev_alloc(a.nbytes) for a in (pub, sig, dig)]
            for p, a in zip(d, (pub, sig, dig)):
                ver.dev_upload(p, a)
            d_bits = ver.dev_alloc(words * 8)
            try:
                ver.set_option("group_promote", 0)         # (a library without the option: nothing to switch off)
            except gvm.GpuVerifyError:
                pass
            ver.set_option("kg", ng)
            ver.set_option("pipeline_dev", 0)
            ver.set_option("time_kernels", 1)
            out = {"kg": ng, "n": N, "keys": KEYS, "steps": args.steps, "label": args.label}
            for name, reuse in (("build", 0), ("warm", 1)):
                ver.set_option("group_reuse", reuse)
                for _ in range(args.warm):
                    ver.dev_verify_digests(0, N, d[0], d[1], d[2], d_bits)
                ver.dev_sync()
                ver.stage_stats4()
                g0 = ver.group_stats()
                for _ in range(args.steps):
                    ver.dev_verify_digests(0, N, d[0], d[1], d[2], d_bits)
                ver.dev_sync()
                cnt, ms = ver.stage_stats4()
                g1 = ver.group_stats()
                out[name + "_stage_ms"] = [round(float(x), 4) for x in ms]
                out[name + "_keys_built_per_call"] = (g1[1] - g0[1]) / max(1, g1[0] - g0[0])
                assert cnt == args.steps
            bits = np.zeros(words, np.uint64)
            ver.dev_download(bits, d_bits)
            assert np.array_equal(bench.unpack_bits(bits, N), exp)
            out["build_ns_per_key"] = round((out["build_stage_ms"][1] - out["warm_stage_ms"][1]) * 1e6 / KEYS, 3)
            out["ladder_ns_per_item"] = round(out["warm_stage_ms"][3] * 1e6 / N, 4)
            print(json.dumps(out), flush=True)
            for p in d + [d_bits]:
                ver.dev_free(p)


if __name__ == "__main__":
    main()
