#!/usr/bin/env python3
"""Record what gv_set_option, gv_get_option and the GV_* option variables of a
libgpuverify.so do, as observed through a live context (needs a GPU):

    python tools/record_options.py PATH/libgpuverify.so [OUT.json]

writes tests/golden/options_parent.json (or OUT.json).  The fixture in the
tree was recorded from the library of the commit before the options moved
into csrc/gv_options.h; tests/test_options_gpu.py requires the current
library to reproduce it entry for entry, tests/test_options_host.py the
host-only table.

Per key (every key of the setter or the getter, and one unknown key): the
default read, then for each probe value the setter's return code and the
getter's return code and value for the key and for its coupled key; the key
goes back to its default afterwards.  Then three fresh child processes, one
after another, open a context with every option variable at "0", at "1" and
at an out-of-range or garbage value, and read every readable option."""
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cosmos-sdk-rootchain_amd"))

K_MAX_ITEMS = 0xFFFFFF00
MB_MAX = (2**64 - 1) >> 20
PROBES = ([-2**63, -1] + list(range(0, 13)) + [32, 33, 64, 65, 255, 256, 257, 1000, 1024, 1025,
          K_MAX_ITEMS, K_MAX_ITEMS + 1, 2**32 + 9, MB_MAX, MB_MAX + 1, 2**63 - 1])

# settable keys and the value that puts each back to its default
SETTABLE = {
    "lat_max": 8192, "lat_max_keyed": 14336, "lat_sl_max": 2048, "lat_sl_max_keyed": 1536,
    "ed_unc_lat_max": 2048, "ed_lat_max": 2048, "lat_zero_copy": 1, "lat_sliced": 1, "lat_rows_max": 512,
    "max_batch": 1 << 20, "pipe_chunk": 262144, "pipe_growth": 4, "stage_threads": 8, "stage_pieces": 2,
    "h2d_serial": 1, "gfull_item": 1, "inv_small": 1, "slice_plain_first": 0, "group_keys": 1,
    "group_min": 16384, "group_div": 5, "ed_btab16": 1, "ed_group_r64": 1, "ed_keys_split": 1, "ed_group": 1,
    "ed_group_min": 196608, "ed_keyed": 1, "ed_keys_wide": 0, "ed_keys_wide_mb": 0, "keys_wide": 2,
    "keys_index": 0, "keys_index_seed": 0, "kg": 0, "keys_wide_qw": 0, "keys_wide_mb": 0, "keys_wide1_cap": 0,
    "two_ladders": 1, "gfull": 1, "k6": 0, "keys_k6": 1, "async_chunk": 262144, "lat_kw": 1, "async_whole": 1,
    "async_growth": 1, "host_ladder_stream": 0, "key_cap": 1 << 22, "ed_key_cap": 1 << 16, "hbm_budget_mb": 0,
    "sort_keys": 1, "pipeline_dev": 1, "time_kernels": 0, "fault_inject": 0,
}
# a key whose accepted value is stored under a second key too, restored first
COUPLED = {"lat_max": "lat_max_keyed", "lat_sl_max": "lat_sl_max_keyed"}
READ_ONLY = ["keys_replaced", "ed_keys_replaced", "ed_keyed_wide", "keys_index_hit", "keys_index_miss",
             "keys_index_launches", "keys_index_find_ns", "kw_qw", "kwn_qw", "kw_arena_qw", "kw_arena_ng",
             "keys_index_live", "keys_index_keys", "keys_index_left_out", "keys_index_words", "ed_kw_rb",
             "ed_kw_keys"]
UNKNOWN = "no_such_option"
KEYS = list(SETTABLE) + READ_ONLY + [UNKNOWN]

# the option variables; the third child's out-of-range or garbage values
ENV_VARS = ["GV_MAX_BATCH", "GV_KEYED_K4", "GV_K6", "GV_KG", "GV_GFULL", "GV_TWO_LADDERS", "GV_KEYS_SCRATCH",
            "GV_SORT_KEYS", "GV_ED_KEYED", "GV_ED_GROUP", "GV_ED_KEYS_SPLIT", "GV_ED_BTAB16", "GV_ED_GROUP_R64",
            "GV_LAT_SLICED", "GV_LAT_ROWS_MAX", "GV_LAT_ZC", "GV_PIPELINE", "GV_GROUP_KEYS", "GV_STAGE_PIECES",
            "GV_SLICE_PLAIN_FIRST", "GV_INV_SMALL", "GV_GFULL_ITEM", "GV_H2D_SERIAL", "GV_LAT_KW", "GV_LANE_BURST",
            "GV_KEYS_K6", "GV_KEYS_WIDE", "GV_KEYS_WIDE_QW", "GV_KEYS_WIDE_MB", "GV_HOST_LADDER_STREAM",
            "GV_ASYNC_CHUNK", "GV_ASYNC_GROWTH", "GV_ASYNC_WHOLE", "GV_KEY_CAP", "GV_ED_KEY_CAP", "GV_ED_KEYS_WIDE",
            "GV_KEYS_INDEX", "GV_ED_KEYS_WIDE_MB", "GV_HBM_BUDGET_MB"]
GARBAGE = dict({v: "abc" for v in ENV_VARS}, GV_ASYNC_GROWTH="70", GV_STAGE_PIECES="70", GV_LANE_BURST="70",
               GV_ED_KEYS_WIDE="7", GV_KEYS_WIDE="7", GV_KEYS_WIDE_QW="10")
ENV_CHILDREN = {"zero": {v: "0" for v in ENV_VARS}, "one": {v: "1" for v in ENV_VARS}, "garbage": GARBAGE}


class Ctx:
    """A context on device 0 through the raw C ABI: return codes, not exceptions."""

    def __init__(self, lib_path=None):
        import gpuverify
        self.L = gpuverify.load(lib_path) if lib_path else gpuverify.load()
        self.ctx = ctypes.c_void_p()
        ids = (ctypes.c_int * 1)(0)
        rc = self.L.gv_open(ids, 1, ctypes.byref(self.ctx))
        if rc:
            raise RuntimeError(f"gv_open: {rc}")

    def close(self):
        self.L.gv_close(self.ctx)

    def set(self, key, val):
        return int(self.L.gv_set_option(self.ctx, key.encode(), ctypes.c_longlong(val)))

    def get(self, key):
        v = ctypes.c_longlong(0)
        rc = int(self.L.gv_get_option(self.ctx, key.encode(), ctypes.byref(v)))
        return [rc, int(v.value) if rc == 0 else None]


def probe_keys(c):
    """The setter / getter record of context c (opened with GV_EAGER_TABLES=0)."""
    out = {}
    for key in KEYS:
        other = COUPLED.get(key)
        rec = {"default": c.get(key), "coupled": other, "set": []}
        for val in PROBES:
            rc = c.set(key, val)
            if key == "keys_index_seed":           # the return code only
                rec["set"].append([rc, None, None])
            else:
                rec["set"].append([rc, c.get(key), c.get(other) if other else None])
        if key in SETTABLE:
            assert c.set(key, SETTABLE[key]) == 0, key
            if other:
                assert c.set(other, SETTABLE[other]) == 0, other
        out[key] = rec
    return out


def read_all(c):
    """Every readable option of context c."""
    got = {k: c.get(k) for k in KEYS}
    return {k: v[1] for k, v in got.items() if v[0] == 0}


def env_child(lib_path, env_values):
    """A fresh process with the option variables set: its readable options."""
    env = {k: v for k, v in os.environ.items() if k not in ENV_VARS}
    env.update(env_values, GV_EAGER_TABLES="0")
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + ([lib_path] if lib_path else [])
    r = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, timeout=120)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def record(lib_path=None):
    os.environ["GV_EAGER_TABLES"] = "0"
    c = Ctx(lib_path)
    try:
        keys = probe_keys(c)
    finally:
        c.close()
    env = {name: env_child(lib_path, values) for name, values in ENV_CHILDREN.items()}   # one at a time
    return {"probes": PROBES, "keys": keys, "env": env}


def main(argv):
    if argv[:1] == ["--child"]:
        c = Ctx(argv[1] if len(argv) > 1 else None)
        try:
            print(json.dumps(read_all(c)))
        finally:
            c.close()
        return 0
    if not argv:
        print(__doc__)
        return 2
    out = argv[1] if len(argv) > 1 else os.path.join(REPO, "tests", "golden", "options_parent.json")
    with open(out, "w") as f:
        json.dump(record(os.path.abspath(argv[0])), f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
