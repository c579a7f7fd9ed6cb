"""The runtime's option table on the CPU (no GPU): csrc/gv_options.h, built by
g++ through tests/options/options_harness.cpp.

Against tests/golden/options_parent.json (tools/record_options.py, recorded on
a GPU from the library before the options moved into the table) the table
must give, for every key it backs, the same setter return code and the same
getter return code and value for every probe value, and the same default.

The environment half of the fixture covers three value sets only, so
opt_from_env is also driven variable by variable, through a fake getenv, at
"0", "1", "2", "70", "255", "256", "abc" and the empty string.  The expected
member values below are transcribed from gv_open as it stood before the
change (its GV_* parsing, rule by rule): they rest on reading that code, not
on a run."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GV_OK, GV_EINVAL = 0, -1
SIZE_MAX = 2**64 - 1
ENV_VALUES = ["0", "1", "2", "70", "255", "256", "abc", ""]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("options") / "options_harness")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-o", exe,
                    os.path.join(REPO, "tests", "options", "options_harness.cpp")], check=True)

    def run(*args):
        out = subprocess.run([exe, *args], check=True, stdout=subprocess.PIPE).stdout.decode()
        return [line.split(" ") for line in out.splitlines()]
    return run


@pytest.fixture(scope="module")
def parent(golden_dir):
    with open(os.path.join(golden_dir, "options_parent.json")) as f:
        return json.load(f)


def test_rows_are_well_formed(harness):
    rows = harness("rows")
    names = [r[1] for r in rows if r[1] != "-"]
    envs = [r[2] for r in rows if r[2] != "-"]
    assert len(names) == len(set(names)) and len(names) >= 50
    assert len(envs) == len(set(envs)) and all(e.startswith("GV_") for e in envs)
    assert all(r[1] != "-" or r[2] != "-" for r in rows)          # a row has a key or a variable
    assert all(int(r[3]) in range(5) for r in rows)               # none, quiesce, ed_keys_mu, keys empty, pools
    assert all(r[4] in ("0", "1") for r in rows)


def test_table_reproduces_the_parent_fixture(harness, parent):
    probes = parent["probes"]
    lines = harness("probe", *[str(v) for v in probes])
    defaults = {l[1]: l for l in lines if l[0] == "default"}
    sets = {}
    for l in lines:
        if l[0] == "set":
            sets.setdefault(l[1], []).append([int(x) for x in l[2:]])
    backed = [k for k, rec in parent["keys"].items() if any(s[0] == GV_OK for s in rec["set"])]
    assert sorted(defaults) == sorted(backed)                     # the table backs exactly the settable keys
    for key in backed:
        rec = parent["keys"][key]
        _, _, other, rc, val = defaults[key]
        assert (other if other != "-" else None) == rec["coupled"], key
        assert [int(rc), int(val) if int(rc) == GV_OK else None] == rec["default"], key
        assert len(sets[key]) == len(probes)
        for (val, src, rc, v, crc, cv), want in zip(sets[key], rec["set"]):
            assert src == want[0], (key, val)
            if key == "keys_index_seed":                          # recorded for its return code only
                continue
            assert [rc, v if rc == GV_OK else None] == want[1], (key, val)
            if rec["coupled"]:
                assert [crc, cv if crc == GV_OK else None] == want[2], (key, val)


def _flag(names):        # on for anything but "0"
    return {n: [0, 1, 1, 1, 1, 1, 1, 1] for n in names}


# variable -> the member's value for each of ENV_VALUES (None: the default stays)
MB = 1 << 20
ENV_EXPECT = {
    **_flag(["GV_KEYED_K4", "GV_K6", "GV_GFULL", "GV_TWO_LADDERS", "GV_KEYS_SCRATCH", "GV_SORT_KEYS", "GV_ED_KEYED",
             "GV_ED_GROUP", "GV_ED_KEYS_SPLIT", "GV_ED_BTAB16", "GV_ED_GROUP_R64", "GV_LAT_SLICED", "GV_LAT_ZC",
             "GV_PIPELINE", "GV_GROUP_KEYS", "GV_INV_SMALL", "GV_GFULL_ITEM", "GV_H2D_SERIAL", "GV_LAT_KW",
             "GV_KEYS_K6", "GV_HOST_LADDER_STREAM", "GV_ASYNC_WHOLE"]),
    "GV_KEYS_INDEX": [0, 1, 0, 0, 0, 0, 0, 0],                    # on for exactly "1"
    "GV_MAX_BATCH": [None, None, None, None, None, 256, None, None],        # [256, kMaxItems], else ignored
    "GV_ASYNC_CHUNK": [None, None, None, None, None, 256, None, None],
    "GV_KEY_CAP": [None, None, None, None, None, 256, None, None],
    "GV_ED_KEY_CAP": [None, None, None, None, None, 256, None, None],
    "GV_KG": [0, None, None, None, None, None, 0, 0],             # atoi; 0 or a kg layout (4, 6, 7, 9)
    "GV_KEYS_WIDE": [0, 1, 2, None, None, None, 0, 0],            # atoi within [0, 2]
    "GV_KEYS_WIDE_QW": [0, None, None, None, None, None, 0, 0],   # atoi; 0 or a built width (9, 11)
    "GV_ED_KEYS_WIDE": [0, None, None, None, None, None, 0, 0],   # atoi; 0, 6 or 8
    "GV_LAT_ROWS_MAX": [0, 1, 2, 70, 255, 256, 0, 0],             # strtoull, unchecked
    "GV_SLICE_PLAIN_FIRST": [0, 1, 2, 70, 255, 256, 0, 0],
    "GV_STAGE_PIECES": [1, 1, 2, 70, 255, 256, 1, 1],             # max(1, atoi)
    "GV_LANE_BURST": [1, 1, 2, 70, 255, 256, 1, 1],
    "GV_ASYNC_GROWTH": [1, 1, 2, 64, 64, 64, 1, 1],               # atoi clamped to [1, 64]
    "GV_KEYS_WIDE_MB": [0, MB, 2 * MB, 70 * MB, 255 * MB, 256 * MB, 0, 0],   # atoll >= 0, stored in bytes
    "GV_ED_KEYS_WIDE_MB": [0, MB, 2 * MB, 70 * MB, 255 * MB, 256 * MB, 0, 0],
    "GV_HBM_BUDGET_MB": [None, MB, 2 * MB, 70 * MB, 255 * MB, 256 * MB, None, None],   # atoll > 0, in bytes
}
ENV_DEFAULT = {"GV_MAX_BATCH": 1 << 20, "GV_ASYNC_CHUNK": 262144, "GV_KEY_CAP": 1 << 22, "GV_ED_KEY_CAP": 1 << 16,
               "GV_KG": 0, "GV_KEYS_WIDE": 2, "GV_KEYS_WIDE_QW": 0, "GV_ED_KEYS_WIDE": 0,
               "GV_HBM_BUDGET_MB": SIZE_MAX}


@pytest.mark.parametrize("value", ENV_VALUES)
def test_each_option_variable_alone(harness, value):
    got = {l[1]: int(l[2]) % 2**64 for l in harness("env", value) if l[0] == "env"}
    assert sorted(got) == sorted(ENV_EXPECT)                      # every variable of the table, and no other
    i = ENV_VALUES.index(value)
    for name, want in ENV_EXPECT.items():
        w = want[i] if want[i] is not None else ENV_DEFAULT[name]
        assert got[name] == w, (name, value)
