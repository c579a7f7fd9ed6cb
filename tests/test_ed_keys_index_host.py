"""The ed25519 key arena's pubkey index on the CPU (no GPU): the exact device
source (csrc/gv_kidx.h at 8-word rows -- hash, probe sequence, insert, lookup
-- built by g++ through tools/fe29/kidx_host.cpp) against the load order:
every resident key is found at its lowest slot, nothing is ever found at a
slot with other bytes, the probe wraps at the table's end and stops at
GV_KIDX_PROBE.  The 9-word routines of the secp256k1 index give the home
words they gave before they became instances of the R-word templates
(tests/golden/kidx_home_parent.json), the option rows stand where
tests/golden/options_parent.json lets them, and the same scenarios run once
more as a program of their own under ASan + UBSan
(tests/kidx/kidx_harness.cpp)."""
import json
import os
import subprocess
import tempfile
from functools import partial

import numpy as np
import pytest

import kidx_model
from kidx_model import NONE, SEED, _p, load_model, table_words

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Model = partial(kidx_model.Model, row=8)                 # the ed25519 arena's rows
homed_keys = partial(kidx_model.homed_keys, row=8)
SAN = ["-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def lib():
    return load_model()


def rand_keys(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def one_bit_variants(keys):
    """Per key three neighbours: byte 0 bit 0, byte 31 bit 7 (the sign bit), byte 31 bit 0."""
    out = np.repeat(keys, 3, axis=0)
    out[0::3, 0] ^= 1
    out[1::3, 31] ^= 0x80
    out[2::3, 31] ^= 1
    return out


def check(m):
    """Every resident key finds its lowest slot -- or, only when keys were left
    out, nothing; never a slot with other bytes.  Returns the misses."""
    lowest = {}
    for s in range(len(m.keys) - 1, -1, -1):
        lowest[m.keys[s].tobytes()] = s
    got = m.find(np.array([np.frombuffer(k, np.uint8) for k in lowest]))
    miss = 0
    for (k, s), g in zip(lowest.items(), got):
        if g == NONE:
            miss += 1
        else:
            assert g == s and m.keys[g].tobytes() == k
    if m.left == 0:
        assert miss == 0
    return miss


def test_row_is_the_arena_row_and_the_bound_is_the_secp_index_s(lib):
    assert lib.edkidx_row_words() == 8 and lib.edkidx_probe_bound() == 64
    key = np.arange(32, dtype=np.uint8)
    rows = np.zeros(3 * 8, np.uint32)
    lib.edkidx_rows(_p(key), 1, 2, None, _p(rows))
    assert not rows[:16].any()
    assert list(rows[16:]) == [int.from_bytes(bytes(key[4 * i:4 * i + 4]), "little") for i in range(8)]
    assert [table_words(c) for c in (0, 1, 256, 257, 65536)] == [512, 512, 512, 1024, 131072]


def test_loads_of_1_255_256_257_keys_in_turn(lib):
    rng = np.random.default_rng(0xE1)
    pool = rand_keys(rng, 769)
    m = Model(lib, table_words(769))
    assert np.all(m.find(pool[:5]) == NONE)                           # the empty index
    lo = 0
    for n in (1, 255, 256, 257):
        m.load(pool[lo:lo + n])
        lo += n
        assert m.left == 0 and check(m) == 0
        assert np.array_equal(m.find(pool[:lo]), np.arange(lo, dtype=np.uint32))
        assert np.all(m.find(pool[lo:]) == NONE)                      # not loaded yet
    assert np.all(m.find(rand_keys(rng, 500)) == NONE)
    assert np.all(m.find(one_bit_variants(pool)) == NONE)


def test_all_32_bytes_enter_the_hash_and_the_comparison(lib):
    """300 keys that differ only in their last 4 bytes (the sign bit's word) spread
    over the table, and any single changed byte of a resident key is another key."""
    rng = np.random.default_rng(0xE2)
    keys = np.repeat(rand_keys(rng, 1), 300, axis=0)
    keys[:, 28:] = rng.integers(0, 256, (300, 4), dtype=np.uint8)
    assert len({k.tobytes() for k in keys}) == 300
    m = Model(lib, 8192)
    m.load(keys)
    assert m.left == 0 and check(m) == 0
    assert len({m.home(k) for k in keys}) > 250
    for byte in range(32):
        e = keys[0].copy()
        e[byte] ^= 4
        if e.tobytes() not in {k.tobytes() for k in keys}:
            assert m.find(e[None])[0] == NONE


def test_same_bytes_in_three_slots_name_the_lowest_then_the_next(lib):
    rng = np.random.default_rng(0xE3)
    keys = rand_keys(rng, 300)
    keys[200] = keys[17]
    keys[299] = keys[17]
    k = keys[17].copy()
    m = Model(lib, table_words(300))
    m.load(keys)
    want = np.arange(300, dtype=np.uint32)
    want[[200, 299]] = 17
    assert np.array_equal(m.find(keys), want) and m.left == 0
    m.replace([17], rand_keys(rng, 1))
    assert m.find(k[None])[0] == 200 and check(m) == 0
    m.replace([299, 200], rand_keys(rng, 2))                          # the order of a replacement's slots does not matter
    assert m.find(k[None])[0] == NONE and check(m) == 0
    m.replace([0], k[None])
    assert m.find(k[None])[0] == 0 and m.find(keys[0][None])[0] == NONE


def test_probe_wraps_from_the_last_word_to_word_0(lib):
    T = 512
    keys = homed_keys(lib, T, T - 1, 3)
    m = Model(lib, T)
    m.load(keys)
    assert [m.home(k) for k in keys] == [T - 1] * 3
    assert list(m.table[[T - 1, 0, 1]]) == [0, 1, 2] and np.count_nonzero(m.table != NONE) == 3
    assert list(m.find(keys)) == [0, 1, 2] and m.left == 0


def test_probe_bound_leaves_exactly_six_keys_out_and_they_miss(lib):
    T, P = 512, lib.edkidx_probe_bound()
    keys = homed_keys(lib, T, 100, P + 6)
    m = Model(lib, T)
    m.load(keys)
    assert m.left == 6                                                # exactly the keys past the bound
    got = m.find(keys)
    assert np.array_equal(got[:P], np.arange(P, dtype=np.uint32))     # every placed key is found
    assert np.all(got[P:] == NONE)                                    # the left-out ones miss
    assert check(m) == 6
    assert np.all(m.find(rand_keys(np.random.default_rng(0xE4), 200)) == NONE)
    other = homed_keys(lib, T, 300, 1)                                # one leaves the window: one more fits
    m.replace([0], other)
    assert m.left == 5 and check(m) == 5 and m.find(other)[0] == 0


def test_find_passes_over_a_slot_at_or_past_count(lib):
    rng = np.random.default_rng(0xE5)
    keys = rand_keys(rng, 40)
    keys[30] = keys[10]
    m = Model(lib, 512)
    m.load(keys)
    assert m.find(keys[20:21])[0] == 20
    assert m.find(keys[20:21], count=21)[0] == 20 and m.find(keys[20:21], count=20)[0] == NONE
    assert m.find(keys[10:11], count=10)[0] == NONE and m.find(keys[30:31], count=11)[0] == 10
    assert np.all(m.find(keys, count=0) == NONE)
    # passed over like another key's word, not like an empty one: on one probe
    # run, the keys in front of the cut are still found
    crowd = homed_keys(lib, 512, 7, 5, stream=3)
    c = Model(lib, 512)
    c.load(crowd)
    assert list(c.table[7:12]) == [0, 1, 2, 3, 4]
    assert list(c.find(crowd, count=3)) == [0, 1, 2, NONE, NONE]


def test_seed_moves_the_home_words(lib):
    keys = homed_keys(lib, 512, 100, 70)
    m = Model(lib, 512, seed=SEED + 1)
    m.load(keys)
    assert m.left == 0 and len({m.home(k) for k in keys}) > 50


def test_nine_word_routines_give_the_parents_home_words():
    """16 fixed (key, seed, T) triples recorded from tools/fe29/kidx_host.cpp
    before gv_kidx.h's routines became instances of the R-word templates."""
    with open(os.path.join(REPO, "tests", "golden", "kidx_home_parent.json")) as f:
        triples = json.load(f)["triples"]
    assert len(triples) == 16
    L = kidx_model.load_model()
    assert L.kidx_row_words() == 9 and L.kidx_probe_bound() == 64
    for t in triples:
        key = np.frombuffer(bytes.fromhex(t["key"]), np.uint8).copy()
        assert L.kidx_home(_p(key), t["seed"], t["T"]) == t["home"], t


def test_nine_word_model_still_behaves():
    """kidx_host.cpp over the templated header: put / find / the bound, as before."""
    L = kidx_model.load_model()
    keys = kidx_model.homed_keys(L, 512, 100, 70)
    m = kidx_model.Model(L, 512)
    m.load(keys)
    assert m.left == 6 and np.array_equal(m.find(keys)[:64], np.arange(64, dtype=np.uint32))
    assert np.all(m.find(keys)[64:] == NONE)


# ---------------------------------------------------------------- the option rows
EXPECT_ROWS = {
    "ed_keys_index found": "1", "ed_keys_index in kRows": "0", "ed_keys_index in kRowsLater": "1",
    "ed_keys_index env": "GV_ED_KEYS_INDEX", "ed_keys_index env rule": "1", "ed_keys_index readable": "1",
    "ed_keys_index effect": "ed_keys_mu",
    "ed_keys_index_seed found": "1", "ed_keys_index_seed in kRows": "0", "ed_keys_index_seed in kRowsLater": "1",
    "ed_keys_index_seed env": "-", "ed_keys_index_seed env rule": "0", "ed_keys_index_seed readable": "0",
    "ed_keys_index_seed effect": "ed_keys_empty",
    "default": "0",
    "set 0": "1 0", "set 1": "1 1",
    **{f"set {v}": "0 0" for v in (-2, -1, 2, 3, 6, 8, 255, 256, 1 << 32, (1 << 32) + 1, -(1 << 32))},
    "env '0'": "0 0", "env '1'": "1 0", "env '2'": "0 0", "env '11'": "0 0", "env 'abc'": "0 0", "env ''": "0 0",
    "env ' 1'": "0 0", "env 'true'": "0 0",
    "others": "0",
}


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_option_rows(flags):
    exe = os.path.join(tempfile.mkdtemp(), "edkidx_options")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", *flags,
                    "-I" + os.path.join(REPO, "cosmos-sdk-rootchain_amd", "csrc"),
                    os.path.join(REPO, "tests", "kidx", "options_harness.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and out.rstrip().endswith("options ok"), out
    assert "Sanitizer" not in out and "runtime error" not in out, out
    got = dict(line.split(" = ") for line in r.stdout.splitlines()[:-1])
    assert got == EXPECT_ROWS, {k: (got.get(k), EXPECT_ROWS.get(k)) for k in set(got) | set(EXPECT_ROWS)
                                if got.get(k) != EXPECT_ROWS.get(k)}


def test_new_rows_are_not_in_the_recorded_table():
    """tests/golden/options_parent.json pins kRows: none of the new keys is among them."""
    with open(os.path.join(REPO, "tests", "golden", "options_parent.json")) as f:
        parent = json.load(f)
    assert not [k for k in parent["keys"] if k.startswith("ed_keys_index")]


# ---------------------------------------------------------------- sanitizers (host code, a program of its own)
def test_the_same_scenarios_under_asan_and_ubsan_as_a_program():
    exe = os.path.join(tempfile.mkdtemp(), "kidx_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", *SAN, os.path.join(REPO, "tests", "kidx", "kidx_harness.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "edkidx ok" in out, out
    assert "Sanitizer" not in out and "runtime error" not in out, out
