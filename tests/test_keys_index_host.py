"""The resident key arena's pubkey index on the CPU (no GPU): the exact device
source (csrc/gv_kidx.h -- hash, probe sequence, insert, lookup -- built by g++
through tools/fe29/kidx_host.cpp) against a Python dict: every resident key is
found at its lowest slot, nothing is ever found at a slot with other bytes,
the probe wraps at the table's end and stops at GV_KIDX_PROBE.  The same
scenarios run once more as a program of their own under ASan + UBSan
(tests/kidx/kidx_harness.cpp)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from kidx_model import NONE, SEED, Model, homed_keys, load_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return load_model()


def rand_keys(rng, n):
    k = rng.integers(0, 256, (n, 33), dtype=np.uint8)
    k[:, 0] = 2 + (k[:, 0] & 1)
    return k


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


def test_random_keys_are_found_at_their_slots_and_unknown_keys_miss(lib):
    rng = np.random.default_rng(1)
    m = Model(lib, 8192)
    keys = rand_keys(rng, 2000)
    m.load(keys[:700])
    m.load(keys[700:])                                   # an append after the first load
    assert m.left == 0 and check(m) == 0
    assert np.array_equal(m.find(keys), np.arange(2000, dtype=np.uint32))
    assert np.all(m.find(rand_keys(rng, 500)) == NONE)


def test_keys_that_share_their_first_16_bytes(lib):
    """The hash covers the prefix and all 32 x bytes: 300 keys that differ only
    past byte 16 spread over the table (a hash of the head alone would put them
    on one probe run, longer than the bound)."""
    rng = np.random.default_rng(2)
    m = Model(lib, 8192)
    keys = np.repeat(rand_keys(rng, 1), 300, axis=0)
    keys[:, 17:] = rng.integers(0, 256, (300, 16), dtype=np.uint8)
    assert len({k.tobytes() for k in keys}) == 300
    m.load(keys)
    assert m.left == 0 and check(m) == 0
    assert len({m.home(k) for k in keys}) > 250


def test_one_byte_neighbours_are_different_keys(lib):
    rng = np.random.default_rng(3)
    a = rand_keys(rng, 1)[0]
    b, c, d = a.copy(), a.copy(), a.copy()
    a[0], b[0] = 2, 3                                    # the prefix alone
    c[32] ^= 1                                           # the last byte
    d[1] ^= 0x80                                         # the first x byte
    m = Model(lib, 512)
    m.load(np.array([a, b, c, d]))
    assert list(m.find(np.array([a, b, c, d]))) == [0, 1, 2, 3]
    for byte in range(33):                               # any other single byte: not resident
        e = a.copy()
        e[byte] ^= 4
        assert m.find(e[None])[0] == NONE


def test_duplicates_name_the_lowest_slot_and_the_next_after_a_replacement(lib):
    rng = np.random.default_rng(4)
    k, x, y = rand_keys(rng, 3)
    m = Model(lib, 512)
    m.load(np.array([x, k, y, k, k]))
    assert m.find(k[None])[0] == 1
    m.replace([1], rand_keys(rng, 1))
    assert m.find(k[None])[0] == 3 and check(m) == 0
    m.replace([4, 3], rand_keys(rng, 2))                 # the order of a replacement's slots does not matter
    assert m.find(k[None])[0] == NONE and check(m) == 0
    m.replace([0], k[None])
    assert m.find(k[None])[0] == 0 and m.find(x[None])[0] == NONE


def test_probe_wraps_from_the_last_word_to_word_0(lib):
    T = 512
    keys = homed_keys(lib, T, T - 1, 3)
    m = Model(lib, T)
    m.load(keys)
    assert [m.home(k) for k in keys] == [T - 1] * 3
    assert list(m.table[[T - 1, 0, 1]]) == [0, 1, 2] and np.count_nonzero(m.table != NONE) == 3
    assert list(m.find(keys)) == [0, 1, 2] and m.left == 0


def test_probe_bound_leaves_keys_out_and_they_miss(lib):
    T, P = 512, lib.kidx_probe_bound()
    assert P == 64
    keys = homed_keys(lib, T, 100, P + 6)
    m = Model(lib, T)
    m.load(keys)
    assert m.left == 6                                   # exactly the keys past the bound
    got = m.find(keys)
    assert np.array_equal(got[:P], np.arange(P, dtype=np.uint32))    # every placed key is found
    assert np.all(got[P:] == NONE)                       # the left-out ones miss
    assert check(m) == 6
    # a full window of other keys in front of it does not make a lookup return them
    assert np.all(m.find(rand_keys(np.random.default_rng(5), 200)) == NONE)
    # after the window's first key is replaced by a key homed elsewhere, one more fits
    other = homed_keys(lib, T, 300, 1)
    m.replace([0], other)
    assert m.left == 5 and check(m) == 5 and m.find(other)[0] == 0


def test_the_same_scenarios_under_asan_and_ubsan_as_a_program():
    d = tempfile.mkdtemp()
    exe = os.path.join(d, "kidx_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "kidx", "kidx_harness.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "\nkidx ok" in "\n" + out, out
    assert "Sanitizer" not in out and "runtime error" not in out, out


def test_seed_moves_the_home_words(lib):
    """Another seed, other home words: the set that overflows one probe window
    under SEED spreads out under SEED + 1."""
    keys = homed_keys(lib, 512, 100, 70)
    m = Model(lib, 512, seed=SEED + 1)
    m.load(keys)
    assert m.left == 0 and len({m.home(k) for k in keys}) > 50
