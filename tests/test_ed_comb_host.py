"""The signed comb-digit recoding of k_ed_keyed on the CPU (no GPU): the exact
device source (csrc/ed_scalar.cuh ed_comb_digit, built by g++ through
tools/fe29/ed_comb_host.cpp) at radix 2^4, 2^6 and 2^8 against Python
integers: the digits sum back to h, stay inside the table's entries and the
top window never carries out."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

from oracle import ed25519_ref as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NW = {4: 64, 6: 43, 8: 32}
TOP_MAX = {4: 1, 6: 1, 8: 17}       # h < L: bit 252 alone (4, 6); bits 248..252 (<= 16) and a carry (8)


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp()
    so = os.path.join(d, "ed_comb_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so,
                    os.path.join(REPO, "tools", "fe29", "ed_comb_host.cpp")], check=True)
    L = ctypes.CDLL(so)
    L.edc_recode.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int)]
    L.edc_recode.restype = ctypes.c_int
    return L


def recode(lib, rb, h):
    words = (ctypes.c_uint32 * 8)(*[(h >> (32 * i)) & 0xFFFFFFFF for i in range(8)])
    out = (ctypes.c_int * 64)(*([12345] * 64))
    nw = lib.edc_recode(rb, words, out)
    return nw, list(out)


def cases(rb):
    nw, ne = NW[rb], 1 << (rb - 1)
    low = range(nw - 1)                                  # the windows below the top one: h < 2^(rb (nw - 1)) <= 2^252 < L
    hs = [0, 1, E.L - 1]
    hs += [sum((ne - 1) << (rb * w) for w in low), sum(ne << (rb * w) for w in low)]     # every window at NE - 1 / at NE
    for w in low:                                        # each window alone at the carry boundary
        hs += [(ne - 1) << (rb * w), ne << (rb * w)]
    # 0x..7F7F80: the lowest window's carry ripples through every window; and the chain started higher up
    for start in (0, 1, nw // 2, nw - 2):
        hs.append((ne << (rb * start)) + sum((ne - 1) << (rb * w) for w in low if w > start))
    hs += [E.L - 2, E.L - (1 << 125), (1 << 252) - 1, 1 << 252, (1 << 252) + 1]          # the top window's edge below L
    rng = random.Random(1000 + rb)
    hs += [rng.randrange(E.L) for _ in range(200)]
    assert all(0 <= h < E.L for h in hs)
    return hs


@pytest.mark.parametrize("rb", [4, 6, 8])
def test_digits_sum_to_h_and_stay_in_the_table(lib, rb):
    nw, ne = NW[rb], 1 << (rb - 1)
    top_seen = set()
    for h in cases(rb):
        got_nw, dg = recode(lib, rb, h)
        assert got_nw == nw == (253 + rb - 1) // rb, (rb, got_nw)
        assert all(v == 12345 for v in dg[nw:]), "wrote past the windows"
        dg = dg[:nw]
        assert sum(v << (rb * w) for w, v in enumerate(dg)) == h, hex(h)
        assert all(-ne <= v < ne for v in dg), (hex(h), dg)
        assert 0 <= dg[-1] <= TOP_MAX[rb], (hex(h), dg[-1])
        top_seen.add(dg[-1])
    assert 0 in top_seen and max(top_seen) >= 1


def test_a_full_ripple_reaches_the_top_window(lib):
    """NE in window 0 under NE - 1 in every other low window: each digit goes
    negative and hands a carry on, the top window ends at exactly 1."""
    for rb in (4, 6, 8):
        nw, ne = NW[rb], 1 << (rb - 1)
        h = ne + sum((ne - 1) << (rb * w) for w in range(1, nw - 1))
        got_nw, dg = recode(lib, rb, h)
        assert got_nw == nw and dg[:nw] == [-ne] * (nw - 1) + [1]


def test_other_radices_are_refused(lib):
    words = (ctypes.c_uint32 * 8)()
    out = (ctypes.c_int * 64)()
    for rb in (0, 3, 5, 7, 9, 16):
        assert lib.edc_recode(rb, words, out) == -1
