"""The [s]B half of ed25519 verification at its edges, on the CPU (no GPU):
chosen-S signatures (tests/ed_chosen_s.py, built from the oracle alone)
through the device source compiled with g++ and the overflow traps
(tools/fe29/ed_host.cpp) -- the radix-256 comb of ed_ladder_check against the
full table, and ed_add_sb16 against a radix-2^16 table that holds ONLY the
16 entries the independent recoding names for the item: an entry the device
code asks for beyond those is (0, 0, 0), which forces X = Y = 0 and an
encoding of 32 zero bytes, so the item fails.  The same items then run on
the GPU routes (test_ed_chosen_s_gpu.py)."""
import ctypes
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

import ed_chosen_s as C
from oracle import ed25519_ref as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = E.P, E.L
PRE_WORDS = 27
BTAB16_ENTRIES = 32769
BTAB16_WORDS = 16 * BTAB16_ENTRIES * PRE_WORDS


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp()
    so = os.path.join(d, "ed_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so,
                    os.path.join(REPO, "tools", "fe29", "ed_host.cpp")], check=True)
    lb = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lb.edh_verify.argtypes = [vp, vp, vp, ctypes.c_uint32, vp]
    lb.edh_verify16.argtypes = [vp, vp, vp, ctypes.c_uint32, vp, vp]
    lb.edh_btab16_entry.argtypes = [ctypes.c_int, ctypes.c_int, vp]
    lb.edh_btab.argtypes = [vp]
    return lb


@pytest.fixture(scope="module")
def btab(lib):
    t = np.zeros(32 * 129 * PRE_WORDS, np.uint32)
    lib.edh_btab(t.ctypes.data)
    return t


class Sparse16:
    """a zeroed radix-2^16 table that holds, for one item at a time, only the
    entries (w, |d_w|) of recode(S, 16)"""

    def __init__(self, lib):
        self.lib = lib
        self.tab = np.zeros(BTAB16_WORDS, np.uint32)
        self.cache = {}

    def entry(self, w, j):
        if (w, j) not in self.cache:
            e = np.zeros(PRE_WORDS, np.uint32)
            self.lib.edh_btab16_entry(w, j, e.ctypes.data)
            self.cache[(w, j)] = e
        return self.cache[(w, j)]

    def verify(self, btab, items, i):
        named = [(w, abs(d)) for w, d in enumerate(C.recode(items.S[i], 16))]
        where = [(w * BTAB16_ENTRIES + j) * PRE_WORDS for w, j in named]
        for (w, j), o in zip(named, where):
            self.tab[o:o + PRE_WORDS] = self.entry(w, j)
        try:
            return host_verify(self.lib, btab, items, i, self.tab)
        finally:
            for o in where:
                self.tab[o:o + PRE_WORDS] = 0


@pytest.fixture(scope="module")
def sparse(lib):
    return Sparse16(lib)


def host_verify(lib, btab, items, i, btab16=None):
    pub, sig, msg = items.pub[i], items.sig[i], items.msg(i)
    mb = (ctypes.c_uint8 * max(1, len(msg)))(*msg)
    if btab16 is None:
        return bool(lib.edh_verify(pub.ctypes.data, sig.ctypes.data, mb, len(msg), btab.ctypes.data))
    return bool(lib.edh_verify16(pub.ctypes.data, sig.ctypes.data, mb, len(msg), btab.ctypes.data, btab16.ctypes.data))


def check(items, verdict, bits):
    assert not (items.sig[:, :32] == 0).all(axis=1).any(), "an R of 32 zero bytes: what a missing entry encodes to"
    bad = [i for i in range(len(items)) if verdict(i) != bool(items.want[i])]
    assert not bad, (len(bad), [items.describe(i, bits) for i in bad[:4]])


def val(limbs):
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


# ------------------------------------------------------------ the inputs
@pytest.mark.parametrize("bits", [16, 8])
def test_recode_balanced_digits(bits):
    nw, half, full = C.geometry(bits)
    rng = random.Random(bits)
    svals = C.edges() + [rng.randrange(L) for _ in range(200)]
    assert len(C.edges()) > 340 and all(0 <= s < L for s in svals)
    for s in svals:
        d = C.recode(s, bits)
        assert len(d) == nw and sum(x << (bits * w) for w, x in enumerate(d)) == s
        assert all(-half < x <= half for x in d)
        assert 0 <= d[-1] <= (0x1000 if bits == 16 else 16), hex(s)
    # the digit edges are really there: +half, -(half - 1), and a carry run through every window
    assert C.recode(half, bits)[0] == half and C.recode(half + 1, bits)[:2] == [-(half - 1), 1]
    assert C.recode((1 << (bits * (nw - 1))) - 1, bits) == [-1] + [0] * (nw - 2) + [1]


def test_item_sets_are_what_they_claim():
    for bits in (8, 16):
        nw, half, _ = C.geometry(bits)
        sw = C.sweeps(bits)
        assert [len(sw[k]) for k in C.SWEEPS] == [half + 1] * 3 + [(0x1000 if bits == 16 else 16) + 1]
        seen = {}
        for kind in C.SWEEPS:
            for s in sw[kind].S:
                for w, d in enumerate(C.recode(s, bits)):
                    seen.setdefault((w, d), kind)
        # every entry below the top window with each sign (-half is no balanced digit), every top entry of an S < L
        for w in range(nw - 1):
            assert all((w, j) in seen for j in range(-half + 1, half + 1)), (bits, w)
        assert all((nw - 1, t) in seen for t in range((0x1000 if bits == 16 else 16) + 1))
    tw = C.twins(C.edge_items())
    assert not tw.want.any() and tw.S == C.edge_items().S
    rng = random.Random(5)
    for i in rng.sample(range(len(tw)), 12):
        assert E.verify(C.IDENT_KEY, b"", bytes(C.edge_items().sig[i]))
        assert not E.verify(C.IDENT_KEY, b"", bytes(tw.sig[i]))
    t = C.torsion_items()
    assert len(set(bytes(p) for p in t.pub)) >= 10 and C.IDENT_KEY not in set(bytes(p) for p in t.pub)
    assert t.want[0::2].all() and 3 * int((t.want[1::2] == 0).sum()) >= len(t) // 2
    assert {L - 1} <= set(t.S) and len(set(t.S)) >= 28


@pytest.mark.parametrize("w", [0, 1, 7, 15])
def test_btab16_entries(lib, w):
    for j in (0, 1, 2, 3, 32767, 32768):
        ent = np.zeros(PRE_WORDS, np.uint32)
        lib.edh_btab16_entry(w, j, ent.ctypes.data)
        x, y = E.point_mul(j * 65536**w, E.B)
        got = (val(ent[0:9]) % P, val(ent[9:18]) % P, val(ent[18:27]) % P)
        assert got == ((y + x) % P, (y - x) % P, 2 * E.D * x * y % P), (w, j)
        if j == 0:
            assert got == (1, 1, 0)


def test_ed_btab16_live_is_documented():
    """the read-only option the GPU file leans on is where an integrator looks for it"""
    for rel in ("include/gpuverify.h", "cosmos-sdk-rootchain_amd/gpuverify.py", "INTEGRATION.md",
                "cosmos-sdk-rootchain_amd/csrc/gv_runtime.cpp"):
        assert "ed_btab16_live" in open(os.path.join(REPO, rel)).read(), rel


# ------------------------------------------------- radix-256 (ed_ladder_check)
def test_radix256_sweeps_and_twins(lib, btab):
    for kind, it in C.sweeps(8).items():
        for items in (it, C.twins(it)):
            check(items, lambda i: host_verify(lib, btab, items, i), 8)


def test_radix256_edges_identity_key(lib, btab):
    e = C.edge_items()
    for items in (e, C.twins(e)):
        check(items, lambda i: host_verify(lib, btab, items, i), 8)


def test_radix256_torsion_keys(lib, btab):
    t = C.torsion_items()
    check(t, lambda i: host_verify(lib, btab, t, i), 8)


# ------------------------------------------ radix-2^16 (ed_add_sb16), sparse table
def test_radix65536_sparse_table_rejects_an_unnamed_entry(lib, btab, sparse):
    """the sparse table does bite: with one named entry left out the item fails"""
    e = C.edge_items()
    i = e.S.index(L - 1)
    assert sparse.verify(btab, e, i)
    d = C.recode(L - 1, 16)
    o = (3 * BTAB16_ENTRIES + abs(d[3])) * PRE_WORDS
    keep = sparse.entry(3, abs(d[3])).copy()
    sparse.cache[(3, abs(d[3]))] = np.zeros(PRE_WORDS, np.uint32)
    try:
        assert not sparse.verify(btab, e, i)
    finally:
        sparse.cache[(3, abs(d[3]))] = keep
    assert not sparse.tab[o:o + PRE_WORDS].any()


def test_radix65536_edges_identity_key(lib, btab, sparse):
    e = C.edge_items()
    for items in (e, C.twins(e)):
        check(items, lambda i: sparse.verify(btab, items, i), 16)


def test_radix65536_torsion_keys(lib, btab, sparse):
    t = C.torsion_items()
    check(t, lambda i: sparse.verify(btab, t, i), 16)


def test_radix65536_sweeps_sampled(lib, btab, sparse):
    rng = random.Random(16)
    for kind, it in C.sweeps(16).items():
        n = len(it)
        js = sorted({j for j in (0, 1, 2, 32766, 32767, 32768) if j < n} | {0, 1, 2, n - 3, n - 2, n - 1}
                    | set(rng.sample(range(n), 64)))
        sub = C.take(it, js)
        for items in (sub, C.twins(sub)):
            check(items, lambda i: sparse.verify(btab, items, i), 16)
