"""The ed25519 pubkey index's host model for the tests:
tools/fe29/edkidx_host.cpp (g++ over csrc/gv_kidx.h, the source the kernels
compile, at the 8-word ed25519 row) behind ctypes, a Model that mirrors what
gv_ed_keys_load / gv_ed_keys_replace do to one device's index, and the search
for keys with a given home word under the tests' fixed seed."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF          # the tests' "ed_keys_index_seed"
NONE = 0xFFFFFFFF
ROW = 8

_lib = None


def load_model():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(tempfile.mkdtemp(), "edkidx_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so,
                    os.path.join(REPO, "tools", "fe29", "edkidx_host.cpp")], check=True)
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.edkidx_probe_bound.restype = u32
    L.edkidx_row_words.restype = u32
    L.edkidx_rows.argtypes = [vp, u32, u32, vp, vp]
    L.edkidx_rows.restype = None
    L.edkidx_home.argtypes = [vp, u64, u32]
    L.edkidx_home.restype = u32
    L.edkidx_clear.argtypes = [vp, u32]
    L.edkidx_clear.restype = None
    L.edkidx_put.argtypes = [vp, u32, vp, u32, u32, vp, u64]
    L.edkidx_put.restype = u32
    L.edkidx_find.argtypes = [vp, u32, vp, u32, u64, vp, u32, vp]
    L.edkidx_find.restype = u32
    L.edkidx_search_home.argtypes = [u64, u32, u32, u32, u64, u64, vp]
    L.edkidx_search_home.restype = u32
    assert L.edkidx_row_words() == ROW
    _lib = L
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def table_words(cap):
    """kidx_table_words (csrc/gv_keytabs.h): a power of two, >= 2 cap and 512."""
    T = 512
    while T < 2 * cap:
        T <<= 1
    return T


def homed_keys(lib, T, home, want, stream=1, seed=SEED):
    """`want` distinct (32,) byte strings whose probe starts at table word `home` of T."""
    out = np.zeros((want, 32), np.uint8)
    got = lib.edkidx_search_home(seed, T, home, want, stream, 1 << 26, _p(out))
    assert got == want, (got, want)
    assert len({k.tobytes() for k in out}) == want
    return out


class Model:
    """One device's index over a table of T words: load appends, replace
    rewrites rows and refills the table from every row."""

    def __init__(self, lib, T, seed=SEED, cap=None):
        self.lib, self.T, self.seed = lib, T, seed
        self.cap = cap or T
        self.keys = np.zeros((0, 32), np.uint8)
        self.rows = np.zeros(self.cap * ROW, np.uint32)
        self.table = np.full(T, NONE, np.uint32)
        self.left = 0

    def load(self, keys):
        keys = np.ascontiguousarray(keys, np.uint8)
        base, n = len(self.keys), len(keys)
        assert base + n <= self.cap
        self.keys = np.concatenate([self.keys, keys])
        self.lib.edkidx_rows(_p(keys), n, base, None, _p(self.rows))
        self.left += self.lib.edkidx_put(_p(self.table), self.T, _p(self.rows), n, base, None, self.seed)

    def replace(self, slots, keys):
        slots = np.ascontiguousarray(slots, np.uint32)
        keys = np.ascontiguousarray(keys, np.uint8)
        self.keys[slots] = keys
        self.lib.edkidx_rows(_p(keys), len(slots), 0, _p(slots), _p(self.rows))
        self.lib.edkidx_clear(_p(self.table), self.T)
        self.left = self.lib.edkidx_put(_p(self.table), self.T, _p(self.rows), len(self.keys), 0, None, self.seed)

    def find(self, keys, count=None):
        keys = np.ascontiguousarray(keys, np.uint8)
        out = np.full(len(keys), 12345, np.uint32)
        self.lib.edkidx_find(_p(self.table), self.T, _p(self.rows), len(self.keys) if count is None else count,
                             self.seed, _p(keys), len(keys), _p(out))
        return out

    def home(self, key):
        key = np.ascontiguousarray(key, np.uint8)
        return self.lib.edkidx_home(_p(key), self.seed, self.T)
