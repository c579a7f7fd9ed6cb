"""The pubkey index's host model for the tests, for both key arenas:
tools/fe29/kidx_host.cpp (g++ over csrc/gv_kidx.h, the source the kernels
compile) behind ctypes, a Model that mirrors what gv_keys_load / gv_keys_replace
(row=9: 33-byte keys) or gv_ed_keys_load / gv_ed_keys_replace (row=8: 32-byte
keys) do to one device's index, and the search for keys with a given home word
under the tests' fixed seed."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF          # the tests' "keys_index_seed" / "ed_keys_index_seed"
NONE = 0xFFFFFFFF
ROWS = {9: ("kidx_", 33), 8: ("edkidx_", 32)}      # row words -> the exports' prefix, the key's bytes

_lib = None


def load_model():
    """The one library: the exports of both row lengths."""
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(tempfile.mkdtemp(), "kidx_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so,
                    os.path.join(REPO, "tools", "fe29", "kidx_host.cpp")], check=True)
    L = ctypes.CDLL(so)
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    for row, (pre, _) in ROWS.items():
        for name, args, res in (("probe_bound", [], u32), ("row_words", [], u32),
                                ("rows", [vp, u32, u32, vp, vp], None), ("home", [vp, u64, u32], u32),
                                ("clear", [vp, u32], None), ("put", [vp, u32, vp, u32, u32, vp, u64], u32),
                                ("find", [vp, u32, vp, u32, u64, vp, u32, vp], u32),
                                ("search_home", [u64, u32, u32, u32, u64, u64, vp], u32)):
            f = getattr(L, pre + name)
            f.argtypes, f.restype = args, res
        assert getattr(L, pre + "row_words")() == row
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


def homed_keys(lib, T, home, want, stream=1, seed=SEED, row=9):
    """`want` distinct keys (33 bytes, or 32 for row=8) whose probe starts at table word `home` of T."""
    pre, kb = ROWS[row]
    out = np.zeros((want, kb), np.uint8)
    got = getattr(lib, pre + "search_home")(seed, T, home, want, stream, 1 << 26, _p(out))
    assert got == want, (got, want)
    assert len({k.tobytes() for k in out}) == want
    return out


class Model:
    """One device's index over a table of T words: load appends, replace
    rewrites rows and refills the table from every row."""

    def __init__(self, lib, T, seed=SEED, cap=None, row=9):
        pre, kb = ROWS[row]
        self.T, self.seed = T, seed
        self.rows_, self.clear_, self.put_, self.find_, self.home_ = (
            getattr(lib, pre + n) for n in ("rows", "clear", "put", "find", "home"))
        self.cap = cap or T
        self.keys = np.zeros((0, kb), np.uint8)
        self.rows = np.zeros(self.cap * row, np.uint32)
        self.table = np.full(T, NONE, np.uint32)
        self.left = 0

    def load(self, keys):
        keys = np.ascontiguousarray(keys, np.uint8)
        base, n = len(self.keys), len(keys)
        assert base + n <= self.cap
        self.keys = np.concatenate([self.keys, keys])
        self.rows_(_p(keys), n, base, None, _p(self.rows))
        self.left += self.put_(_p(self.table), self.T, _p(self.rows), n, base, None, self.seed)

    def replace(self, slots, keys):
        slots = np.ascontiguousarray(slots, np.uint32)
        keys = np.ascontiguousarray(keys, np.uint8)
        self.keys[slots] = keys
        self.rows_(_p(keys), len(slots), 0, _p(slots), _p(self.rows))
        self.clear_(_p(self.table), self.T)
        self.left = self.put_(_p(self.table), self.T, _p(self.rows), len(self.keys), 0, None, self.seed)

    def find(self, keys, count=None):
        keys = np.ascontiguousarray(keys, np.uint8)
        out = np.full(len(keys), 12345, np.uint32)
        self.find_(_p(self.table), self.T, _p(self.rows), len(self.keys) if count is None else count,
                   self.seed, _p(keys), len(keys), _p(out))
        return out

    def home(self, key):
        key = np.ascontiguousarray(key, np.uint8)
        return self.home_(_p(key), self.seed, self.T)
