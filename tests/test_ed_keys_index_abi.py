"""CPU tests of the gv_ed_keys_find / gv_dev_ed_keys_find boundary and the
"ed_keys_index" options: the symbols answer without a GPU, and the Python
wrappers check shapes, dtypes and pointers before they call."""
import ctypes
import os
import re

import numpy as np
import pytest

import gpuverify as gvm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_null_context_is_einval_without_gpu():
    L = gvm.load()
    pub = np.zeros((2, 32), np.uint8)
    out = np.full(2, 7, np.uint32)
    assert L.gv_ed_keys_find(None, 2, _p(pub), _p(out)) == gvm.GV_EINVAL
    assert L.gv_ed_keys_find(None, 0, None, None) == gvm.GV_EINVAL
    vp = ctypes.c_void_p
    assert L.gv_dev_ed_keys_find(None, 0, 2, vp(256), vp(512), None) == gvm.GV_EINVAL
    assert L.gv_dev_ed_keys_find(None, 0, 0, None, None, None) == gvm.GV_EINVAL
    assert list(out) == [7, 7]


def test_library_exports_and_header_declares_both_calls():
    L = gvm.load()
    for name in ("gv_ed_keys_find", "gv_dev_ed_keys_find"):
        assert name in gvm.EXPORTED_SYMBOLS and hasattr(L, name)
    with open(os.path.join(REPO, "include", "gpuverify.h")) as f:
        hdr = f.read()
    assert re.search(r"int gv_ed_keys_find\(gv_ctx\* ctx, size_t n, const uint8_t\* pub32, uint32_t\* slot_out\);", hdr)
    assert re.search(r"int gv_dev_ed_keys_find\(gv_ctx\* ctx, int dev_slot, size_t n, const void\* d_pub32,\s*"
                     r"void\* d_slot_out, void\* stream\);", hdr)


@pytest.mark.parametrize("key", ["ed_keys_index", "ed_keys_index_seed"])
def test_options_are_refused_without_a_context(key):
    L = gvm.load()
    assert L.gv_set_option(None, key.encode(), 1) == gvm.GV_EINVAL
    v = ctypes.c_longlong(7)
    assert L.gv_get_option(None, key.encode(), ctypes.byref(v)) == gvm.GV_EINVAL and v.value == 7


@pytest.mark.parametrize("key", ["ed_keys_index_live", "ed_keys_index_keys", "ed_keys_index_left_out",
                                 "ed_keys_index_hit", "ed_keys_index_miss", "ed_keys_index_words",
                                 "ed_keys_index_launches"])
def test_read_only_options_are_refused_without_a_context(key):
    L = gvm.load()
    v = ctypes.c_longlong(7)
    assert L.gv_get_option(None, key.encode(), ctypes.byref(v)) == gvm.GV_EINVAL and v.value == 7
    assert L.gv_set_option(None, key.encode(), 0) == gvm.GV_EINVAL


class _NoCall:
    """Stands in for the loaded library: any call is a test failure."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} called before the argument checks")


def _wrapper_only():
    v = gvm.Verifier.__new__(gvm.Verifier)             # no gv_open: only the wrapper's own checks run
    v._L, v._ctx, v._inflight = _NoCall(), None, {}
    return v


@pytest.mark.parametrize("pub", [
    np.zeros(32, np.uint8),                            # one key, not (1, 32)
    np.zeros((2, 33), np.uint8),                       # secp256k1 keys
    np.zeros((2, 31), np.uint8),
    np.zeros((2, 32), np.int8),                        # not bytes
    np.zeros((2, 32), np.uint32),
    np.zeros((2, 32), np.float64),
    np.zeros((2, 4, 8), np.uint8),
    [b"\x02" * 32],
])
def test_ed_keys_find_wrapper_checks_before_any_call(pub):
    with pytest.raises(ValueError):
        _wrapper_only().ed_keys_find(pub)


def test_ed_keys_find_wrapper_empty_call_is_a_no_op():
    out = _wrapper_only().ed_keys_find(np.zeros((0, 32), np.uint8))
    assert out.shape == (0,) and out.dtype == np.uint32


@pytest.mark.parametrize("kw", [
    dict(n=-1), dict(n=2.0), dict(n=True), dict(slot="0"), dict(slot=False), dict(d_pub=1.5), dict(d_pub=-32),
    dict(d_pub=None), dict(d_pub=0), dict(d_slots_out=None), dict(d_slots_out=0), dict(d_slots_out=514),
    dict(d_slots_out=513), dict(d_slots_out="512"), dict(d_slots_out=[512]), dict(stream=-1), dict(stream=2.0),
])
def test_dev_ed_keys_find_wrapper_checks_before_any_call(kw):
    args = dict(slot=0, n=4, d_pub=257, d_slots_out=512, stream=None)     # d_pub: any alignment
    args.update(kw)
    with pytest.raises(ValueError):
        _wrapper_only().dev_ed_keys_find(**args)


def test_dev_ed_keys_find_wrapper_empty_call_is_a_no_op():
    _wrapper_only().dev_ed_keys_find(0, 0, 0, 0)
    _wrapper_only().dev_ed_keys_find(0, 0, None, None, stream=None)
