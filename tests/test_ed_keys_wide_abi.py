"""CPU tests of the gv_dev_verify_ed25519_msgs_keyed / gv_ed_keys_wide_point
boundary: the symbols answer without a GPU, and the Python wrappers check
shapes, w and j before they call."""
import ctypes

import numpy as np
import pytest

import gpuverify as gvm


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_null_context_is_einval_without_gpu():
    L = gvm.load()
    slots = np.array([0, 1], np.uint32)
    enc, ok = np.zeros((2, 32), np.uint8), np.zeros(2, np.uint8)
    assert L.gv_ed_keys_wide_point(None, 2, _p(slots), 0, 1, _p(enc), _p(ok)) == gvm.GV_EINVAL
    assert L.gv_ed_keys_wide_point(None, 0, None, 0, 1, None, None) == gvm.GV_EINVAL
    vp = ctypes.c_void_p
    assert L.gv_dev_verify_ed25519_msgs_keyed(None, 0, 2, vp(256), vp(512), vp(1024), vp(2048), vp(4096), vp(8192),
                                              None) == gvm.GV_EINVAL
    assert L.gv_dev_verify_ed25519_msgs_keyed(None, 0, 0, None, None, None, None, None, None, None) == gvm.GV_EINVAL
    assert "gv_dev_verify_ed25519_msgs_keyed" in gvm.EXPORTED_SYMBOLS
    assert "gv_ed_keys_wide_point" in gvm.EXPORTED_SYMBOLS
    # the new options are refused like every other one without a context
    assert L.gv_set_option(None, b"ed_keys_wide", 8) == gvm.GV_EINVAL
    v = ctypes.c_longlong(7)
    assert L.gv_get_option(None, b"ed_kw_rb", ctypes.byref(v)) == gvm.GV_EINVAL and v.value == 7


class _NoCall:
    """Stands in for the loaded library: any call is a test failure."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} called before the argument checks")


def _wrapper_only():
    v = gvm.Verifier.__new__(gvm.Verifier)             # no gv_open: only the wrapper's own checks run
    v._L, v._ctx, v._inflight = _NoCall(), None, {}
    return v


@pytest.mark.parametrize("slots, w, j", [
    (np.zeros((2, 1), np.uint32), 0, 1),               # slots not 1-d
    (np.array([0.0, 1.0]), 0, 1),                      # slots not integers
    (np.array([0, -1]), 0, 1),                         # not a u32
    (np.array([0, 1 << 32]), 0, 1),
    (np.arange(2, dtype=np.uint32), -1, 1),            # w below every radix's windows
    (np.arange(2, dtype=np.uint32), 43, 1),            # w past the radix-64 comb's 43 windows
    (np.arange(2, dtype=np.uint32), 0, 0),             # entries are j = 1..NE
    (np.arange(2, dtype=np.uint32), 0, 129),           # j past the radix-256 comb's 128 entries
    (np.arange(2, dtype=np.uint32), 0.5, 1),
    (np.arange(2, dtype=np.uint32), 0, "1"),
    (np.arange(2, dtype=np.uint32), True, 1),
])
def test_wide_point_wrapper_checks_before_any_call(slots, w, j):
    with pytest.raises(ValueError):
        _wrapper_only().ed_keys_wide_point(slots, w, j)


def test_wide_point_wrapper_empty_call_is_a_no_op():
    enc, ok = _wrapper_only().ed_keys_wide_point(np.zeros(0, np.uint32), 3, 2)
    assert enc.shape == (0, 32) and ok.shape == (0,)


@pytest.mark.parametrize("kw", [
    dict(n=-1), dict(n=2.0), dict(n=True), dict(slot="0"), dict(d_slots=1.5), dict(d_sig=-16), dict(d_off="x"),
    dict(d_len=[1]), dict(d_bits=2.0), dict(d_blob=b"ab"), dict(stream=-1),
])
def test_dev_wrapper_checks_before_any_call(kw):
    args = dict(slot=0, n=4, d_slots=256, d_sig=512, d_blob=1024, d_off=2048, d_len=4096, d_bits=8192, stream=None)
    args.update(kw)
    with pytest.raises(ValueError):
        _wrapper_only().dev_verify_ed25519_keyed(**args)


def test_dev_wrapper_empty_call_is_a_no_op():
    _wrapper_only().dev_verify_ed25519_keyed(0, 0, 0, 0, 0, 0, 0, 0)
    _wrapper_only().dev_verify_ed25519_keyed(0, 0, None, None, None, None, None, None, stream=None)
