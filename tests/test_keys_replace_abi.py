"""CPU tests of the gv_keys_replace boundary: the symbol answers without a
GPU, the Python wrapper checks shapes before it calls, and the host mirror
exposes the resident-size setting."""
import ctypes

import numpy as np
import pytest

import gpuverify as gvm


def test_null_context_is_einval_without_gpu():
    L = gvm.load()
    slots = np.array([0, 1], np.uint32)
    pub = np.zeros((2, 33), np.uint8)
    assert L.gv_keys_replace(None, 2, slots.ctypes.data_as(ctypes.c_void_p),
                             pub.ctypes.data_as(ctypes.c_void_p)) == gvm.GV_EINVAL
    assert L.gv_keys_replace(None, 0, None, None) == gvm.GV_EINVAL
    assert "gv_keys_replace" in gvm.EXPORTED_SYMBOLS


class _NoCall:
    """Stands in for the loaded library: any call is a test failure."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} called before the argument checks")


def _wrapper_only():
    v = gvm.Verifier.__new__(gvm.Verifier)             # no gv_open: only the wrapper's own checks run
    v._L, v._ctx, v._inflight = _NoCall(), None, {}
    return v


@pytest.mark.parametrize("slots, pub", [
    (np.arange(3, dtype=np.uint32), np.zeros((2, 33), np.uint8)),          # lengths differ
    (np.arange(2, dtype=np.uint32), np.zeros((2, 32), np.uint8)),          # not 33-byte keys
    (np.arange(2, dtype=np.uint32), np.zeros(66, np.uint8)),               # not (n, 33)
    (np.arange(2, dtype=np.uint32), np.zeros((2, 33), np.uint16)),         # not bytes
    (np.zeros((2, 1), np.uint32), np.zeros((2, 33), np.uint8)),            # slots not 1-d
    (np.array([0.0, 1.0]), np.zeros((2, 33), np.uint8)),                   # slots not integers
    (np.array([0, -1]), np.zeros((2, 33), np.uint8)),                      # not a u32
    (np.array([0, 1 << 32]), np.zeros((2, 33), np.uint8)),
])
def test_wrapper_checks_shapes_before_any_call(slots, pub):
    with pytest.raises(ValueError):
        _wrapper_only().keys_replace(slots, pub)


def test_wrapper_empty_call_is_a_no_op():
    _wrapper_only().keys_replace(np.zeros(0, np.uint32), np.zeros((0, 33), np.uint8))


def test_gvhost_exposes_the_resident_setting():
    import gvhost
    L = gvhost.lib()
    assert hasattr(L, "gvh_set_key_resident") and hasattr(L, "gvh_get_key_stats")
    assert callable(gvhost.HostApp.set_key_resident) and callable(gvhost.HostApp.key_stats)
