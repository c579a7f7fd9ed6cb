"""CPU tests of the gv_ed_keys_replace / gv_ed_keys_point boundary: the symbols
answer without a GPU, the Python wrapper checks shapes before it calls, and
the host mirror exposes the ed25519 resident-size setting."""
import ctypes

import numpy as np
import pytest

import gpuverify as gvm


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_null_context_is_einval_without_gpu():
    L = gvm.load()
    slots = np.array([0, 1], np.uint32)
    pub = np.zeros((2, 32), np.uint8)
    enc, ok = np.zeros((2, 32), np.uint8), np.zeros(2, np.uint8)
    assert L.gv_ed_keys_replace(None, 2, _p(slots), _p(pub)) == gvm.GV_EINVAL
    assert L.gv_ed_keys_replace(None, 0, None, None) == gvm.GV_EINVAL
    assert L.gv_ed_keys_point(None, 2, _p(slots), 0, 1, _p(enc), _p(pub), _p(ok)) == gvm.GV_EINVAL
    assert L.gv_ed_keys_point(None, 0, None, 0, 1, None, None, None) == gvm.GV_EINVAL
    assert "gv_ed_keys_replace" in gvm.EXPORTED_SYMBOLS and "gv_ed_keys_point" in gvm.EXPORTED_SYMBOLS


class _NoCall:
    """Stands in for the loaded library: any call is a test failure."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} called before the argument checks")


def _wrapper_only():
    v = gvm.Verifier.__new__(gvm.Verifier)             # no gv_open: only the wrapper's own checks run
    v._L, v._ctx, v._inflight = _NoCall(), None, {}
    return v


@pytest.mark.parametrize("slots, pub", [
    (np.arange(3, dtype=np.uint32), np.zeros((2, 32), np.uint8)),          # lengths differ
    (np.arange(2, dtype=np.uint32), np.zeros((2, 33), np.uint8)),          # not 32-byte keys
    (np.arange(2, dtype=np.uint32), np.zeros(64, np.uint8)),               # not (n, 32)
    (np.arange(2, dtype=np.uint32), np.zeros((2, 32), np.uint16)),         # not bytes
    (np.zeros((2, 1), np.uint32), np.zeros((2, 32), np.uint8)),            # slots not 1-d
    (np.array([0.0, 1.0]), np.zeros((2, 32), np.uint8)),                   # slots not integers
    (np.array([0, -1]), np.zeros((2, 32), np.uint8)),                      # not a u32
    (np.array([0, 1 << 32]), np.zeros((2, 32), np.uint8)),
])
def test_wrapper_checks_shapes_before_any_call(slots, pub):
    with pytest.raises(ValueError):
        _wrapper_only().ed_keys_replace(slots, pub)


def test_wrapper_empty_call_is_a_no_op():
    _wrapper_only().ed_keys_replace(np.zeros(0, np.uint32), np.zeros((0, 32), np.uint8))


def test_gvhost_exposes_the_ed_resident_setting():
    import gvhost
    L = gvhost.lib()
    assert hasattr(L, "gvh_set_ed_key_resident") and hasattr(L, "gvh_get_ed_key_stats")
    assert callable(gvhost.HostApp.set_ed_key_resident) and callable(gvhost.HostApp.ed_key_stats)


def test_ed_resident_setting_without_a_verifier():
    """The setting is stored, clamped to GV_ED_KEY_CAP, and off by default."""
    import gvhost
    app = gvhost.HostApp(None)
    assert app.ed_key_stats() == (0, 0, 0)
    app.set_ed_key_resident(128)
    assert app.ed_key_stats() == (128, 0, 0)
    app.set_ed_key_resident((1 << 16) + 5)
    assert app.ed_key_stats() == (1 << 16, 0, 0)
    app.set_ed_key_resident(0)
    assert app.ed_key_stats() == (0, 0, 0)
    app.close()
