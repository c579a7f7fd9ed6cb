"""CPU tests of the gv_keys_entry / gv_group_entry boundary (key-table entry
readback, include/gpuverify.h): the symbols are exported and declared and
answer without a GPU, and the Python wrappers check the triples' shapes before
they call."""
import ctypes
import os
import re

import numpy as np
import pytest

import gpuverify as gvm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gv_keys_entry", "gv_group_entry")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_are_exported_and_declared():
    L = gvm.load()
    hdr = open(os.path.join(REPO, "include", "gpuverify.h")).read()
    for name in NEW:
        assert name in gvm.EXPORTED_SYMBOLS
        assert hasattr(L, name)
        assert len(re.findall(r"^int %s\(gv_ctx\* ctx, int dev_slot, int \w+, size_t n," % name, hdr, re.M)) == 1


def test_null_context_is_einval_without_gpu():
    L = gvm.load()
    a = np.array([0, 1], np.uint32)
    g = np.zeros(2, np.uint32)
    j = np.ones(2, np.uint32)
    key, xy, ok = np.full((2, 33), 7, np.uint8), np.full((2, 64), 7, np.uint8), np.full(2, 7, np.uint8)
    for tabs in (0, 1, 2):
        assert L.gv_keys_entry(None, 0, tabs, 2, _p(a), _p(g), _p(j), _p(xy), _p(ok)) == gvm.GV_EINVAL
    assert L.gv_keys_entry(None, 0, 0, 0, None, None, None, None, None) == gvm.GV_EINVAL
    for s in (0, 1, 2, 3):
        assert L.gv_group_entry(None, 0, s, 2, _p(a), _p(g), _p(j), _p(key), _p(xy), _p(ok)) == gvm.GV_EINVAL
    assert L.gv_group_entry(None, 0, 0, 0, None, None, None, None, None, None) == gvm.GV_EINVAL
    assert (key == 7).all() and (xy == 7).all() and (ok == 7).all()      # nothing was written


class _NoCall:
    """Stands in for the loaded library: any call is a test failure."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} called before the argument checks")


def _wrapper_only():
    v = gvm.Verifier.__new__(gvm.Verifier)             # no gv_open: only the wrapper's own checks run
    v._L, v._ctx, v._inflight = _NoCall(), None, {}
    return v


U = np.uint32
BAD_TRIPLES = [
    (np.zeros((2, 1), U), np.zeros(2, U), np.ones(2, U)),            # slots not 1-d
    (np.zeros(2, U), np.zeros((1, 2), U), np.ones(2, U)),            # groups not 1-d
    (np.zeros(2, U), np.zeros(2, U), np.ones((2, 1), U)),            # js not 1-d
    (np.zeros(2, U), np.zeros(2, U), U(1)),                          # js a scalar
    (np.zeros(3, U), np.zeros(2, U), np.ones(2, U)),                 # unequal lengths, each position
    (np.zeros(2, U), np.zeros(3, U), np.ones(2, U)),
    (np.zeros(2, U), np.zeros(2, U), np.ones(1, U)),
    (np.zeros(0, U), np.zeros(0, U), np.ones(1, U)),
    (np.array([0.0, 1.0]), np.zeros(2, U), np.ones(2, U)),           # not integers
    (np.array([0, -1]), np.zeros(2, U), np.ones(2, U)),              # not a u32
    (np.zeros(2, U), np.array([0, 1 << 32]), np.ones(2, U)),
]


@pytest.mark.parametrize("slots, groups, js", BAD_TRIPLES)
def test_wrappers_check_the_triples_before_any_call(slots, groups, js):
    with pytest.raises(ValueError):
        _wrapper_only().keys_entry(0, slots, groups, js)
    with pytest.raises(ValueError):
        _wrapper_only().group_entry(0, slots, groups, js)


@pytest.mark.parametrize("which", [0.5, "0", True, None])
def test_wrappers_check_the_selectors_before_any_call(which):
    t = (np.zeros(2, U), np.zeros(2, U), np.ones(2, U))
    with pytest.raises(ValueError):
        _wrapper_only().keys_entry(which, *t)
    with pytest.raises(ValueError):
        _wrapper_only().keys_entry(0, *t, dev_slot=which)
    with pytest.raises(ValueError):
        _wrapper_only().group_entry(which, *t)
    with pytest.raises(ValueError):
        _wrapper_only().group_entry(0, *t, dev_slot=which)


def test_empty_calls_are_no_ops():
    e = np.zeros(0, U)
    xy, ok = _wrapper_only().keys_entry(2, e, e, e, dev_slot=1)
    assert xy.shape == (0, 64) and ok.shape == (0,) and xy.dtype == ok.dtype == np.uint8
    key, xy, ok = _wrapper_only().group_entry(3, e, e, e)
    assert key.shape == (0, 33) and xy.shape == (0, 64) and ok.shape == (0,)
