"""The options of the resident key arena's wide-window layouts
(include/gpuverify.h "keys_wide_qw", "keys_wide_mb" and the read-only keys
"kw_qw", "kwn_qw", "kw_arena_qw", "kw_arena_ng"): accepted and rejected
values, and gv_get_option reading back what gv_set_option wrote."""
import pytest

import gpuverify as gvm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    yield v
    v.close()


def test_build_widths(ver):
    assert ver.get_option("kw_qw") == 11
    assert ver.get_option("kwn_qw") == 9


def test_keys_wide_qw_values_round_trip(ver):
    assert ver.get_option("keys_wide_qw") == 0            # the default: every layout
    try:
        for v in (9, 11, 0):
            ver.set_option("keys_wide_qw", v)
            assert ver.get_option("keys_wide_qw") == v
        for bad in (7, 10, -1, 12, (1 << 32) + 9):
            with pytest.raises(gvm.GpuVerifyError):
                ver.set_option("keys_wide_qw", bad)
            assert ver.get_option("keys_wide_qw") == 0    # a rejected value changes nothing
    finally:
        ver.set_option("keys_wide_qw", 0)


def test_keys_wide_mb_round_trip(ver):
    assert ver.get_option("keys_wide_mb") == 0            # the default: no limit
    try:
        ver.set_option("keys_wide_mb", 1536)
        assert ver.get_option("keys_wide_mb") == 1536
        with pytest.raises(gvm.GpuVerifyError):
            ver.set_option("keys_wide_mb", -1)
        assert ver.get_option("keys_wide_mb") == 1536
    finally:
        ver.set_option("keys_wide_mb", 0)
    assert ver.get_option("keys_wide_mb") == 0


def test_arena_keys_are_read_only_and_zero_without_an_arena(ver):
    # no test of this module loads a key: the context has no wide arena
    assert ver.get_option("kw_arena_qw") == 0 and ver.get_option("kw_arena_ng") == 0
    for k in ("kw_arena_qw", "kw_arena_ng", "kw_qw", "kwn_qw"):
        with pytest.raises(gvm.GpuVerifyError):
            ver.set_option(k, 9)
