"""The one-lane 9 x 29 field, group and scalar layers on the device
(gv_debug_lane_op: k_debug_lane in csrc/gv_kernels.hip with one mad chain per
column, k_debug_lane_lat in csrc/gv_lat.hip with two, k_debug_elane in
csrc/ed_verify.hip), one function per item and one item per lane, on the
operand sets of tests/lane_ops.py -- the sets tests/test_lane_host.py proves
sharp against single-fault mutants of the headers.

Every comparison is exact.  The device result must be the true one (Python
integers, the oracles' group laws) at the magnitude the function's comment
states, and every output word must equal the word the g++ host build of the
same configuration gives for the same item: the arithmetic is integer and
deterministic, so the host run, where every wrapping mad or limb add traps,
vouches for the code object that ships.  Without a host compiler these tests
fail.
"""
import numpy as np
import pytest

import gpuverify as gvm
import lane_ops as LO

pytestmark = pytest.mark.gpu
SECP_OPS = sorted((o for o, c in gvm.LNOP.items() if c < gvm.LNOP_SECP_END), key=gvm.LNOP.get)
ED_OPS = sorted((o for o, c in gvm.LNOP.items() if c >= 128), key=gvm.LNOP.get)
RUNS = [(op, ch) for op in SECP_OPS for ch in (1, 2)] + [(op, 1) for op in ED_OPS]
KNOWN = LO.ST + gvm.LNS_KNOWN


@pytest.fixture(scope="module")
def ver():
    v = gvm.Verifier([0])
    yield v
    v.close()


@pytest.fixture(scope="module")
def host():
    return {ch: LO.host_lib(ch) for ch in (1, 2)}


_DEV = {}


def dev_out(ver, op, chains):
    """the device result of the op's whole case, run once per unit"""
    if (op, chains) not in _DEV:
        out = ver.debug_lane_op(op, LO.cases()[op].inp, chains)
        out.setflags(write=False)
        _DEV[op, chains] = out
    return _DEV[op, chains]


def same_as_host(case, dev, hst):
    """every word of every item, but the coordinates of an infinite sum"""
    skip = case.undefined(hst)
    assert np.array_equal(skip, case.undefined(dev))
    assert np.array_equal(dev[:, LO.ST:], hst[:, LO.ST:])
    diff = np.nonzero((dev != hst).any(axis=1) & ~skip)[0]
    assert diff.size == 0, (case.op, "device and host limbs differ at items", diff[:8])


@pytest.mark.parametrize("op,chains", RUNS, ids=[f"{op}-{ch}ch" for op, ch in RUNS])
def test_device_op_is_true_and_equals_the_host_build(ver, host, op, chains):
    case = LO.cases()[op]
    dev = dev_out(ver, op, chains)
    case.check(dev)
    same_as_host(case, dev, LO.host_run(host[chains], op, case.inp))


@pytest.mark.parametrize("op", SECP_OPS)
def test_the_two_secp_units_agree(ver, op):
    case = LO.cases()[op]
    a, b = dev_out(ver, op, 1), dev_out(ver, op, 2)
    assert np.array_equal(a[:, LO.ST:], b[:, LO.ST:])
    skip = case.undefined(a)
    wordy = op == "to_words"
    for i in np.nonzero(~skip)[0]:
        for s in range(4):
            x, y = LO.slot(a, i, s), LO.slot(b, i, s)
            assert (x == y) if wordy else (LO.val(x) % LO.SECP.p == LO.val(y) % LO.SECP.p), (op, i, s)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_sizes_on_a_divergent_op(ver, host, n):
    """gej29x_add_scaled with general, doubling and infinity items in neighbouring
    lanes: the tail block's inactive lanes write nothing, the live ones everything"""
    case = LO.cases()["gejx_add_scaled"]
    inp = case.inp[:n]
    kinds = LO.host_run(host[1], "gejx_add_scaled", case.inp[:257])[:, LO.ST + gvm.LNS_INF]
    assert len(case.inp) >= 257 and kinds[:63].any() and not kinds[:63].all()
    for ch in (1, 2):
        dev = ver.debug_lane_op("gejx_add_scaled", inp, ch)
        assert dev.shape == (n, gvm.LN_OUT) and (dev[:, KNOWN] == 1).all()
        assert np.array_equal(dev, LO.host_run(host[ch], "gejx_add_scaled", inp)), (n, ch)
        assert np.array_equal(dev, dev_out(ver, "gejx_add_scaled", ch)[:n]), (n, ch)


def test_unknown_ops_and_mismatched_flags_are_refused(ver):
    one = LO.pack([([1] + [0] * 8,) * 2])
    for code in (-1, gvm.LNOP_SECP_END, 63, gvm.LNOP_LAT + gvm.LNOP_SECP_END, 127, gvm.LNOP_ED_END, 1 << 20):
        with pytest.raises(gvm.GpuVerifyError):
            ver.debug_lane_op(code, one)
    for op, ch in (("mul", 1), ("mul", 2), ("ed_mul", 1)):   # limb ops do not take words, word ops need the bit
        assert not ver.debug_lane_op(op, LO.pack([1], words=True), ch).any()
        out = ver.debug_lane_op(op, one, ch)
        assert out[0, KNOWN] == 1 and LO.slot(out, 0, 0) == [1] + [0] * 8
    for op, ch in (("from_words", 1), ("from_words", 2), ("ed_from_words", 1), ("ge_frombytes", 1), ("sc_reduce512", 1),
                   ("ed_comb8", 1)):
        assert not ver.debug_lane_op(op, one, ch).any()
    bad_entry = LO.pack([([1] + [0] * 8,) * 8], 9 << gvm.LNF_ENTRY_SHIFT)     # ge_add_tab has entries 0..8
    assert not ver.debug_lane_op("ge_add_tab", bad_entry).any()
