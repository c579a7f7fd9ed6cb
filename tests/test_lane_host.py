"""The one-lane 9 x 29 field, group and scalar layers (csrc/secp_fe29.cuh,
secp_fe29x.cuh, secp_group29.cuh, secp_group29x.cuh, ed_fe29.cuh,
ed_group.cuh, ed_scalar.cuh) in a g++ host build with the GV_F29_CHECK
overflow traps (tools/fe29/lane_host.cpp: the op bodies of gv_debug_lane_op),
in both chain configurations, on the operand sets of tests/lane_ops.py: every
value against Python integers and the oracles' group laws, every output
magnitude as the function's comment states it, no trap (a trap aborts).

The sharpness test shows that the shared operand set tells each single-fault
mutant of the headers from the true arithmetic: the device tests
(tests/test_lane_gpu.py) run the same set, so the same fault in the shipped
kernels would fail there.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

import lane_ops as LO


@pytest.fixture(scope="module", params=[1, 2], ids=["one-chain", "two-chain"])
def lib(request):
    return LO.host_lib(request.param)


@pytest.mark.parametrize("op", sorted(LO.gvm.LNOP, key=LO.gvm.LNOP.get))
def test_op_matches_python_integers(lib, op):
    case = LO.cases()[op]
    case.check(LO.host_run(lib, op, case.inp))


def test_unknown_ops_and_mismatched_flags_are_refused(lib):
    one = LO.pack([([1] + [0] * 8,) * 2])
    for code in (-1, LO.gvm.LNOP_SECP_END, 127, LO.gvm.LNOP_ED_END):
        assert lib.lane_host_ops(code, 1, one.ctypes.data, one.copy().ctypes.data) == -1
    for op in ("mul", "ed_mul"):                             # limb ops do not take words, word ops need the bit
        assert LO.host_run(lib, op, LO.pack([1], words=True))[0, LO.ST + LO.gvm.LNS_KNOWN] == 0
        assert LO.slot(LO.host_run(lib, op, one), 0, 0) == [1] + [0] * 8
    for op in ("from_words", "ed_from_words", "ge_frombytes", "sc_reduce512", "ed_comb8"):
        assert not LO.host_run(lib, op, one).any()
    bad_entry = LO.pack([([1] + [0] * 8,) * 8], 9 << LO.gvm.LNF_ENTRY_SHIFT)
    assert not LO.host_run(lib, "ge_add_tab", bad_entry).any()


def test_the_set_reaches_the_last_carry_of_a_reduction():
    """chi, the part above 2^32 of the carry out of column 8, is non-zero once
    column 8 alone reaches 2^61: the F29_RH1 / F29_RH2 / E29_RH terms act"""
    for k, op in ((LO.SECP, "mul"), (LO.SECP, "x_mul"), (LO.ED, "ed_mul")):
        inp = LO.cases()[op].inp
        n = sum(LO.col8([int(x) for x in r[:9]], [int(x) for x in r[9:18]]) >= 1 << 61 for r in inp)
        assert n >= 200, (op, n)


# ---------------------------------------------------------------- sharpness
FE, FX, G29, EFE, EG = "secp_fe29.cuh", "secp_fe29x.cuh", "secp_group29.cuh", "ed_fe29.cuh", "ed_group.cuh"
MUTANTS = {
    # name: (header, text, replacement, ops whose cases must tell it apart)
    "F29_R0+1": (FE, "#define F29_R0 31264u", "#define F29_R0 31265u", ["mul", "x_mul", "norm"]),
    "F29_R1+1": (FE, "#define F29_R1 256u", "#define F29_R1 257u", ["mul", "x_mul", "norm"]),
    "F29_RH1+1": (FE, "#define F29_RH1 250112u", "#define F29_RH1 250113u", ["mul", "multi_mm", "x_mul"]),
    "F29_RH2+1": (FE, "#define F29_RH2 2048u", "#define F29_RH2 2049u", ["mul", "multi_mm", "x_mul"]),
    "E29_R+1": (EFE, "#define E29_R 1216u", "#define E29_R 1217u", ["ed_mul", "ed_norm"]),
    "E29_RH+1": (EFE, "#define E29_RH 9728u", "#define E29_RH 9729u", ["ed_mul", "ed_sqr"]),
    "no chi*RH2 (f29_mulsqr)": (FE, "f29_add32((u32)(x >> 29), chi * F29_RH2)", "(u32)(x >> 29)", ["mul", "sqr"]),
    "no chi*RH2 (f29_multi)": (FE, "f29_add32((u32)(x[s] >> 29), chi[s] * F29_RH2)", "(u32)(x[s] >> 29)",
                               ["multi_ss", "multi_mmm", "multi_mm", "multi_ssm"]),
    "no chi*RH2 (f29x_reduce)": (FX, "f29_add32((u32)(x >> 29), chi * F29_RH2)", "(u32)(x >> 29)", ["x_mul", "x_sqr"]),
    "hi<<2 (f29x_high)": (FX, "t[8] = hi << 3;", "t[8] = hi << 2;", ["x_mul", "x_sqr"]),
    "hi<<2 (e29_mulsqr)": (EFE, "t[8] = hi << 3;", "t[8] = hi << 2;", ["ed_mul", "ed_sqr"]),
    "kk.eight->kk.one": (FX, "A.mad(hi, kk.eight)", "A.mad(hi, kk.one)", ["x_mul", "x_sqr"]),
    # The window is reached only by multiples k p with k >= 128 (magnitude 5 and above).  The addition laws
    # test an H of magnitude 1 (k <= 32), where both windows answer alike, so their cases cannot see this
    # fault: it shows in f29_is_zero_fast itself, on the magnitude-7 multiples.
    "977*128": (G29, "977u * 256u", "977u * 128u", ["gej_add_ge", "gejx_add_scaled", "is_zero_fast"]),
    "h*978 (f29_to_words)": (FE, "h * 977u", "h * 978u", ["to_words", "is_zero"]),
    "h*20 (e29_to_words)": (EFE, "h * 19u", "h * 20u", ["ed_to_words", "ed_is_zero"]),
    "28-S (f29_shl_norm)": (FE, "a.n[i] >> (29 - S)", "a.n[i] >> (28 - S)", ["shl_norm1", "shl_norm2", "shl_norm3"]),
    "ge_add_cached qa": (EG, "// mag 3\n  fe_select(qa, neg, q.ymx, q.ypx);", "// mag 3\n  fe_select(qa, neg, q.ypx, q.ymx);",
                         ["ge_add_cached"]),
    "ge_add_cached z1": (EG, "fe_select(z1, neg, dmc, dpc);       // Z'", "fe_select(z1, neg, dpc, dmc);       // Z'",
                         ["ge_add_cached"]),
}


@pytest.fixture(scope="module")
def true_lib_without_traps():
    return LO.host_lib(1, traps=False)


def test_the_mutant_build_without_faults_passes(true_lib_without_traps):
    """the build the mutants use (no traps, so none of them can abort) is otherwise the checked one"""
    for op in sorted({o for m in MUTANTS.values() for o in m[3]}):
        case = LO.cases()[op]
        case.check(LO.host_run(true_lib_without_traps, op, case.inp))


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_operand_set_tells_each_mutant_from_the_true_arithmetic(name):
    header, old, new, ops = MUTANTS[name]
    d = tempfile.mkdtemp()
    try:
        csrc = os.path.join(d, "csrc")
        shutil.copytree(LO.CSRC, csrc, ignore=lambda _, names: [n for n in names if not n.endswith((".cuh", ".inc", ".h"))])
        path = os.path.join(csrc, header)
        txt = open(path).read()
        assert txt.count(old) == 1, (name, txt.count(old))
        open(path, "w").write(txt.replace(old, new))
        L = LO.host_lib(1, csrc=csrc, traps=False, out_dir=d)
        told = []
        for op in ops:
            case = LO.cases()[op]
            try:
                case.check(LO.host_run(L, op, case.inp))
            except AssertionError:
                told.append(op)
        assert told, (name, "no item of", ops, "is wrong under this fault: a gap in the operand set")
    finally:
        shutil.rmtree(d, ignore_errors=True)
