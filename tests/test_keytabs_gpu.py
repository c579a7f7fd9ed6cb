"""The runtime's key table sets (KeyTabs, csrc/gv_keytabs.h) against the
library of the commit before them: tools/record_keytabs.py's sequence of loads,
arena growths, keyed calls, grouped calls and a layout promotion is replayed
and every number it recorded there (tests/golden/keytabs_parent.json: the HBM
held by the optional tables, the route counters, the grouped layout and
arena, the wide arena's layout, after each step) must come out equal.  Every
verifying call's verdicts are checked against construction by the sequence
itself.

After each growth of the resident arena (4,096 -> 8,192 slots) the tables of
64 slots loaded before it -- the prefix the growth copied, the Z rows to a
new stride -- are read back with gv_keys_entry: entry 1 of every group of the
k4, the kn and the wide set must be the affine point 2^(QW w0(k)) Q of the
slot's key, computed by oracle/secp_ref.py.  Byte equality; no tolerance."""
import importlib.util
import json
import os

import numpy as np
import pytest

import gpuverify as gvm
from oracle import secp_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QWIN = {5: 26, 6: 22, 11: 12, 9: 15}                     # windows per 128-bit half
COPIED = np.r_[0:24, 130:150, 280:300].astype(np.uint32)  # 64 slots of the first load: both ends and the middle


def recorder():
    spec = importlib.util.spec_from_file_location("record_keytabs", os.path.join(REPO, "tools", "record_keytabs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def group_bits(qw, ng):
    """The bit each group's table starts at (csrc/gv_kernels.h: ceil(QWIN / NG) windows in the first groups)."""
    p = -(-QWIN[qw] // ng)
    r = QWIN[qw] - (p - 1) * ng
    return [qw * (k * p - max(0, k - r)) for k in range(ng)]


def doublings(pub, top):
    """[2^i Q for i = 0..top] as 64-byte affine x || y."""
    pt, out = R.parse_pubkey(bytes(pub)), []
    for _ in range(top + 1):
        out.append(pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big"))
        pt = R.point_add(pt, pt)
    return out


def test_sequence_reproduces_the_parent_and_copied_prefix_holds_its_points():
    rec = recorder()
    assert len(COPIED) == 64 and COPIED.max() < rec.FIRST
    with open(os.path.join(REPO, "tests", "golden", "keytabs_parent.json")) as f:
        want = json.load(f)["steps"]
    w = rec.Workload()
    dbl = [doublings(w.pub[s], 121) for s in COPIED]     # the highest group start: 11 x 11 bits
    checked = []

    def copied_prefix(v, step):
        wide = (v.get_option("kw_arena_qw"), v.get_option("kw_arena_ng"))
        assert wide == ((11, 12) if step.startswith("A") else (11, 6)), step
        for tabs, (qw, ng) in enumerate(((5, 4), (6, 11), wide)):
            bits = group_bits(qw, ng)
            slots, groups = np.repeat(COPIED, ng), np.tile(np.arange(ng, dtype=np.uint32), len(COPIED))
            xy, ok = v.keys_entry(tabs, slots, groups, np.ones(len(slots), np.uint32))
            assert ok.all(), f"{step}: verdicts of table set {tabs}"
            exp = np.frombuffer(b"".join(d[b] for d in dbl for b in bits), np.uint8).reshape(-1, 64)
            bad = np.nonzero((xy != exp).any(axis=1))[0]
            assert not len(bad), f"{step}: table set {tabs} ({qw} x {ng}), first wrong (slot, group): " \
                                 f"{[(int(slots[i]), int(groups[i])) for i in bad[:6]]}"
            checked.append((step, tabs))

    got = rec.run(lambda: gvm.Verifier([0]), w, hook=copied_prefix)
    assert [s for s, _ in checked] == ["A grown"] * 3 + ["B grown"] * 3
    assert [name for name, _ in got] == [name for name, _ in want]
    for (name, g), (_, e) in zip(got, want):
        assert g == e, f"step {name!r}: " + ", ".join(f"{k}: {g[k]} != {e[k]}" for k in e if g.get(k) != e[k])
    # the sequence took the paths it is there for
    by = dict(got)
    assert by["A grown"]["routes"] == by["A open"]["routes"] and by["A keyed 16384"]["routes"]["kw"] == 1
    assert by["B keyed 16384"]["routes"]["kw2"] == 1 and by["B keyed 1024"]["routes"]["lat_keyed"] == 1
    assert by["B grouped 9"]["group_promoted"] == 2 and by["B grouped 9"]["group_layout"] == 9
    assert by["B grouped 9"]["hbm_optional_bytes"] > by["B grouped 7"]["hbm_optional_bytes"]
