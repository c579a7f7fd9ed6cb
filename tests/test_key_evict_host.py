"""The host mirror's clock eviction (gvh_set_key_resident) on the CPU:
tests/evict/evict_harness.cpp -- host/gvhost.cpp over a CPU fake that also
defines gv_keys_replace -- built with ASan + UBSan and with TSan and run as a
program.  It replays the churn workload (tests/evict_workload.py) through
gvh_deliver_blocks with the DeliverTx pool under 8 concurrent gvh_checktx
threads, checks the key-slot bookkeeping after every block, and compares the
codes with a run without eviction; here they are also compared with
tests/ante_ref.py."""
import json
import os
import subprocess

import pytest

import evict_workload as W

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(REPO, "tests", "evict")


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    r = subprocess.run(["make", "-s", "-j2", "-C", DIR], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    accts, blocks, parts, check = W.workload(check_threads=8)
    path = str(tmp_path_factory.mktemp("evict") / "fixture.bin")
    W.write_fixture(path, accts, blocks, check)
    return path, accts, blocks, parts


def _run(binary, path, env_extra):
    r = subprocess.run([os.path.join(DIR, "build", binary), path, str(W.RESIDENT)], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **env_extra))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-6000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    return json.loads(r.stdout)


def _common(got, blocks):
    assert len(got["blocks"]) == sum(len(b) for b in blocks)
    assert got["replaced"] > 0 and got["resets"] == 0 and got["count"] <= W.RESIDENT
    assert 4 in got["check"] and 0 in got["check"]


def test_asan_ubsan_eviction(fixture):
    path, accts, blocks, parts = fixture
    got = _run("evict_asan", path, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:halt_on_error=1"})
    _common(got, blocks)
    assert 0 < got["blocks"].count(0) < len(got["blocks"])
    assert got["blocks"] == W.reference_codes(accts, blocks, parts)[0]


def test_tsan_eviction(fixture):
    path, _, blocks, _ = fixture
    got = _run("evict_tsan", path, {"TSAN_OPTIONS": "halt_on_error=1:detect_deadlocks=0"})
    _common(got, blocks)
