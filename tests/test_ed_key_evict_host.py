"""The host mirror's clock eviction over the ed25519 key arena
(gvh_set_ed_key_resident) on the CPU: tests/evict/evict_ed_harness.cpp --
host/gvhost.cpp over a CPU fake that also defines gv_ed_keys_replace -- built
with ASan + UBSan and with TSan and run as a program.  Four threads drive
gvh_verify_commits (keys_trusted) over 12 validator sets of 40 keys with a
resident size of 128; the harness checks the key-slot bookkeeping after every
call and compares every result with a run without eviction."""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(REPO, "tests", "evict")
RESIDENT = 128


@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-s", "-j2", "-C", DIR], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def _run(binary, env_extra):
    r = subprocess.run([os.path.join(DIR, "build", binary), str(RESIDENT)], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, **env_extra))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-6000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    return json.loads(r.stdout)


def _common(got):
    assert got["replaced"] > 0 and got["resets"] == 0 and got["count"] <= RESIDENT
    # 4 threads x (12 calls of one commit + 6 of two); commits with a flipped bit answer "wrong signature" (3)
    assert len(got["codes"]) == 4 * 24
    assert set(got["codes"]) == {0, 3} and 0 < got["codes"].count(3) < len(got["codes"]) // 2


def test_asan_ubsan_ed_eviction(built):
    _common(_run("evict_ed_asan", {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:halt_on_error=1"}))


def test_tsan_ed_eviction(built):
    _common(_run("evict_ed_tsan", {"TSAN_OPTIONS": "halt_on_error=1:detect_deadlocks=0"}))
