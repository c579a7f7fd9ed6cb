"""gv_set_option, gv_get_option and the GV_* option variables of the built
library against tests/golden/options_parent.json, the record of the library
before the options moved into csrc/gv_options.h (tools/record_options.py, run
once on that commit's library): every return code, every value read back and
every default, entry for entry, and the readable options of three fresh
processes that open a context with every option variable at "0", at "1" and
at an out-of-range or garbage value (one process at a time)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("record_options", os.path.join(REPO, "tools", "record_options.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def parent(golden_dir):
    with open(os.path.join(golden_dir, "options_parent.json")) as f:
        return json.load(f)


def test_setter_and_getter_reproduce_the_parent(parent, monkeypatch):
    tool = _tool()
    assert parent["probes"] == tool.PROBES and sorted(parent["keys"]) == sorted(tool.KEYS)
    monkeypatch.setenv("GV_EAGER_TABLES", "0")
    for v in tool.ENV_VARS:
        monkeypatch.delenv(v, raising=False)
    c = tool.Ctx()
    try:
        got = tool.probe_keys(c)
    finally:
        c.close()
    for key in tool.KEYS:
        want = parent["keys"][key]
        assert got[key]["default"] == want["default"], key
        assert got[key]["coupled"] == want["coupled"], key
        for val, g, w in zip(tool.PROBES, got[key]["set"], want["set"]):
            assert g == w, (key, val)


@pytest.mark.parametrize("child", ["zero", "one", "garbage"])
def test_option_variables_reproduce_the_parent(parent, child):
    tool = _tool()
    assert tool.env_child(None, tool.ENV_CHILDREN[child]) == parent["env"][child]
