"""The Python model layer against tests/golden/model_config.json (recorded by tests/golden/make_model_config_golden.py, on the CPU): what a
params dict becomes - every field of the engine configuration, the defaults check_params inserts - for the reference's 81 single-task
configs and for the options they do not reach, every refusal with its exception class and its exact text, the initial value of every
variable (the engine's tables and the three module-level stores), and the endpoint order.  No GPU."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_script():
    spec = importlib.util.spec_from_file_location("make_model_config_golden", os.path.join(GOLDEN, "make_model_config_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def script():
    return _load_script()


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "model_config.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded(script):
    return json.loads(json.dumps(script.record()))      # through JSON: tuples become lists, as in the file


def test_the_file_holds_every_case_the_script_lists(script, golden):
    held = ["configs/" + n for n in golden["configs"]] + ["refusals/" + n for n in golden["refusals"] if not n.startswith("store/")]
    assert sorted(held) == script.case_names()
    assert sum(1 for n in golden["configs"] if not n.startswith("extra/")) == 81
    assert all(v is not None for v in golden["refusals"].values()), "every listed refusal case raises"
    assert os.path.getsize(os.path.join(GOLDEN, "model_config.json")) < os.path.getsize(os.path.join(GOLDEN, "engine_layout.json"))


def test_engine_configs(golden, recorded):
    assert recorded["base"] == golden["base"]
    for name, (train, predict, added, sha) in golden["configs"].items():
        got = recorded["configs"][name]
        assert recorded["dumps"][got[0]] == golden["dumps"][train], name
        assert recorded["dumps"][got[1]] == golden["dumps"][predict], name + " (predict form)"
        assert got[2:] == [added, sha], name + " (params.dict as the call left it)"
    assert recorded["configs"].keys() == golden["configs"].keys()


def test_refusals(golden, recorded):
    for name, want in golden["refusals"].items():
        assert recorded["refusals"][name] == want, name
    assert recorded["refusals"].keys() == golden["refusals"].keys()


def test_initial_values(golden, recorded):
    assert len(golden["init"]) == 22
    for name, want in golden["init"].items():
        assert [recorded["init_hashes"][i] for i in recorded["init"][name]] == [golden["init_hashes"][i] for i in want], name
    assert recorded["stores"] == golden["stores"]


def test_endpoint_order(golden, recorded):
    assert recorded["endpoint_order"] == golden["endpoint_order"]
