"""The engine's layout, per pooling kind and loss-head kind, against tests/golden/engine_layout.json (recorded by
tests/golden/make_engine_layout_golden.py before pooling and loss head moved behind one interface each): variable names, shapes, trainable
flags and offsets, the three counts, the stage gradient ranges, the arena size and the byte offset of every endpoint the configuration
serves.  Equality, not closeness: a checkpoint, a gradient exchange and every arena pointer depend on these numbers."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_engine_layout_golden as M  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(M.PATH) as f:
        return json.load(f)


def test_the_golden_file_holds_every_configuration(golden):
    assert sorted(golden) == sorted(M.CONFIGS)


@pytest.mark.parametrize("name", sorted(M.CONFIGS))
def test_layout_equals_the_recorded_one(golden, name):
    got = json.loads(json.dumps(M.record(name)))      # (tuples -> lists, as the file has them)
    want = golden[name]
    assert got["counts"] == want["counts"]
    assert got["stages"] == want["stages"]
    assert got["variables"] == want["variables"]
    assert got["arena_bytes"] == want["arena_bytes"]
    assert got["endpoints"] == want["endpoints"]
    assert sorted(got) == sorted(want)
