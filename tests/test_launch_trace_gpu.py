"""GPU suite: the launches of both engines' forward and backward walks, call by call, against the trace recorded before the
host-side MX-fp8 bookkeeping was restructured (tests/launch_trace.py; tests/golden/launch_trace.json).  The comparison is
exact: entry point, every scalar, and the wiring of every pointer."""
import json
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import launch_trace                                       # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "launch_trace.json")) as f:
        return json.load(f)


def test_golden_covers_the_scenarios(golden):
    assert sorted(golden) == sorted(launch_trace.SCENARIOS)
    assert all(len(v) > 0 for v in golden.values())


@pytest.mark.parametrize("name", sorted(launch_trace.SCENARIOS))
def test_launch_trace(name, golden):
    rec, _, _ = launch_trace.record(name)
    got, want = rec.lines(), golden[name]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: call %d differs: recorded %s, golden %s; its operands now: %s" % (
            name, k, g, w, json.dumps(rec.calls[k][1:], sort_keys=True))
    n = min(len(got), len(want))
    assert len(got) == len(want), "%s: %d launches, the golden has %d (the first %d agree); the next one: %s" % (
        name, len(got), len(want), n, (got if len(got) > n else want)[n])
