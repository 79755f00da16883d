"""The launch program of the training step, pinned: one eager step's libkodhip calls, stream / event operations and aten
operations (tools/launch_trace.py) for every engine switch, freeze set, BatchNorm mode, collective mode and clipping mode,
against tests/golden/launch_trace.json (per configuration: number of lines, launches per entry point, SHA-256 of the text).

The eager sequence of stream operations is what a capture turns into graph nodes and edges: equal traces mean an equal
captured graph.  A refactor of engine/forward.py / engine/backward.py / the optimizer step must leave every hash where it
is.  A pull request that changes the program on purpose re-records the file on its own tree and shows the diff of the
traces (`--keep` writes them next to the JSON):

    python tools/launch_trace.py --record tests/golden/launch_trace.json [--keep DIR]

The eval_forward* rows pin one eval forward (two-pass and fused) the same way.  tests/golden/profile_families.json pins what
the launch text does not show: the (family, algorithmic bytes, name) sequence of eng.profile for one eager training step and
the two eval forwards - the byte formulas bench.py --full builds its roofline table from, and the one-stream schedule of a
profiled step.  The byte counts are integer arithmetic carried in floats: compared for equality.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("launch_trace", os.path.join(ROOT, "tools", "launch_trace.py"))
launch_trace = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(launch_trace)

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "launch_trace.json")))
PROFILES = json.load(open(os.path.join(ROOT, "tests", "golden", "profile_families.json")))
# a child that ended by a signal, an abort or its time limit: no further GPU child is started in this run
_stopped = []


def test_golden_covers_the_table():
    assert sorted(GOLDEN) == sorted(launch_trace.CONFIGS)


@pytest.mark.parametrize("config", list(launch_trace.CONFIGS))
def test_launch_trace_equals_golden(config, tmp_path):
    if _stopped:
        pytest.fail(f"not started: the trace child of {_stopped[0]} ended by a signal or its time limit")
    out = str(tmp_path / (config + ".trace"))
    rc, err = launch_trace.run_child(config, out)
    if rc is None or rc < 0 or rc in (124, 134, 137, 139):
        _stopped.append(config)
        pytest.fail(f"trace child of {config} ended by a signal or its time limit (rc {rc}):\n{err}")
    assert rc == 0, err
    got = launch_trace.summary(open(out).read())
    want = GOLDEN[config]
    hint = (f"full trace: {out}; the recorded tree's, for a diff: python tools/launch_trace.py {config} "
            "(on a checkout of the commit that recorded tests/golden/launch_trace.json)")
    assert got["lines"] == want["lines"], hint
    assert got["launches"] == want["launches"], hint
    assert got["sha256"] == want["sha256"], hint


def test_profile_golden_covers_the_cases():
    assert sorted(PROFILES) == sorted(launch_trace.PROFILE_CASES)


@pytest.mark.parametrize("case", list(launch_trace.PROFILE_CASES))
def test_profile_families_equal_golden(case, tmp_path):
    if _stopped:
        pytest.fail(f"not started: the trace child of {_stopped[0]} ended by a signal or its time limit")
    out = str(tmp_path / (case + ".json"))
    rc, err = launch_trace.run_child(case, out, profile=True)
    if rc is None or rc < 0 or rc in (124, 134, 137, 139):
        _stopped.append(case)
        pytest.fail(f"profile child of {case} ended by a signal or its time limit (rc {rc}):\n{err}")
    assert rc == 0, err
    got, want = json.load(open(out)), PROFILES[case]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"launch {i}: {g} != {w}"
