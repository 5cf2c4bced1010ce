"""Every host path of the Segmenter asks of its ops exactly what it asked before the per-batch step was folded into
``_step_features`` / ``_step_cluster``: the same calls in the same order, with the same scalars and tensors of the same dtype
and shape. Labels can survive a launch that a path gained, lost or reordered (a missing ``position_features`` with a zero
weight, a second smoothing of an all-equal image); the call log cannot.

The log of the code under test (tests/golden/make_host_call_traces.py, which also says what is logged) is compared with ``==``
against tests/golden/host_call_traces.json, recorded once by that script on the GPU at the commit before the change and never
regenerated from the code under test. No timing; nothing outside the repository is read."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_host_call_traces", os.path.join(GOLD, "make_host_call_traces.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    with open(os.path.join(GOLD, "host_call_traces.json")) as f:
        return json.load(f)


def test_the_fixture_holds_every_plan_and_path(golden):
    assert {plan: sorted(paths) for plan, paths in golden.items()} == {plan: sorted(rec.PATHS) for plan in rec.PLANS}
    for plan, paths in golden.items():
        for path in ("segment_device", "segment_batch_graph", "segment_batch_chunked", "segment_stream", "segment_images",
                     "features_device"):
            assert isinstance(paths[path], list) and paths[path], (plan, path)          # a recorded run, not a refusal


@pytest.mark.parametrize("path", list(rec.PATHS))
@pytest.mark.parametrize("plan", list(rec.PLANS))
def test_the_ops_calls_are_the_parents(golden, plan, path):
    got, want = json.loads(json.dumps(rec.record(plan, path))), golden[plan][path]
    if isinstance(want, list) and isinstance(got, list):
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, f"{plan} / {path}: call {i} of {len(got)} (fixture: {len(want)})"
    assert got == want
