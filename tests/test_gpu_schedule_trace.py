"""The inference schedule (image-prior encoder on a side stream joined level by level, CVEncoder's deferred last level, the
decoder's early first column and forked nodes) pinned as a launch trace: tests/schedule_trace.py says what a trace holds.
The fixture tests/golden/decoder_schedule_trace.json.gz was recorded by scripts/record_decoder_schedule_trace.py from the
commit BEFORE the schedule's code was folded and is never regenerated: a change that cannot pass it has changed the schedule."""
import pytest
import torch

import schedule_trace as st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def traced():
    return st.run_cases()


def test_inference_schedule_trace_matches_the_golden(traced):
    traces, golden = traced[0], st.load_golden()
    assert sorted(traces) == sorted(golden) == sorted(st.CASES)
    for case in st.CASES:
        got, want = traces[case], golden[case]
        first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
        assert got == want, (case, first, got[first:first + 3], want[first:first + 3])


def test_schedules_compute_the_same_outputs(traced):
    """Side stream on / off / without level events, and forked / partly forked / unforked decoder nodes: the same launches on
    the same inputs, so the outputs are bit-identical."""
    outputs = traced[1]
    for group in st.EQUAL_OUTPUTS:
        ref = outputs[group[0]]
        for case in group[1:]:
            assert list(outputs[case]) == list(ref)
            for k in ref:
                assert torch.equal(outputs[case][k], ref[k]), (group[0], case, k)


def test_pending_pyramid_reaches_the_differentiable_paths(traced):
    """Case L: grad mode with a pending pyramid -- every depth output requires grad, nothing else does."""
    op, outs = traced[0]["L"][-1]
    assert op == "outputs" and len(outs) == 10
    for key, (_shape, _dtype, requires_grad) in outs:
        assert requires_grad == key.endswith("_b1hw"), key
