"""Records tests/golden/decoder_schedule_trace.json.gz: the launch trace of DepthModel's inference schedule that
tests/test_gpu_schedule_trace.py::test_inference_schedule_trace_matches_the_golden compares against (the cases and what is
recorded of each are tests/schedule_trace.py's).  Needs the GPU: the fork / join logic does not run without one.
    python scripts/record_decoder_schedule_trace.py [TREE]
TREE: another checkout (built) whose simplerecon_amd package is traced instead of this one -- the fixture pins the behaviour of
the commit BEFORE a change to the schedule, so it is recorded from that commit with this tree's helper.  Also checks the output
equalities of tests/test_gpu_schedule_trace.py and says which hold."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT, os.path.join(ROOT, "tests")]
import torch
import schedule_trace as st
import simplerecon_amd

traces, outputs = st.run_cases()
for group in st.EQUAL_OUTPUTS:
    for case in group[1:]:
        same = all(torch.equal(outputs[case][k], v) for k, v in outputs[group[0]].items())
        print(f"outputs {group[0]} == {case}: {same}")
size = st.write_golden(traces)
print(f"{len(traces)} cases ({', '.join(f'{c}: {len(t)}' for c, t in traces.items())} records) of "
      f"{os.path.dirname(simplerecon_amd.__file__)} -> {st.GOLDEN}, {size} bytes")
