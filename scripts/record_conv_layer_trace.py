"""Records tests/golden/conv_layer_trace.json.gz: the launch trace of autograd_ops._ConvBiasAct that
tests/test_host_logic_stub.py::test_conv_layer_launch_trace_matches_the_golden compares against (the cases and what is recorded
of each are that test's: _layer_cases / _layer_trace).  Runs on the CPU against the test's stub of the library.
    python scripts/record_conv_layer_trace.py [TREE]
TREE: another checkout (built) whose simplerecon_amd package is traced instead of this one -- the fixture pins the behaviour of
the commit BEFORE a change to the layer, so it is recorded from that commit with this tree's test."""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT, os.path.join(ROOT, "tests")]
import pytest
import test_host_logic_stub as t
import simplerecon_amd

with pytest.MonkeyPatch.context() as mp:
    traces = t._layer_traces(t.make_stub(mp), mp)
with open(t._GOLDEN_LAYER, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:
    z.write(json.dumps(traces, sort_keys=True, separators=(",", ":")).encode())
raising = [cid for cid, tr in traces.items() if "raises" in tr]
print(f"{len(traces)} cases ({len(raising)} raise) of {os.path.dirname(simplerecon_amd.__file__)} -> {t._GOLDEN_LAYER}, "
      f"{os.path.getsize(t._GOLDEN_LAYER)} bytes")
