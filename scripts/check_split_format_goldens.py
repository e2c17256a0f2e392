"""Checks the re-recording of tests/golden/conv2d_dispatch.json.gz and tests/golden/conv_layer_trace.json.gz for the change
that made the Winograd split format an argument (`split_format` of sr_wino_pack_weights and
sr_conv3x3_wino_splitk_nhwc_fwd): against the goldens of git revision REV (default HEAD^, the commit before the change)
    python scripts/check_split_format_goldens.py [REV]
the case ids are the same, every trace is the same once the one inserted integer is deleted from each of those two calls, that
integer is the case's split answer (0 throughout the layer trace, which never sets the option), and the pack and the launch
of a case carry the same integer.  Prints a one-line summary; any difference is an assertion."""
import gzip
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REV = sys.argv[1] if len(sys.argv) > 1 else "HEAD^"
# where the inserted integer sits in a pinned call [name, arg0, arg1, ...] (tests/test_host_logic_stub.py::_pinned_call)
INSERTED = {"sr_wino_pack_weights": 1 + 3, "sr_conv3x3_wino_splitk_nhwc_fwd": 1 + 17}
FORMATS = {"": 0, "bf16": 1, "f16": 2}
seen = {name: 0 for name in INSERTED}


def load(path, rev=None):
    raw = open(os.path.join(ROOT, path), "rb").read() if rev is None else \
        subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{path}"], check=True, capture_output=True).stdout
    return json.loads(gzip.decompress(raw))


def strip(node, fmt, carried, cid):
    """`node` with the inserted integer deleted from every pinned call of the two entry points (checked against `fmt`)."""
    if isinstance(node, dict):
        return {k: strip(v, fmt, carried, cid) for k, v in node.items()}
    if not isinstance(node, list):
        return node
    if node and isinstance(node[0], str) and node[0] in INSERTED:
        at = INSERTED[node[0]]
        assert node[at] == fmt, (cid, node[0], node[at], fmt)
        carried.add(node[at])
        seen[node[0]] += 1
        return node[:at] + node[at + 1:]
    return [strip(v, fmt, carried, cid) for v in node]


def check(path, fmt_of):
    old, new = load(path, REV), load(path)
    assert sorted(old) == sorted(new), f"{path}: case ids differ"
    with_calls = 0
    for cid in old:
        carried = set()
        assert strip(new[cid], fmt_of(cid), carried, cid) == old[cid], (path, cid)
        assert len(carried) <= 1, (path, cid, carried)   # the pack and the launch of a case carry one format
        with_calls += bool(carried)
    return len(old), with_calls


n_d, w_d = check("tests/golden/conv2d_dispatch.json.gz", lambda cid: FORMATS[cid.split("/")[0].split("-")[9]])
n_l, w_l = check("tests/golden/conv_layer_trace.json.gz", lambda cid: 0)
print(f"{n_d} dispatch cases ({w_d} with Winograd F(2x2) calls) and {n_l} layer cases ({w_l}): same ids, traces equal to {REV}'s "
      f"after deleting split_format from {seen['sr_wino_pack_weights']} pack and {seen['sr_conv3x3_wino_splitk_nhwc_fwd']} "
      f"launch calls; it equals the case's split answer everywhere (0 in the layer trace)")
