"""The ops.PROFILE records of real launches -- kernel name, algorithmic FLOPs, shape, executed FLOPs -- equal what
tests/golden/launch_records.json holds for the cases of tests/launch_record_cases.py.  The fixture was recorded on an MI355X
from the commit BEFORE the launchers reported their own kernel (scripts/record_launch_records.py): then ops.py worked the
name and the executed FLOPs out a second time, in Python; now the library's launch sites note them (sr_last_launch).  One
record differs on purpose: F(4x4) form 2 launches sr_wino4pp_kernel, which the Python restatement called sr_wino4_kernel."""
import json
import os

import pytest

import launch_record_cases as cases

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_records.json")
RENAMED = {"wino4/form2": ("sr_wino4_kernel", "sr_wino4pp_kernel"), "wino4/form2+res": ("sr_wino4_kernel", "sr_wino4pp_kernel")}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    cus = cases.device_cus()
    if cus != g["cus"]:   # (launch plans follow the CU count)
        pytest.skip(f"the fixture was recorded on a device with {g['cus']} CUs, this one has {cus}")
    return g["records"]


def test_the_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(cases.CASE_IDS)


@pytest.mark.parametrize("cid", cases.CASE_IDS)
def test_records_match_the_parent_recorded_fixture(cid, golden):
    want = [list(r) for r in golden[cid]]
    if cid in RENAMED:
        old, new = RENAMED[cid]
        assert [r[0] for r in want] == [old]
        want[0][0] = new
    got = cases.run(cid)
    print(f"{cid}: {got}")
    assert got == want
