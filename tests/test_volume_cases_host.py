"""Host-side checks of tests/volume_cases.py (no GPU): the case tables of tests/test_gpu_mlp_volume_bwd_paths.py and
tests/test_gpu_dot_volume_channels.py reach the launch shapes they are listed for, and the references of the MLP backward
are trustworthy at the project's 1e-4 bar from the oracle alone: at the persistent sizes the kink mask zeroes at most 3 % of
the cotangent and brings the fp32 and fp64 oracles to within 3e-5 of each other; at the small sizes they agree to 3e-5
without any treatment."""
import pytest

import volume_cases as vc


def test_persistent_cases_exceed_the_cu_count_with_a_ragged_tile():
    assert len(vc.PERSISTENT_CASES) >= 2
    for c in vc.PERSISTENT_CASES:
        items = vc.mlp_bwd_items(c["B"], c["h"], c["w"])
        assert items > vc.MI355X_CUS, (c["name"], items)            # some workgroup takes a second item
        assert (c["h"] * c["w"]) % 32 != 0, c["name"]               # ... and the last tile of an image is ragged
    assert vc.mlp_bwd_items(2, 77, 83) == 400
    assert any(c["K"] == 7 and vc.mlp_cin(7) == 202 for c in vc.PERSISTENT_CASES)
    for c in vc.SMALL_CASES:                                         # (the small cases are one item per workgroup)
        assert vc.mlp_bwd_items(c["B"], c["h"], c["w"]) <= vc.MI355X_CUS


def test_mlp_cases_hit_every_dw1_instantiation():
    assert [vc.mlp_bwd_nt1(K) for K in (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 15)] == [4, 4, 4, 4, 7, 7, 10, 10, 10, 13, 13]
    assert {vc.mlp_bwd_nt1(c["K"]) for c in vc.MLP_CASES} == {4, 7, 10, 13}
    assert {c["K"] for c in vc.VIEW_CASES} == {1, 4, 5, 9, 11, 12}
    # K = 5: two wholly unused column tiles whose reads run past the 150-float feature row; K = 11 fills NT1 = 10
    assert vc.mlp_bwd_nt1(5) - (vc.mlp_cin(5) + 31) // 32 == 2 and (vc.mlp_cin(11) + 31) // 32 == 10
    assert all(vc.mlp_cin(c["K"]) <= 416 for c in vc.MLP_CASES)
    assert vc.BATCH_CASE["B"] >= 3 and vc.EDGE_CASE["K"] == 4 and vc.EDGE_CASE["edge"] and vc.PIXEL_PLANES_CASE["pixel_planes"]


def test_dot_shapes_take_the_three_generic_launch_shapes():
    for want, s in vc.DOT_SHAPES.items():
        got, S = vc.dot_launch_shape(s["B"], s["h"], s["w"], s["D"])
        assert got == want, (want, got, S)
    s = vc.DOT_SHAPES["spread"]
    assert (s["B"], s["h"], s["w"], s["D"]) == (2, 37, 29, 5) and vc.dot_launch_shape(2, 37, 29, 5) == ("spread", 4)
    s = vc.DOT_SHAPES["workgroup"]
    assert s["B"] * ((s["h"] * s["w"] + 63) // 64) >= 1024 and s["D"] >= 4
    assert vc.dot_launch_shape(s["B"], s["h"], s["w"], s["D"]) == ("workgroup", 4)
    # both split shapes leave the last plane group without a plane (ceil(5 / 4) = 2 planes per group: 2 + 2 + 1 + 0)
    assert vc.DOT_SHAPES["nosplit"]["D"] == 1
    assert 16 not in vc.DOT_CHANNELS and set(vc.DOT_WORKGROUP_CHANNELS) <= set(vc.DOT_CHANNELS)
    assert all(64 % C != 0 for C in vc.DOT_BWD_EDGE_CHANNELS)       # the scatter leaves the last lanes of a wave idle
    # the split rule by hand: 80 tiles -> 16 groups; 2400 tiles -> 2 (4800 waves >= 4096); 4800 tiles -> no split
    assert vc.dot_plane_split(1, 64 * 80, 64) == 16 and vc.dot_plane_split(8, 120 * 160, 64) == 2
    assert vc.dot_plane_split(16, 120 * 160, 64) == 1 and vc.dot_plane_split(1, 64 * 80, 5) == 4


@pytest.mark.parametrize("name", [c["name"] for c in vc.PERSISTENT_CASES])
def test_at_size_kink_share_and_oracle_agreement(name):
    ref = vc.at_size_reference(name)
    print(f"{name}: zeroed share {ref['share']:.4f}, f32 vs f64 oracle {ref['agree']:.3e}")
    assert 0.0 < ref["share"] <= vc.KINK_SHARE_MAX, ref["share"]
    assert ref["agree"] <= vc.ORACLE_AGREE_MAX, ref["agree"]


@pytest.mark.parametrize("case", vc.SMALL_CASES, ids=lambda c: c["name"])
def test_small_cases_need_no_kink_treatment(case):
    inp, mlp = vc.inputs(case), vc.mlp_dict(vc.manager(case))
    agree, _ = vc.oracle_agreement(case, inp, mlp, vc.cotangent(case))
    print(f"{case['name']}: f32 vs f64 oracle {agree:.3e}")
    assert agree <= vc.ORACLE_AGREE_MAX, agree
