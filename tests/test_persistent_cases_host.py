"""Host-side checks of tests/persistent_cases.py (no GPU): on devices of 64, 104, 256 and 304 compute units every case of
tests/test_gpu_persistent_rounds.py has the property it is listed for, and the restated item -> (workgroup, trip) maps, which
the GPU module uses to say WHERE an error sits, run every item exactly once.  (The maps are restatements of the kernels' loops;
this guards the helper, it does not stand in for the kernels.)"""
import numpy as np
import pytest

import persistent_cases as pc

CUS = (64, 104, 256, 304)


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("case", pc.CASES, ids=[c["name"] for c in pc.CASES])
def test_case_has_its_property(case, cus):
    B = pc.shape_for(case, cus)
    if B is None:
        assert case["kind"] != "multi" and cus != 256, "on 256 CUs no case may be without a shape"
        return
    total = pc.items_of(case, B)
    assert pc.has_property(case, B, cus), (case["name"], cus, B, total)
    assert pc.case_bytes(case, B) < pc.GIB, (case["name"], cus, B, pc.case_bytes(case, B))
    if case["kind"] == "multi":
        plan = pc.case_plan(case, B, cus)
        assert plan["grid"] == pc.PER_CU[case["op"] if case["op"] != "w4" else "w4_ws"] * cus
        assert total >= 2 * plan["grid"] + plan["grid"] // 3
        trips = np.bincount(plan["trip"])
        assert len(trips) >= 3 and trips[0] == trips[1] == plan["grid"] and 0 < trips[-1], trips
        if case["op"] == "t16":     # two remapped rounds, then a tail in launch order
            G, work = plan["grid"], np.arange(total)
            assert G % 8 == 0
            moved = plan["item"] != work
            assert moved[:G].any() and moved[G:2 * G].any() and not moved[total // G * G:].any()
            assert total % G != 0
        if case["op"] == "w4":      # the other two forms: three trips as well, unless that size would pass 1 GiB
            for form in ("w4", "w4_pp"):
                other = pc.case_plan(case, B, cus, form)
                assert other["trip"].max() >= 1
                if cus == 256 or pc.case_bytes(case, 2 * B) < pc.GIB:
                    assert pc.multi_round(total, other["workers"]) and other["trip"].max() >= 2, (form, total)
            if case["co"] > 64:     # a later trip crosses into the next image and into the second channel block
                assert B > 1
                w_of, t_of = pc.attribution(plan)
                per_block = total // 2
                assert t_of[per_block:].max() >= 1 and t_of[:per_block].max() >= 1
                assert pc.walk_crosses_blocks(case, B, cus) == bool(case.get("carry"))
    else:
        n = pc.items_per_worker(pc.wino4ws_plan(total, cus))
        assert total <= cus and total % 8 != 0 and n.max() == 2 and n.min() == 0
        if case["kind"] == "uneven":
            assert 0.6 * cus <= total


def test_on_256_cus_the_table_is_the_one_the_issue_names():
    B = {c["name"]: pc.shape_for(c, 256) for c in pc.CASES}
    assert all(b is not None for b in B.values()), B
    assert B["t16_tail_128_16"] == 72 and pc.items_of(pc.BY_NAME["t16_tail_128_16"], 72) == 1800
    assert B["stem_bn_relu"] == 60 and pc.items_of(pc.BY_NAME["stem_bn_relu"], 60) == 1200
    assert B["c1s_64_128"] == 256 and pc.items_of(pc.BY_NAME["c1s_64_128"], 256) == 1792
    assert B["w4_s1_16_64"] == 60 and B["w4_s12_192_64"] == 60 and B["w4_s8_128_128"] == 30
    assert (B["w4_uneven_low"], B["w4_uneven_high"], B["w4_uneven_b7"]) == (9, 11, 7)
    assert pc.items_of(pc.BY_NAME["w4_uneven_low"], 9) == 180 and pc.items_of(pc.BY_NAME["w4_uneven_b7"], 7) == 140
    # the slab counts of the F(4x4) multi-round cases: 1, 3, 2 (with a Cin tail), 8 (two channel blocks), 12
    S = sorted({pc.cdiv(c["ci"], 16) for c in pc.CASES if c["op"] == "w4" and c["kind"] == "multi"})
    assert S == [1, 2, 3, 8, 12]
    assert B["w4_s8_128_128_block_carry"] == 41 and 30 * 41 % 8 != 0
    # ADVICE.md's reading of the split at 140 items: XCDs 5 and 6 have 18 items and 17 workgroups
    plan = pc.wino4ws_plan(140, 256)
    n = pc.items_per_worker(plan)
    for xcd in (5, 6):
        mine = n[xcd::8]
        assert len(mine) == 17 and mine.sum() == 18 and mine.max() == 2


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("kernel", list(pc.PLANS))
def test_every_item_runs_exactly_once(kernel, cus):
    for total in range(1, 3001):
        plan = pc.PLANS[kernel](total, cus)
        want = min(pc.PER_CU[kernel] * cus, total if kernel != "w4_pp" else (total + 1) // 2)
        assert plan["grid"] == want, (kernel, cus, total)
        try:
            w_of, t_of = pc.attribution(plan)
        except AssertionError as e:
            raise AssertionError(f"{kernel}, {cus} CUs, {total} items: {e}") from None
        # a worker's trips are 0, 1, ... without a gap
        n = pc.items_per_worker(plan)
        assert np.array_equal(np.bincount(plan["worker"], weights=plan["trip"], minlength=plan["workers"]), n * (n - 1) / 2)


def test_item_of_output_matches_the_kernels_decode():
    """item_of_output against the decode written out as the kernels have it (tile -> tx, ty, b; w4_decode)."""
    for name, B in (("t16_tail_128_16", 3), ("stem_bn_relu", 2), ("c1s_64_128", 3), ("w4_s8_128_128", 3)):
        case = pc.BY_NAME[name]
        H, W = case["H"], case["W"]
        total = pc.items_of(case, B)
        seen = np.zeros(total, np.int64)
        if case["op"] == "stem":
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        co = {"t16": case.get("co"), "stem": 64, "c1s": 128, "w4": case.get("co")}[case["op"]]
        b, c, y, x = np.meshgrid(np.arange(B), np.arange(co), np.arange(H), np.arange(W), indexing="ij")
        item = pc.item_of_output(case, B, b, c, y, x)
        assert item.min() == 0 and item.max() == total - 1
        if case["op"] in ("t16", "stem"):
            th, tw = (8, 16) if case["op"] == "t16" else (16, 16)
            tiles_x, tiles_y = pc.cdiv(W, tw), pc.cdiv(H, th)
            tx, ty, bb = item % tiles_x, (item // tiles_x) % tiles_y, item // (tiles_x * tiles_y)
            assert np.array_equal(bb, b) and np.array_equal(ty, y // th) and np.array_equal(tx, x // tw)
        elif case["op"] == "c1s":
            tiles = pc.cdiv(H * W, 64)
            assert np.array_equal(item // tiles, b) and np.array_equal((item % tiles) * 64 // 64, (y * W + x) // 64)
        else:
            rx_n, ry_n = pc.cdiv(W, 16), pc.cdiv(H, 16)
            rem = item
            rx, rem = rem % rx_n, rem // rx_n
            ry, rem = rem % ry_n, rem // ry_n
            assert np.array_equal(rem % B, b) and np.array_equal(rem // B * 64, c // 64 * 64)
            assert np.array_equal(ry * 16, y // 16 * 16) and np.array_equal(rx * 16, x // 16 * 16)
        np.add.at(seen, item.ravel(), 1)
        assert seen.min() > 0
