"""Case table and launch-plan arithmetic of tests/test_gpu_persistent_rounds.py: the persistent inference kernels
(csrc/sr_matching.hip: sr_t16_kernel, sr_stem_kernel, sr_conv1x1_stats_kernel; csrc/sr_wino4.hip: the three F(4x4) forms) at
sizes where a workgroup takes a second and a third work item, so that what is carried from one item to the next (LDS buffers
handed over, prefetch registers, barrier protocols, XCD index remaps) is run and checked.

Everything here runs on any device: the GPU module uses it for its shapes and to attribute an error to (item, workgroup,
trip); tests/test_persistent_cases_host.py checks the table and the maps on the CPU for several CU counts.

The plan arithmetic RESTATES the launchers on purpose (there is no library query for a launch's grid): a case asserts the
property it is listed for from these numbers.  The multi-round property carries a margin of a third of a round, so that a small
change of a workgroups-per-CU constant does not silently turn a multi-round case into a one-round one.

A plan is dict(total, grid, workers, item, worker, trip): `total` work items, `grid` workgroups, and three equally long arrays
that enumerate the launch the way the kernel walks it -- worker `worker[i]` runs item `item[i]` as its trip `trip[i]` (0 = its
first item).  A worker is a workgroup, except in the ping-pong F(4x4) form, where each of a workgroup's two 4-wave groups
walks its own list (worker = 2 * workgroup + group)."""
import numpy as np

GIB = 1 << 30


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------- item counts --------
def t16_items(B, H, W):
    """sr_conv3x3_c16_nhwc_fwd (sr_matching.hip:845-846): 8 x 16 output pixels of one image; tile = (b, ty, tx), tx fastest."""
    return cdiv(W, 16) * cdiv(H, 8) * B


def stem_items(B, H, W):
    """sr_stem7x7_fwd (sr_matching.hip:880-882): 16 x 16 tiles of the (H - 1) // 2 + 1 x (W - 1) // 2 + 1 output."""
    return cdiv((W - 1) // 2 + 1, 16) * cdiv((H - 1) // 2 + 1, 16) * B


def c1s_items(B, H, W):
    """sr_conv1x1_stats_nhwc_fwd (sr_matching.hip:1002): 64 consecutive pixels of one image."""
    return cdiv(H * W, 64) * B


def wino4_items(B, H, W, Cout):
    """w4_run (sr_wino4.hip:1096-1101): 16 x 16 regions x blocks of 64 output channels; item = (cb, b, ry, rx), rx fastest."""
    return cdiv(W, 16) * cdiv(H, 16) * cdiv(Cout, 64) * B


# ------------------------------------------------------------------------------------------- walks --------------
def _round_robin(total, grid, workers=None):
    work = np.arange(total)
    return dict(total=total, grid=grid, workers=workers or grid, item=work, worker=work % (workers or grid),
                trip=work // (workers or grid))


def t16_plan(total, cus):
    """grid = min(3 * CUs, total) (sr_matching.hip:848-849); `for (work = blockIdx.x; work < total; work += gridDim.x)` with
    the XCD remap of a FULL round of a grid that is a multiple of 8 (sr_matching.hip:702-709):
        r0 = work / G * G;  if (r0 + G <= total) { bb = work - r0; tile = r0 + (bb & 7) * (G >> 3) + (bb >> 3); }
    The partial last round is walked in launch order."""
    G = min(3 * cus, total)
    p = _round_robin(total, G)
    work = p["item"]
    if G % 8 == 0:
        r0 = work // G * G
        bb = work - r0
        p["item"] = np.where(r0 + G <= total, r0 + (bb & 7) * (G >> 3) + (bb >> 3), work)
    return p


def stem_plan(total, cus):
    """grid = min(2 * CUs, total) (sr_matching.hip:883-884); `for (tile = blockIdx.x; tile < total; tile += gridDim.x)` (:106)."""
    return _round_robin(total, min(2 * cus, total))


def c1s_plan(total, cus):
    """grid = min(3 * CUs, total) (sr_matching.hip:1003-1004); `for (; item < total; item += gridDim.x)` (:589-591)."""
    return _round_robin(total, min(3 * cus, total))


def wino4_plan(total, cus):
    """The 4-wave form: grid = min(2 * CUs, total) (sr_wino4.hip:1120-1121); work = blockIdx.x, += gridDim.x (:330-337)."""
    return _round_robin(total, min(2 * cus, total))


def wino4pp_plan(total, cus):
    """The ping-pong form: grid = min(CUs, ceil(total / 2)) (sr_wino4.hip:1126-1127); group g of workgroup b walks
    slot = 2 b + g, slot + 2 * gridDim.x, ... (:399-401)."""
    G = min(cus, (total + 1) // 2)
    return _round_robin(total, G, workers=2 * G)


def wino4ws_plan(total, cus):
    """The wave-specialised form: grid = min(CUs, total) (sr_wino4.hip:1104-1105); every XCD walks a contiguous eighth of the
    items (:692-696):  xcd = b & 7;  n_x = (grid - xcd + 7) >> 3;  x_chunk = (total + 7) >> 3;
    first = xcd * x_chunk + (b >> 3);  stride n_x;  end = min(total, (xcd + 1) * x_chunk)."""
    G = min(cus, total)
    b = np.arange(G)
    xcd = b & 7
    n_x = (G - xcd + 7) >> 3
    x_chunk = (total + 7) >> 3
    first = xcd * x_chunk + (b >> 3)
    end = np.minimum(total, (xcd + 1) * x_chunk)
    n_items = np.where(first < end, (end - first + n_x - 1) // n_x, 0)
    worker = np.repeat(b, n_items)
    trip = np.arange(int(n_items.sum())) - np.repeat(np.cumsum(n_items) - n_items, n_items)
    return dict(total=total, grid=G, workers=G, item=first[worker] + trip * n_x[worker], worker=worker, trip=trip)


PLANS = {"t16": t16_plan, "stem": stem_plan, "c1s": c1s_plan, "w4": wino4_plan, "w4_pp": wino4pp_plan, "w4_ws": wino4ws_plan}
PER_CU = {"t16": 3, "stem": 2, "c1s": 3, "w4": 2, "w4_pp": 1, "w4_ws": 1}     # grid = min(PER_CU * CUs, ...)


def attribution(plan):
    """(worker of item, trip of item), after checking that the walk runs every item exactly once and no worker runs two items
    in one trip."""
    total = plan["total"]
    item, worker, trip = plan["item"], plan["worker"], plan["trip"]
    assert len(item) == total and np.array_equal(np.sort(item), np.arange(total)), "the walk does not cover every item once"
    assert worker.min() >= 0 and worker.max() < plan["workers"] and trip.min() >= 0
    slots = worker.astype(np.int64) * (int(trip.max()) + 1) + trip
    assert len(np.unique(slots)) == total, "two items in one (worker, trip)"
    w_of, t_of = np.empty(total, np.int64), np.empty(total, np.int64)
    w_of[item], t_of[item] = worker, trip
    return w_of, t_of


def items_per_worker(plan):
    return np.bincount(plan["worker"], minlength=plan["workers"])


# ------------------------------------------------------------------------------------------- the cases ----------
# kind "multi": items >= 2 * grid + grid // 3 on the device's full grid (two full rounds and a partial third).  The three F(4x4)
# forms run the same operands: the batch is sized for the 4-wave form's 2 * CUs workgroups (= the ping-pong form's 4-wave
# groups), which gives the wave-specialised form, the one every production launch takes, 4 2/3 rounds -- unless the case's
# tensors would then pass 1 GiB (192 channels on a 304-CU device); then for the wave-specialised form's CUs workgroups alone,
# and the other two forms reach a second trip only.
# kind "uneven": one round of the wave-specialised form on 60-100 % of the CUs whose total is not a multiple of 8, so that the XCD
# split hands one workgroup two items and lets others return with none (`pick`: the smallest / largest such batch).
# kind "fixed": the batch is given; the case exists on the devices where that batch has the split's property (w4_uneven_b7).
def _t16(name, ci, co, mode, norm, act, sliced=False):
    return dict(name=name, op="t16", kind="multi", H=37, W=72, ci=ci, co=co, mode=mode, norm=norm, act=act, sliced=sliced)


def _w4(name, ci, co, kind="multi", H=56, W=72, **kw):
    return dict(name=name, op="w4", kind=kind, H=H, W=W, ci=ci, co=co, **kw)


CASES = [
    # 37 x 72 maps: 5 x 5 items per image, ragged at the bottom (37 = 4 * 8 + 5) and the right (72 = 4 * 16 + 8)
    _t16("t16_tail_128_16", 128, 16, "replicate", True, True),      # the matching encoder's production tail: 4 slabs
    _t16("t16_one_slab_32_12", 32, 12, "zeros", True, True),        # no double-buffer hand-over inside an item; a Cout tail
    _t16("t16_norm_no_act_64", 64, 16, "zeros", True, False),       # sr_t16_kernel<true, false>
    _t16("t16_act_no_norm_64", 64, 16, "replicate", False, True),   # sr_t16_kernel<false, true>
    _t16("t16_slices_64_12", 64, 12, "replicate", True, True, sliced=True),   # channels [4:68] of 72 -> [4:16] of 20
    # 100 x 140 images: 50 x 70 outputs, 4 x 5 tiles, ragged (50 = 3 * 16 + 2, 70 = 4 * 16 + 6)
    dict(name="stem_bn_relu", op="stem", kind="multi", H=100, W=140, bn=True, leaky=0.0),
    dict(name="stem_bias_only", op="stem", kind="multi", H=100, W=140, bn=False, leaky=None),
    # 17 x 23 = 391 pixels: 7 items per image, the last one 7 pixels
    dict(name="c1s_64_128", op="c1s", kind="multi", H=17, W=23),
    # 56 x 72 maps: 4 x 5 regions, ragged (56 = 3 * 16 + 8, 72 = 4 * 16 + 8); residual and LeakyReLU(0.2) on
    _w4("w4_s1_16_64", 16, 64),          # S = 1: the one-slab tick protocol (barrier B4, residual loads after the cursor advance)
    _w4("w4_s3_48_64", 48, 64),          # S = 3
    _w4("w4_s2_24_64", 24, 64),          # S = 2 with a Cin tail (24 = 16 + 8)
    _w4("w4_s8_128_128", 128, 128),      # S = 8, two output-channel blocks, B > 1: the cursor carries into the next image
    _w4("w4_s12_192_64", 192, 64),       # S = 12
    # 56 x 72 x 128 channels is 40 items per image: every total is a multiple of 8, the XCD chunks end on the channel-block
    # boundary and no walk of the wave-specialised form crosses it.  40 x 72 maps (3 x 5 regions, 30 items per image) at a batch
    # whose total is no multiple of 8: XCD 3's chunk straddles the boundary and w4_cursor_advance carries into block 1 mid-walk
    _w4("w4_s8_128_128_block_carry", 128, 128, H=40, W=72, carry=True),
    _w4("w4_uneven_low", 64, 64, kind="uneven", H=60, W=80, pick="low"),
    _w4("w4_uneven_high", 64, 64, kind="uneven", H=60, W=80, pick="high"),
    # B = 7 at 60 x 80 = 140 items (the example of ADVICE.md's finding on the XCD split): below 60 % of 256 CUs, so the
    # property is the split's alone -- one round, not a multiple of 8, a workgroup with two items and one with none
    _w4("w4_uneven_b7", 64, 64, kind="fixed", H=60, W=80, B=7),
]
BY_NAME = {c["name"]: c for c in CASES}


def items_of(case, B):
    if case["op"] == "t16":
        return t16_items(B, case["H"], case["W"])
    if case["op"] == "stem":
        return stem_items(B, case["H"], case["W"])
    if case["op"] == "c1s":
        return c1s_items(B, case["H"], case["W"])
    return wino4_items(B, case["H"], case["W"], case["co"])


def case_plan(case, B, cus, form=None):
    """The walk of the case's kernel (`form`: which F(4x4) form, default the wave-specialised one)."""
    key = case["op"] if case["op"] != "w4" else (form or "w4_ws")
    return PLANS[key](items_of(case, B), cus)


def multi_round(total, full_grid):
    """At least two full rounds and a third of a round more: a remapped round, a second one and an unremapped tail."""
    return total >= 2 * full_grid + full_grid // 3


def one_round_split(total, cus):
    """The XCD split of one round with an uneven total: a workgroup with two items, and one with none."""
    if total > cus or total % 8 == 0:
        return False
    n = items_per_worker(wino4ws_plan(total, cus))
    return bool(n.max() == 2 and n.min() == 0)


def one_round_uneven(total, cus):
    return 0.6 * cus <= total and one_round_split(total, cus)


def walk_crosses_blocks(case, B, cus):
    """Some workgroup of the wave-specialised form goes from an item of output-channel block 0 to one of block 1."""
    plan = case_plan(case, B, cus)
    half = plan["total"] // 2
    lo = np.bincount(plan["worker"], weights=plan["item"] < half, minlength=plan["workers"])
    hi = np.bincount(plan["worker"], weights=plan["item"] >= half, minlength=plan["workers"])
    return bool(((lo > 0) & (hi > 0)).any())


def shape_for(case, cus):
    """The batch size at which the case has its property on a device of `cus` compute units, or None (with the uneven
    cases: no such batch exists)."""
    if case["kind"] == "fixed":
        return case["B"] if one_round_split(items_of(case, case["B"]), cus) else None
    per_image = items_of(case, 1)
    if case["kind"] == "multi":
        full = PER_CU[case["op"] if case["op"] != "w4" else "w4"] * cus
        B = cdiv(2 * full + full // 3, per_image)
        if case["op"] == "w4" and case_bytes(case, B + 1 if case.get("carry") else B) >= GIB:
            B = cdiv(2 * cus + cus // 3, per_image)
        while case.get("carry") and not walk_crosses_blocks(case, B, cus):
            B += 1
        return B
    good = [B for B in range(1, cus // per_image + 1) if one_round_uneven(B * per_image, cus)]
    if not good or (case["pick"] == "high" and len(good) == 1):
        return None
    return good[0] if case["pick"] == "low" else good[-1]


def has_property(case, B, cus):
    total = items_of(case, B)
    if case["kind"] == "multi":
        plan = case_plan(case, B, cus)
        return multi_round(total, plan["grid"]) and int(plan["trip"].max()) >= 2
    if case["kind"] == "uneven":
        return one_round_uneven(total, cus)
    return one_round_split(total, cus)


def case_bytes(case, B):
    """fp32 input, output and residual of the case with a float64 copy of each (the reference works on those)."""
    H, W = case["H"], case["W"]
    if case["op"] == "t16":
        wide = 8 if case["sliced"] else 0
        elems = B * H * W * (case["ci"] + wide + case["co"] + wide)
    elif case["op"] == "stem":
        elems = B * (3 * H * W + 64 * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1))
    elif case["op"] == "c1s":
        elems = B * H * W * (64 + 128)
    else:
        elems = B * H * W * (case["ci"] + 2 * case["co"])
    return elems * (4 + 8)


# ------------------------------------------------------------------------------------------- output -> item -----
def item_of_output(case, B, b, c, y, x):
    """The work item that writes output element (b, c, y, x); any mix of integers and broadcastable integer arrays / tensors."""
    H, W = case["H"], case["W"]
    if case["op"] == "t16":
        return (b * cdiv(H, 8) + y // 8) * cdiv(W, 16) + x // 16 + 0 * c
    if case["op"] == "stem":
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        return (b * cdiv(Ho, 16) + y // 16) * cdiv(Wo, 16) + x // 16 + 0 * c
    if case["op"] == "c1s":
        return b * cdiv(H * W, 64) + (y * W + x) // 64 + 0 * c
    return ((c // 64 * B + b) * cdiv(H, 16) + y // 16) * cdiv(W, 16) + x // 16
