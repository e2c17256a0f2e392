"""Times the device part of visualization.quick_viz_export for one batch of 4 frames -- ground truth 480 x 640,
prediction and lowest-cost depth 192 x 256, colour 480 x 640, everything resident on the device -- next to the same
sixteen 8-bit pictures made with the reference's sequence of torch operators on the same GPU (masked min / max, subtract,
divide, multiply, clamp, byte, long, table gather, permute; subtract and divide for the colour picture; multiply by 255
and a cast for each).  Device events around each repeat, warm-up first, median of the repeats (scripts/bench_frames.py's
bracket).  The device-to-host copy and the PNG encoding are the same for both and are not timed.

    python scripts/bench_viz.py [--repeats 30] [--warmup 5] [--out profiles/viz_quick.json]

There is no CPU path for the GPU side: without a GPU this script fails."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_frames import gpu_ms  # noqa: E402
from simplerecon_amd import synthetic  # noqa: E402
from simplerecon_amd import visualization as viz  # noqa: E402

B, H, W, h, w = 4, 480, 640, 192, 256


def torch_colormap_u8(image_1hw, vmin, vmax, table):
    """One picture with torch operators, as colormap_image and the np.uint8(... * 255) around it compute it."""
    norm = (image_1hw - vmin) / (vmax - vmin)
    idx = torch.clamp(norm * 255, 0, 255).byte().long()
    rgb = table[idx.flatten(start_dim=1)].permute([0, 2, 1]).view([-1, *image_1hw.shape[1:]])
    return (rgb.permute(1, 2, 0) * 255).to(torch.uint8)


def torch_quick_viz(outputs, cur_data, valid, table, mean, std):
    gt = cur_data["full_res_depth_b1hw"]
    if valid.sum() == 0:          # (host decisions, as in the reference: each one waits for the device)
        vmin, vmax = 0.0, 5.0
    else:
        vmin, vmax = gt[valid].min(), gt[valid].max()
    if vmax == vmin:
        vmin, vmax = 0.0, 5.0
    pictures = []
    for i in range(gt.shape[0]):
        if valid[i].sum() == 0:
            lo = hi = 0.0
        else:
            lo, hi = gt[i][valid[i]].min(), gt[i][valid[i]].max()
        if lo != hi:
            pictures.append(torch_colormap_u8(gt[i], vmin, vmax, table))
        pictures.append(torch_colormap_u8(outputs["lowest_cost_bhw"][i].unsqueeze(0), vmin, vmax, table))
        pictures.append(torch_colormap_u8(outputs["depth_pred_s0_b1hw"][i], vmin, vmax, table))
        color = (cur_data["high_res_color_b3hw"][i] - mean) / std
        pictures.append((color.permute(1, 2, 0) * 255).to(torch.uint8))
    return pictures


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viz_quick.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    gt = synthetic.raycast_scene(B, H, W, seed=3, holes=0.02)["depths"].float().unsqueeze(1).to(dev)
    pred = synthetic.raycast_scene(B, h, w, seed=3, noise=0.05)["depths"].float().unsqueeze(1).to(dev)
    lowest = synthetic.raycast_scene(B, h, w, seed=3, noise=0.2)["depths"].float().to(dev)
    mean = torch.tensor((-2.11790393, -2.03571429, -1.80444444)).view(3, 1, 1)
    std = torch.tensor((4.36681223, 4.46428571, 4.44444444)).view(3, 1, 1)
    color = (torch.rand((B, 3, H, W), generator=g) * std + mean).to(dev)
    cur = {"full_res_depth_b1hw": gt, "high_res_color_b3hw": color}
    outputs = {"depth_pred_s0_b1hw": pred, "lowest_cost_bhw": lowest}
    valid = gt > 0.5
    table = torch.flip(viz.colormap_table("turbo"), (0,)).to(dev)
    mean, std = mean.to(dev), std.to(dev)

    # the two make the same bytes
    buf, shapes = viz.quick_viz_pictures(outputs, cur, valid)
    ours = buf[(B + 1) * 8:].cpu()
    theirs = torch_quick_viz(outputs, cur, valid, table, mean, std)
    start, same = 0, True
    for k, s in enumerate(shapes):     # ours: all gt pictures, all lowest-cost, all predictions, all colour
        for i in range(B):
            n = s[1] * s[2] * 3
            same &= torch.equal(ours[start:start + n].view(s[1:]), theirs[4 * i + k].cpu())
            start += n
    if not same:
        raise SystemExit("the torch pictures differ from the kernels'")

    # the ground truth is read three times (two ranges, one picture), its mask twice
    in_bytes = 4 * (3 * gt.numel() + pred.numel() + lowest.numel() + color.numel()) + 2 * valid.numel()
    result = {"batch": B, "gt": [H, W], "pred": [h, w], "color": [H, W], "repeats": a.repeats, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0), "pictures": 4 * B, "pictures_equal": True,
              "picture_bytes": int(ours.numel()), "input_bytes_read": in_bytes}
    for name, fn in (("hip", lambda: viz.quick_viz_pictures(outputs, cur, valid)),
                     ("torch_ops", lambda: torch_quick_viz(outputs, cur, valid, table, mean, std)),
                     ("hip_again", lambda: viz.quick_viz_pictures(outputs, cur, valid)),
                     ("torch_ops_again", lambda: torch_quick_viz(outputs, cur, valid, table, mean, std))):
        med, lo, hi = gpu_ms(fn, a.warmup, a.repeats)
        result[name] = {"ms_median": med, "ms_min": lo, "ms_max": hi}
    result["torch_over_hip"] = result["torch_ops"]["ms_median"] / result["hip"]["ms_median"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
