"""The reference's test loop (test.py:203-455) without its datasets: run the model over the frames of each scan, score
every frame on the GPU (metrics.score_block: nearest upsample to the ground truth, gt > 0.5, the batched rule with
mult_a=True, in two launches), average per scene and over all frames / scenes with ResultsAverager, write the
reference's score files and, optionally, fuse the depths into a TSDF and export one mesh per scan.

    scans = [("scene0707_00", frames), ...]     # frames: iterable of (cur_data, src_data), one frame each
    frame_avg, scene_avg = evaluate(model, scans, "results/hero", "hero", batch_size=4)

A frame is what a dataset's __getitem__ returns: dicts with the reference's keys (image_b3hw, full_res_depth_b1hw,
K_full_depth_b44, cam_T_world_b44, world_T_cam_b44, K_s1_b44, invK_s1_b44, ... for the current frame; the source frames'
images, poses and intrinsics stacked along a first dimension), without a batch dimension.  `batch_size` frames are
collated into one batch, as test.py's DataLoader does (drop_last=False).  frames.FramePreparer.tuple makes such frames
from decoded images."""
import os

import torch
import torch.nn.functional as F
from torch.utils.data import default_collate

from . import metrics

MIN_DEPTH = 0.5   # test.py: inf max depth matches DVMVS metrics, 0.5 m minimum


def _batches(frames, batch_size):
    batch = []
    for item in frames:
        batch.append(item)
        if len(batch) == batch_size:
            yield default_collate(batch)
            batch = []
    if batch:
        yield default_collate(batch)


def _to(d, device):
    return {k: (v.to(device, non_blocking=True) if torch.is_tensor(v) else v) for k, v in d.items()}


def _upsample_nearest(x_bhw, size):
    return F.interpolate(x_bhw.unsqueeze(1).float(), size=size, mode="nearest")


def _model_device(model):
    for p in model.parameters():
        return p.device
    return torch.device("cuda")


def _mesh_folder(fuser, mask_pred_depth, fusion_use_raw_lowest_cost, fuse_color=False):
    """test.py's mesh folder name (test.py:139-146): {fusion_resolution}_{max depth}_{depth fuser}, then _masked /
    _color / _raw_cv.  The fuser's name is its `depth_fuser` attribute ("ours" when it has none)."""
    name = (f"{getattr(fuser, 'fusion_resolution', 0.04)}_{getattr(fuser, 'max_fusion_depth', 3)}_"
            f"{getattr(fuser, 'depth_fuser', 'ours')}")
    if mask_pred_depth:
        name += "_masked"
    if fuse_color:
        name += "_color"
    if fusion_use_raw_lowest_cost:
        name += "_raw_cv"
    return name


def evaluate(model, scans, output_dir, name, split="test", batch_size=4, run_fusion=False, fuser_factory=None,
             mask_pred_depth=False, fusion_use_raw_lowest_cost=False, gt_mesh_factory=None, depth_fuser="ours",
             fuse_color=False, dump_depth_visualization=False):
    """Scores `model` on `scans` as test.py does and writes output_dir/scores/{scan}_metrics.json (`/` in the scan
    name becomes `_`), all_scene_avg_metrics_{split}.json and all_frame_avg_metrics_{split}.json.  With run_fusion,
    `fuser_factory(scan_name)` (default: on the model's device, tsdf.OurFuser for depth_fuser="ours" or
    scalable_tsdf.Open3DFuser(fuse_color=fuse_color) for depth_fuser="open3d") fuses the nearest-upsampled depths --
    set to -1 outside the cost volume's overall mask with mask_pred_depth, or replaced by the cost volume's lowest-cost
    depths with fusion_use_raw_lowest_cost -- and each scan's mesh goes to output_dir/meshes/<folder>/{scan}.ply, <folder> as test.py names it:
    {fusion_resolution}_{max depth}_{fuser's depth_fuser}[_masked][_color][_raw_cv].
    With run_fusion and `gt_mesh_factory(scan_name)` returning a ground truth (a TriangleMesh, a PointCloud or a PLY path; None skips the
    scan), the exported mesh is scored against it by mesh_metrics.mesh_metrics with its defaults, into
    scores/{scan}_mesh_metrics.json and all_scene_avg_mesh_metrics_{split}.json.
    With dump_depth_visualization (test.py --dump_depth_visualization), visualization.quick_viz_export writes four PNGs
    per frame -- ground truth, lowest-cost and predicted depth, colour -- to output_dir/viz/quick_viz/{scan}/, with
    valid_mask_b = full_res_depth_b1hw > 0.5 (test.py:172-177, 375-388); the scores are not affected.

    Returns (all_frame_metrics, all_scene_metrics), the two top-level ResultsAveragers with final averages."""
    device = _model_device(model)
    scores_dir = os.path.join(output_dir, "scores")
    os.makedirs(scores_dir, exist_ok=True)
    if depth_fuser not in ("ours", "open3d"):
        raise ValueError(f"depth_fuser must be 'ours' or 'open3d', got {depth_fuser!r}")
    if fuser_factory is None and run_fusion:
        if depth_fuser == "open3d":
            from .scalable_tsdf import Open3DFuser

            def fuser_factory(_scan):
                return Open3DFuser(fuse_color=fuse_color, device=device)
        else:
            from .tsdf import OurFuser

            def fuser_factory(_scan):
                return OurFuser(device=device)

    all_frame_metrics = metrics.ResultsAverager(name, "frame metrics")
    all_scene_metrics = metrics.ResultsAverager(name, "scene metrics")
    score_meshes = run_fusion and gt_mesh_factory is not None
    all_scene_mesh_metrics = metrics.ResultsAverager(name, "scene mesh metrics") if score_meshes else None
    with torch.inference_mode():
        start_time = torch.cuda.Event(enable_timing=True)
        end_time = torch.cuda.Event(enable_timing=True)
        for scan, frames in scans:
            fuser = fuser_factory(scan) if run_fusion else None
            scene_frame_metrics = metrics.ResultsAverager(name, f"scene {scan} metrics")
            if dump_depth_visualization:
                from .visualization import quick_viz_export
                viz_dir = os.path.join(output_dir, "viz", "quick_viz", scan)
                os.makedirs(viz_dir, exist_ok=True)
            for batch_ind, (cur_data, src_data) in enumerate(_batches(frames, batch_size)):
                cur_data, src_data = _to(cur_data, device), _to(src_data, device)
                depth_gt = cur_data["full_res_depth_b1hw"]
                B, size = depth_gt.shape[0], depth_gt.shape[-2:]

                start_time.record()
                outputs = model("test", cur_data, src_data, unbatched_matching_encoder_forward=True,
                                return_mask=True)
                end_time.record()
                torch.cuda.synchronize()
                elapsed_model_time = start_time.elapsed_time(end_time)

                # one device-to-host copy: the [B,12] metrics and the valid counts
                buf = metrics.score_block(depth_gt, outputs["depth_pred_s0_b1hw"], min_depth=MIN_DEPTH, mult_a=True)
                block, counts = metrics.split_block(buf.cpu(), B)
                for i in range(B):
                    if counts[i] == 0:   # no valid ground truth in this frame
                        continue
                    element_metrics = {k: block[i, j] for j, k in enumerate(metrics.METRIC_KEYS)}
                    element_metrics["model_time"] = elapsed_model_time / B
                    scene_frame_metrics.update_results(element_metrics)
                    all_frame_metrics.update_results(element_metrics)

                if run_fusion:
                    if fusion_use_raw_lowest_cost:
                        depth = _upsample_nearest(outputs["lowest_cost_bhw"], size)
                    else:
                        depth = _upsample_nearest(outputs["depth_pred_s0_b1hw"].squeeze(1), size)
                    if mask_pred_depth or fusion_use_raw_lowest_cost:
                        overall_mask = _upsample_nearest(outputs["overall_mask_bhw"], size).bool()
                        depth[~overall_mask] = -1
                    color = cur_data.get("high_res_color_b3hw", cur_data.get("image_b3hw"))
                    fuser.fuse_frames(depth, cur_data["K_full_depth_b44"], cur_data["cam_T_world_b44"], color)

                if dump_depth_visualization:
                    quick_viz_export(viz_dir, outputs, cur_data, batch_ind, depth_gt > MIN_DEPTH, batch_size)

            if run_fusion:
                mesh_dir = os.path.join(output_dir, "meshes",
                                        _mesh_folder(fuser, mask_pred_depth, fusion_use_raw_lowest_cost, fuse_color))
                os.makedirs(mesh_dir, exist_ok=True)
                mesh_path = os.path.join(mesh_dir, f"{scan.replace('/', '_')}.ply")
                fuser.export_mesh(mesh_path)
                gt_mesh = gt_mesh_factory(scan) if score_meshes else None
                if gt_mesh is not None:
                    from .mesh_metrics import mesh_metrics
                    scene_mesh_metrics = metrics.ResultsAverager(name, f"scene {scan} mesh metrics")
                    scene_mesh_metrics.update_results(mesh_metrics(mesh_path, gt_mesh, device=device))
                    scene_mesh_metrics.compute_final_average()
                    all_scene_mesh_metrics.update_results(scene_mesh_metrics.final_metrics)
                    print("\nScene mesh metrics:")
                    scene_mesh_metrics.print_sheets_friendly(include_metrics_names=True, print_running_metrics=False)
                    scene_mesh_metrics.output_json(
                        os.path.join(scores_dir, f"{scan.replace('/', '_')}_mesh_metrics.json"))

            scene_frame_metrics.compute_final_average()
            all_scene_metrics.update_results(scene_frame_metrics.final_metrics)
            print("\nScene metrics:")
            scene_frame_metrics.print_sheets_friendly(include_metrics_names=True)
            scene_frame_metrics.output_json(os.path.join(scores_dir, f"{scan.replace('/', '_')}_metrics.json"))
            print("\nRunning frame metrics:")
            all_frame_metrics.print_sheets_friendly(include_metrics_names=False, print_running_metrics=True)

        print("\nFinal metrics:")
        for averager, kind in ((all_scene_metrics, "scene"), (all_frame_metrics, "frame")):
            averager.compute_final_average()
            averager.pretty_print_results(print_running_metrics=False)
            averager.print_sheets_friendly(include_metrics_names=True, print_running_metrics=False)
            averager.output_json(os.path.join(scores_dir, f"all_{kind}_avg_metrics_{split}.json"))
            if kind == "scene":
                print("")
        if all_scene_mesh_metrics is not None and all_scene_mesh_metrics.elem_metrics_list:
            print("\nFinal mesh metrics:")
            all_scene_mesh_metrics.compute_final_average()
            all_scene_mesh_metrics.pretty_print_results(print_running_metrics=False)
            all_scene_mesh_metrics.output_json(os.path.join(scores_dir, f"all_scene_avg_mesh_metrics_{split}.json"))
    return all_frame_metrics, all_scene_metrics
