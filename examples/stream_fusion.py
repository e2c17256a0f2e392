"""End-to-end streaming example on synthetic data: posed frames -> online keyframe / source selection
(simplerecon_amd.keyframes) -> DepthModel.forward (image-prior + matching encoders, plane-sweep cost volume, cost-volume
encoder and UNet++ decoder, all on HIP kernels) -> TSDF fusion of the predicted depth (simplerecon_amd.tsdf; with
--fuser open3d the sparse, unbounded colour volume of simplerecon_amd.scalable_tsdf, --color for vertex colours) -> with
--mesh, marching cubes on the GPU and a PLY file; with --point-cloud, multi-view consistency fusion of the same depth maps
into a coloured point cloud (simplerecon_amd.point_cloud, the reference's pc_fusion.py); with --viz DIR, the colour-mapped
predicted depth and the normal map of every keyframe as PNGs (simplerecon_amd.visualization); with --render FILE, a shaded
picture of the fused mesh from the last keyframe's camera (simplerecon_amd.render.render_color).  It mirrors what the reference's test.py does per scan
(test.py:210-410) without datasets or checkpoints.

    python examples/stream_fusion.py [--frames 120] [--height 192] [--width 256] [--mesh out.ply] [--point-cloud out.ply]
                                     [--fuser {ours,open3d}] [--color] [--viz DIR] [--render out.png]

Weights are random, so the depth maps are meaningless -- the point is the data flow and the API.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplerecon_amd import depth_model as dm  # noqa: E402
from simplerecon_amd import keyframes as kf  # noqa: E402
from simplerecon_amd import synthetic  # noqa: E402
from simplerecon_amd.point_cloud import PointCloudFuser  # noqa: E402
from simplerecon_amd.scalable_tsdf import Open3DFuser  # noqa: E402
from simplerecon_amd.tsdf import OurFuser  # noqa: E402


def intrinsics(width, height, scale):
    """ScanNet-like pinhole intrinsics at 1 / 2**scale of the image resolution."""
    K = torch.eye(4)
    K[0, 0] = K[1, 1] = 577.87 * width / 640.0
    K[0, 2], K[1, 2] = width / 2.0, height / 2.0
    K[:2] /= 2 ** scale
    return K


def camera_path(n, seed=0):
    """Slow forward / sideways motion with a little rotation: camera-to-world poses."""
    rng = np.random.default_rng(seed)
    T, out = np.eye(4), []
    for _ in range(n):
        a = 0.01 + 0.004 * rng.standard_normal()
        step = np.eye(4)
        step[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        step[:3, 3] = [0.02, 0.002 * rng.standard_normal(), 0.015]
        T = T @ step
        out.append(T.copy())
    return out


def run(frames=120, height=192, width=256, views=8, device="cuda:0", verbose=True, mesh_path=None,
        point_cloud_path=None, fuser_name="ours", color=False, viz_dir=None, render_path=None):
    opts = dm.default_options(image_width=width, image_height=height, model_num_views=views)
    model = dm.DepthModel(opts)
    for i, m in enumerate((model.encoder, model.matching_model, model.cost_volume_net, model.depth_decoder,
                           model.cost_volume.mlp)):
        synthetic.seeded_fill_(m, seed=20 + i)
    model = model.to(device).eval()
    if fuser_name == "open3d":   # sparse: grows where the depth lands, no bounds needed
        fuser = Open3DFuser(max_fusion_depth=3.0, fuse_color=color, device=device)
    else:
        fuser = OurFuser(bounds=dict(xmin=-2.0, xmax=6.0, ymin=-2.0, ymax=2.0, zmin=-1.0, zmax=7.0),
                         max_fusion_depth=3.0, fuse_color=color, device=device)
    pc_fuser = PointCloudFuser(fusion_size=(height, width)) if point_cloud_path else None   # pc_fusion.py:122-150
    cfg = kf.DVMVS_Config
    buf = kf.KeyframeBuffer(cfg.test_keyframe_buffer_size, cfg.test_keyframe_pose_distance, cfg.test_optimal_t_measure,
                            cfg.test_optimal_R_measure, store_return_indices=True)
    K1 = intrinsics(width, height, 1)          # matching resolution = image / 4 -> "s1" of the reference's pyramid
    K_depth = intrinsics(width, height, 1)     # the s0 prediction comes out at image / 2
    invK1 = torch.linalg.inv(K1)
    if viz_dir:
        from PIL import Image
        from simplerecon_amd import visualization as viz
        os.makedirs(viz_dir, exist_ok=True)
    g = torch.Generator(device="cpu").manual_seed(0)
    predicted, last_cam_T_world = 0, None
    for i, world_T_cam in enumerate(camera_path(frames)):
        image = torch.randn((3, height, width), generator=g)
        if buf.try_new_keyframe(world_T_cam, image, index=i) != kf.KeyframeBuffer.ADDED:
            continue
        sources = buf.get_best_measurement_frames(views - 1)
        if len(sources) < views - 1:
            continue                              # the reference only predicts with a full tuple
        order = kf.sort_sources_by_pose_penalty(np.linalg.inv(world_T_cam).astype(np.float32),
                                                np.stack([s[0] for s in sources]).astype(np.float32))
        sources = [sources[j] for j in order]
        f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32)
        cur = {"image_b3hw": image[None].to(device), "invK_s1_b44": invK1[None].to(device),
               "cam_T_world_b44": f32(np.linalg.inv(world_T_cam))[None].to(device),
               "world_T_cam_b44": f32(world_T_cam)[None].to(device)}
        src = {"image_b3hw": torch.stack([s[1] for s in sources])[None].to(device),
               "K_s1_b44": K1[None, None].repeat(1, views - 1, 1, 1).to(device),
               "cam_T_world_b44": f32(np.stack([np.linalg.inv(s[0]) for s in sources]))[None].to(device),
               "world_T_cam_b44": f32(np.stack([s[0] for s in sources]))[None].to(device)}
        with torch.inference_mode():
            out = model("test", cur, src, unbatched_matching_encoder_forward=False, return_mask=True)
            depth = out["depth_pred_s0_b1hw"]
            fuser.fuse_frames(depth, K_depth[None].to(device), cur["cam_T_world_b44"], cur["image_b3hw"])
            if pc_fuser is not None:
                pc_fuser.fuse_frames(depth, K_depth[None].to(device), cur["cam_T_world_b44"], cur["image_b3hw"])
            if viz_dir:   # both pictures are made on the device; 8-bit pixels come to the host
                normals = model.compute_normals(depth, torch.linalg.inv(K_depth)[None].to(device))
                for name, picture in (("pred_depth", viz.colormap_u8(depth)), ("normals", viz.normals_u8(normals))):
                    Image.fromarray(picture[0].cpu().numpy()).save(os.path.join(viz_dir, f"{i:06d}_{name}.png"))
        predicted += 1
        last_cam_T_world = cur["cam_T_world_b44"]
    if fuser_name == "open3d":
        vol = fuser.volume
        touched = int((vol.weights > 0).sum())
        shape = f"{vol.num_blocks} blocks of 16^3"
    else:
        vol = fuser.tsdf_fuser_pred
        touched = int((vol.tsdf_weights > 0).sum())
        shape = str(tuple(vol.shape))
    if verbose:
        print(f"{frames} frames -> {predicted} keyframes predicted and fused; TSDF {shape}: {touched} voxels touched")
    if mesh_path:
        fuser.export_mesh(mesh_path)   # test.py:405-410
        if verbose:
            mesh = fuser.get_mesh()
            print(f"mesh: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} triangles -> {mesh_path}")
    if point_cloud_path and predicted:
        pc_fuser.export_point_cloud(point_cloud_path)   # pc_fusion.py:152-172
        if verbose:
            print(f"point cloud: {len(pc_fuser.get_point_cloud())} points -> {point_cloud_path}")
    if render_path and predicted:   # shaded on the device; the 8-bit picture comes to the host for PNG encoding
        from PIL import Image
        from simplerecon_amd.render import render_color
        picture = render_color(fuser.get_mesh(), intrinsics(width, height, 0)[None].to(device), last_cam_T_world, height,
                               width, output="u8")
        Image.fromarray(picture[0].cpu().numpy()).save(render_path)
        if verbose:
            print(f"render: {width} x {height} -> {render_path}")
    return predicted, touched


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--mesh", default=None, help="write the fused surface to this .ply file")
    ap.add_argument("--point-cloud", default=None, help="write the fused point cloud to this .ply file")
    ap.add_argument("--fuser", choices=["ours", "open3d"], default="ours",
                    help="ours: dense TSDF over fixed bounds; open3d: sparse colour TSDF, unbounded")
    ap.add_argument("--color", action="store_true", help="fuse vertex colours (the open3d fuser; ours ignores it)")
    ap.add_argument("--viz", default=None, metavar="DIR",
                    help="write each keyframe's colour-mapped predicted depth and normal map as PNGs into DIR")
    ap.add_argument("--render", default=None, metavar="FILE",
                    help="write a shaded picture of the fused mesh, seen from the last keyframe's camera, to this .png file")
    a = ap.parse_args()
    run(a.frames, a.height, a.width, mesh_path=a.mesh, point_cloud_path=a.point_cloud, fuser_name=a.fuser,
        color=a.color, viz_dir=a.viz, render_path=a.render)
