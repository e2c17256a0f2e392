"""Point-cloud fusion of predicted depth maps (the reference's pc_fusion.py with tools/torch_point_cloud_fusion.py,
then open3d's voxel_down_sample and PLY writer) on HIP kernels: csrc/sr_pcfusion.hip.  The rules are stated in
include/simplerecon_hip.h, section "point-cloud fusion".

    fuse_scene(depths, images, cam_T_world, K)     -> (PointCloud, valid [N,h,w])   device tensors
    process_scene / process_depth                  the reference's functions: same signatures, numpy results
    PointCloudFuser                                pc_fusion.py's per-batch steps, fusion, downsampling and export

There is no CPU path: without a GPU every entry point raises HipLibraryError."""
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, ply

SCRATCH_BYTES = 1 << 30   # per-chunk output of the consistency kernel (points + counts), about 1 GB by default
_FRAME_BYTES_PER_PIXEL = 16


class PointCloud:
    """`points` [M,3] fp32 and `colors` [M,3] uint8 (or None), on the device they were made on."""

    def __init__(self, points: torch.Tensor, colors: Optional[torch.Tensor] = None):
        if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
            raise TypeError(f"points must be an fp32 [M,3] tensor, got {points.dtype} {tuple(points.shape)}")
        if colors is not None and (colors.shape != points.shape or colors.dtype != torch.uint8):
            raise TypeError(f"colors must be a uint8 [M,3] tensor, got {colors.dtype} {tuple(colors.shape)}")
        self.points = points
        self.colors = colors

    def __len__(self):
        return int(self.points.shape[0])

    def cpu(self):
        return PointCloud(self.points.cpu(), None if self.colors is None else self.colors.cpu())

    def voxel_down_sample(self, voxel_size) -> "PointCloud":
        """open3d's PointCloud.voxel_down_sample: one point per occupied voxel, the fp64 mean of its points; colours
        are the integer mean of the voxel's uint8 colours, rounded half up.  Voxels come out in ascending key order."""
        vs = float(voxel_size)
        if not (vs > 0.0 and np.isfinite(vs)):
            raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
        pts = self.points
        if not pts.is_cuda:
            raise _lib.HipLibraryError("the point cloud lives on the host: voxel_down_sample runs on the GPU only")
        M = len(self)
        if M == 0:
            return PointCloud(pts.clone(), None if self.colors is None else self.colors.clone())
        pts = pts.contiguous()
        cols = None if self.colors is None else self.colors.contiguous()
        dev = pts.device
        with _lib.on_device(dev):
            p64 = pts.double()
            ext = torch.stack([p64.amin(0), p64.amax(0)]).cpu().numpy()
            if not np.isfinite(ext).all():
                raise ValueError("voxel_down_sample: the point cloud has non-finite coordinates")
            min_bound = ext[0] - vs * 0.5
            extent = np.floor((ext[1] - min_bound) / vs)
            if (extent >= 2 ** 21).any():
                raise ValueError(f"voxel_down_sample: {extent.astype(np.int64).tolist()} voxels per axis; keys hold "
                                 f"fewer than 2^21 per axis (use a larger voxel_size)")
            keys = torch.empty(M, dtype=torch.int64, device=dev)
            _lib.call("sr_pc_voxel_keys", dev, pts, M, *min_bound, vs, keys)
            skeys, order = torch.sort(keys, stable=True)
            _, counts = torch.unique_consecutive(skeys, return_counts=True)
            S = int(counts.shape[0])
            seg = torch.zeros(S + 1, dtype=torch.int64, device=dev)
            torch.cumsum(counts, 0, out=seg[1:])
            out_pts = torch.empty((S, 3), dtype=torch.float32, device=dev)
            out_cols = None if cols is None else torch.empty((S, 3), dtype=torch.uint8, device=dev)
            _lib.call("sr_pc_voxel_mean", dev, pts, cols, M, order, seg, S, out_pts, out_cols)
        return PointCloud(out_pts, out_cols)

    def write_ply(self, path):
        """Binary little-endian PLY: `float x,y,z` and, with colours, `uchar red,green,blue` per vertex."""
        v = self.points.detach().cpu().numpy().astype("<f4", copy=False).reshape(-1, 3)
        columns = [(n, "<f4", v[:, i]) for i, n in enumerate("xyz")]
        if self.colors is not None:
            c = self.colors.detach().cpu().numpy().reshape(-1, 3)
            columns += [(n, "u1", c[:, i]) for i, n in enumerate(("red", "green", "blue"))]
        ply.write_ply(path, columns)


def frame_constants(cam_T_world, K):
    """[N, SR_PC_FRAME_FLOATS] fp32 per-frame constants of sr_pc_consistency, computed in fp64 (layout: the header)."""
    P = torch.as_tensor(cam_T_world).detach().to("cpu", torch.float64)
    Kd = torch.as_tensor(K).detach().to("cpu", torch.float64)[:, :3, :3]
    R, t = P[:, :3, :3], P[:, :3, 3:]
    Kinv = torch.linalg.inv(Kd)
    Pinv = torch.linalg.inv(P)
    proj = Kd @ torch.cat([R, t], 2)                                   # K [R | t]
    back = R.transpose(1, 2) @ Kinv                                    # R^T K^-1
    back_t = -(R.transpose(1, 2) @ t)                                  # -R^T t
    ref = Pinv[:, :3, :3] @ Kinv                                       # P^-1[:3,:3] K^-1
    ref_t = Pinv[:, :3, 3:]
    c = torch.cat([proj.reshape(-1, 12), back.reshape(-1, 9), back_t.reshape(-1, 3), ref.reshape(-1, 9),
                   ref_t.reshape(-1, 3)], 1)
    if not torch.isfinite(c).all():
        raise ValueError("point-cloud fusion: singular or non-finite poses / intrinsics")
    return c.float()


def _device_of(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not _lib.cuda_available():
        raise _lib.HipLibraryError("point-cloud fusion runs on the GPU only and no GPU is visible (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _fuse(depths, images, cam_T_world, K, z_thresh, n_consistent_thresh, ref_begin=0, ref_count=None,
          scratch_bytes=SCRATCH_BYTES, chunk_frames=None):
    """Kept points [M,3] fp32, their colours (the images' dtype; None without images) and the keep masks of the
    reference frames [ref_begin, ref_begin + ref_count).  `chunk_frames` (default: as many as scratch_bytes holds)
    sets how many reference frames one launch covers."""
    if not isinstance(depths, torch.Tensor) or depths.dim() != 3:
        raise ValueError("depths must be an [N,h,w] tensor")
    N, h, w = (int(s) for s in depths.shape)
    if N < 1 or h < 2 or w < 2:
        raise ValueError(f"point-cloud fusion needs N >= 1 frames of at least 2 x 2 pixels, got {tuple(depths.shape)}")
    if tuple(cam_T_world.shape) != (N, 4, 4):
        raise ValueError(f"cam_T_world must be [N,4,4] = [{N},4,4], got {tuple(cam_T_world.shape)}")
    if K.dim() != 3 or K.shape[0] != N or tuple(K.shape[1:]) not in ((3, 3), (4, 4)):
        raise ValueError(f"K must be [N,3,3] or [N,4,4] with N = {N}, got {tuple(K.shape)}")
    if images is not None and tuple(images.shape) != (N, h, w, 3):
        raise ValueError(f"images must be [N,h,w,3] = [{N},{h},{w},3], got {tuple(images.shape)}")
    zt = float(z_thresh)
    if not (zt > 0 and np.isfinite(zt)):
        raise ValueError(f"z_thresh must be positive and finite, got {z_thresh}")
    ref_count = N - ref_begin if ref_count is None else ref_count
    if ref_count < 1 or ref_begin < 0 or ref_begin + ref_count > N:
        raise ValueError(f"bad reference range [{ref_begin}, {ref_begin + ref_count}) of {N} frames")
    dev = _device_of(depths, images, cam_T_world, K)
    consts = frame_constants(cam_T_world, K).to(dev)
    D = depths.detach().to(dev, torch.float32).contiguous()
    imgs = None if images is None else images.detach().to(dev)
    per_frame = h * w * _FRAME_BYTES_PER_PIXEL
    chunk = chunk_frames or max(1, min(ref_count, int(scratch_bytes) // per_frame))
    chunk = max(1, min(chunk, (2 ** 31 - 1) // (h * w * 12)))
    pts_out, rgb_out, valid_out = [], [], []
    with _lib.on_device(dev):
        for b in range(ref_begin, ref_begin + ref_count, chunk):
            c = min(chunk, ref_begin + ref_count - b)
            points = torch.empty((c, h, w, 3), dtype=torch.float32, device=dev)
            counts = torch.empty((c, h, w), dtype=torch.int32, device=dev)
            _lib.call("sr_pc_consistency", dev, D, consts, N, h, w, b, c, zt, points, counts)
            keep = counts >= int(n_consistent_thresh)
            pts_out.append(points[keep])
            if imgs is not None:
                rgb_out.append(imgs[b:b + c][keep])
            valid_out.append(keep)
    pts = torch.cat(pts_out, 0)
    rgb = torch.cat(rgb_out, 0) if imgs is not None else None
    return pts, rgb, torch.cat(valid_out, 0)


def fuse_scene(depths, images, cam_T_world, K, z_thresh=0.04, n_consistent_thresh=3, scratch_bytes=SCRATCH_BYTES):
    """Fuses every frame of a scene against all others: depths [N,h,w], images [N,h,w,3] uint8 or None, cam_T_world
    [N,4,4], K [N,3,3] (or [N,4,4]).  Returns (PointCloud, valid [N,h,w] bool), on the GPU.  Reference frames are
    processed in chunks whose outputs fit `scratch_bytes`."""
    if images is not None and images.dtype != torch.uint8:
        raise TypeError(f"images must be uint8, got {images.dtype}")
    pts, rgb, valid = _fuse(depths, images, cam_T_world, K, z_thresh, n_consistent_thresh, scratch_bytes=scratch_bytes)
    return PointCloud(pts, rgb), valid


def process_depth(ref_depth, ref_image, src_depths, src_images, ref_P, src_Ps, ref_K, src_Ks, z_thresh=0.1,
                  n_consistent_thresh=3):
    """tools/torch_point_cloud_fusion.process_depth: the reference frame against the given sources, in their order.
    Returns numpy (points [M,3] fp32, colours [M,3], valid [h,w] bool)."""
    dev = _device_of(ref_depth, src_depths, ref_P, src_Ps)
    depths = torch.cat([ref_depth.to(dev)[None], src_depths.to(dev)], 0)
    images = torch.cat([ref_image.to(dev)[None], src_images.to(dev)], 0) if ref_image is not None else None
    P = torch.cat([ref_P.to(dev)[None], src_Ps.to(dev)], 0)
    K = torch.cat([ref_K.to(dev)[None, :3, :3], src_Ks.to(dev)[:, :3, :3]], 0)
    pts, rgb, valid = _fuse(depths, images, P, K, z_thresh, n_consistent_thresh, ref_begin=0, ref_count=1)
    return pts.cpu().numpy(), (rgb.cpu().numpy() if rgb is not None else None), valid[0].cpu().numpy()


def process_scene(depth_preds, images, poses, K, z_thresh, n_consistent_thresh):
    """tools/torch_point_cloud_fusion.process_scene: every frame against all others.  Returns numpy (fused_pts [M,3]
    fp32, fused_rgb [M,3], all_valid [N,h,w] bool)."""
    pts, rgb, valid = _fuse(depth_preds, images, poses, K, z_thresh, n_consistent_thresh)
    return pts.cpu().numpy(), (rgb.cpu().numpy() if rgb is not None else None), valid.cpu().numpy()


_IMAGENET_MEAN = (0.485, 0.456, 0.406)
_IMAGENET_STD = (0.229, 0.224, 0.225)


class PointCloudFuser:
    """pc_fusion.py's fusion of a scan (pc_fusion.py:122-172): fuse_frames takes each batch of predictions, then
    get_point_cloud fuses all frames and downsamples, and export_point_cloud writes a .ply."""

    def __init__(self, z_thresh=0.04, n_consistent_thresh=3, voxel_downsample=0.02, max_fusion_depth=3.0,
                 fusion_size=(480, 640)):
        self.z_thresh = z_thresh
        self.n_consistent_thresh = n_consistent_thresh
        self.voxel_downsample = voxel_downsample
        self.max_fusion_depth = max_fusion_depth
        self.fusion_size = tuple(int(s) for s in fusion_size)
        self.depths, self.poses, self.Ks, self.images = [], [], [], []

    def fuse_frames(self, depths_b1hw, K_b44, cam_T_world_b44, color_b3hw=None):
        if depths_b1hw.dim() != 4 or depths_b1hw.shape[1] != 1:
            raise ValueError(f"depths must be [B,1,h,w], got {tuple(depths_b1hw.shape)}")
        B, _, h, w = depths_b1hw.shape
        if tuple(K_b44.shape) != (B, 4, 4) or tuple(cam_T_world_b44.shape) != (B, 4, 4):
            raise ValueError("K_b44 and cam_T_world_b44 must be [B,4,4]")
        if (self.images or self.depths) and (color_b3hw is None) != (not self.images):
            raise ValueError("colour must be given for every batch or for none")
        H, W = self.fusion_size
        depth = depths_b1hw.detach().float().clone()
        depth[depth > self.max_fusion_depth] = 0
        depth = F.interpolate(depth, size=(H, W), mode="nearest")
        K = K_b44.detach().float().clone()
        K[:, 0] *= W / w
        K[:, 1] *= H / h
        self.depths.append(depth[:, 0])
        self.Ks.append(K[:, :3, :3])
        self.poses.append(cam_T_world_b44.detach().float().clone())
        if color_b3hw is not None:
            if color_b3hw.dim() != 4 or color_b3hw.shape[:2] != (B, 3):
                raise ValueError(f"color_b3hw must be [B,3,h,w], got {tuple(color_b3hw.shape)}")
            img = F.interpolate(color_b3hw.detach().float(), size=(H, W), mode="bilinear")
            mean = torch.tensor(_IMAGENET_MEAN, device=img.device).view(1, 3, 1, 1)
            std = torch.tensor(_IMAGENET_STD, device=img.device).view(1, 3, 1, 1)
            img = (img * std + mean).permute(0, 2, 3, 1) * 255
            self.images.append(img.clamp(0, 255).to(torch.uint8))

    def get_point_cloud(self) -> PointCloud:
        if not self.depths:
            raise ValueError("no frames fused")
        depths = torch.cat(self.depths, 0)
        images = torch.cat(self.images, 0) if self.images else None
        pc, _ = fuse_scene(depths, images, torch.cat(self.poses, 0), torch.cat(self.Ks, 0), self.z_thresh,
                           self.n_consistent_thresh)
        return pc.voxel_down_sample(self.voxel_downsample)

    def export_point_cloud(self, filepath):
        if not str(filepath).endswith(".ply"):
            raise ValueError(f"point clouds are written as .ply only, got {filepath}")
        self.get_point_cloud().write_ply(filepath)
