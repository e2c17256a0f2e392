"""TSDF fusion of predicted depth maps -- API-compatible with the reference's tools/tsdf.py (`TSDF`, `TSDFFuser`)
and tools/fusers_helper.py (`OurFuser`), the step right after the depth hot path in `test.py --run_fusion`
(SURVEY.md §8f "next" #2).

`TSDFFuser.integrate_depth` runs ONE hand-written HIP kernel per batch of depth maps (`sr_tsdf_integrate_fwd`,
csrc/sr_tsdf.hip): the fp16 volume is streamed once, every voxel applies the frames of the batch in order in
registers.  The reference instead materialises ~10 [B, N]-sized fp16 temporaries per call (N = voxels) and does a
masked gather / scatter per frame.  Results are bit-identical to the reference executed on CPU (tests/golden/tsdf_*).

Mesh export (`TSDF.extract_mesh` / `TSDF.save`, `OurFuser.export_mesh` / `get_mesh`) runs marching cubes on the GPU
(`sr_mesh_count` + `sr_mesh_emit`, csrc/sr_mesh.hip) and returns a `TriangleMesh`; the reference copies the volume to the
host and runs skimage + trimesh there (tools/tsdf.py:128-168).  The surface rules are in include/simplerecon_hip.h.

`TSDF.from_mesh` and `OurFuser(gt_path=...)` size the volume from a ground-truth mesh read by `ply.read_ply`.

The reference's other fuser, `depth_fuser="open3d"` (sparse, unbounded, with colour), is
`scalable_tsdf.Open3DFuser`.  Not provided: `to_mesh` (its contract is a trimesh.Trimesh).  There is no CPU fallback:
tensors must live on the GPU.
"""
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib, ply


class TriangleMesh:
    """An indexed triangle mesh: `vertices` [V,3] fp32, `faces` [F,3] int32 (counter-clockwise seen from the side of
    increasing TSDF, i.e. from free space), `normals` [V,3] fp32 unit vectors or None, `colors` [V,3] fp32 in [0, 1]
    or None."""

    def __init__(self, vertices: torch.Tensor, faces: torch.Tensor, normals: Optional[torch.Tensor] = None,
                 colors: Optional[torch.Tensor] = None):
        self.vertices = vertices
        self.faces = faces
        self.normals = normals
        self.colors = colors

    def cpu(self):
        return TriangleMesh(self.vertices.cpu(), self.faces.cpu(), None if self.normals is None else self.normals.cpu(),
                            None if self.colors is None else self.colors.cpu())

    def write_ply(self, path):
        """Binary little-endian PLY: `float x,y,z` (+ `nx,ny,nz`) (+ `uchar red,green,blue`, clamp(floor(c * 255 + 0.5))
        of the [0, 1] colours) per vertex and a `list uchar int vertex_indices` face element -- the layout trimesh
        writes."""
        def f32(t):
            return t.detach().cpu().numpy().astype("<f4", copy=False).reshape(-1, 3)
        columns = [(n, "<f4", f32(self.vertices)[:, i]) for i, n in enumerate("xyz")]
        if self.normals is not None:
            columns += [(n, "<f4", f32(self.normals)[:, i]) for i, n in enumerate(("nx", "ny", "nz"))]
        if self.colors is not None:
            c8 = np.clip(np.floor(f32(self.colors) * np.float32(255) + np.float32(0.5)), 0, 255).astype(np.uint8)
            columns += [(n, "u1", c8[:, i]) for i, n in enumerate(("red", "green", "blue"))]
        ply.write_ply(path, columns, self.faces.detach().cpu().numpy().astype("<i4", copy=False).reshape(-1, 3))


def marching_cubes(tsdf_values: torch.Tensor, level=0.0, origin=(0.0, 0.0, 0.0), scale=1.0,
                   compute_normals=True) -> TriangleMesh:
    """Marching cubes on an fp16 [X,Y,Z] device volume (sr_mesh_count + sr_mesh_emit; rules: include/simplerecon_hip.h,
    "mesh extraction").  Vertices are origin + voxel index * scale in fp32.  One host synchronisation (the totals)."""
    vals = tsdf_values
    if not isinstance(vals, torch.Tensor) or vals.dtype != torch.float16 or vals.dim() != 3:
        raise TypeError("tsdf_values must be an fp16 [X,Y,Z] tensor")
    if not vals.is_cuda:
        raise _lib.HipLibraryError("the TSDF volume lives on the host: call tsdf.cuda() (no CPU fallback)")
    X, Y, Z = vals.shape
    if min(X, Y, Z) < 2:
        raise ValueError(f"marching cubes needs every volume dimension >= 2, got {tuple(vals.shape)}")
    vals = vals.contiguous()
    dev = vals.device
    lib = _lib.lib()
    with _lib.on_device(dev):
        cbytes = lib.sr_mesh_count_scratch_bytes(X, Y, Z)
        cscratch = torch.empty(cbytes, dtype=torch.uint8, device=dev)
        totals = torch.empty(3, dtype=torch.int64, device=dev)
        _lib.call("sr_mesh_count", dev, vals, X, Y, Z, float(level), cscratch, cbytes, totals)
        active, nv, nf = (int(x) for x in totals.tolist())
        if nv >= 2 ** 31 or nf >= 2 ** 31:
            raise _lib.HipLibraryError(f"mesh of {nv} vertices / {nf} faces: int32 face indices cannot address it")
        lbytes = lib.sr_mesh_list_scratch_bytes(active)
        lscratch = torch.empty(max(lbytes, 1), dtype=torch.uint8, device=dev)
        verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
        normals = torch.empty((nv, 3), dtype=torch.float32, device=dev) if compute_normals else None
        faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
        ox, oy, oz = (float(o) for o in origin)
        _lib.call("sr_mesh_emit", dev, vals, X, Y, Z, float(level), ox, oy, oz, float(scale), cscratch, cbytes, lscratch,
                  lbytes, active, nv, nf, verts, normals, faces)
        # the scratch buffers go back to torch's caching allocator, which orders their reuse on this stream
    return TriangleMesh(verts, faces, normals)


class TSDF:
    """Housing for a TSDF volume (reference tools/tsdf.py:11-97).  `tsdf_values`, `tsdf_weights`: fp16 [X,Y,Z];
    `voxel_coords`: fp16 [3,X,Y,Z] world coordinates (materialised lazily -- the HIP kernel regenerates them from
    `origin` and `voxel_size` when the volume comes from `from_bounds`)."""
    VOX_MOD = 8  # volume dimensions are multiples of 8 (tsdf.py:16)

    def __init__(self, voxel_coords, tsdf_values, tsdf_weights, voxel_size, origin):
        self._voxel_coords = voxel_coords.half() if voxel_coords is not None else None
        self.tsdf_values = tsdf_values.half().contiguous()
        self.tsdf_weights = tsdf_weights.half().contiguous()
        self.voxel_size = voxel_size
        self.origin = origin.half()
        self._origin_f32 = None   # set by from_bounds: the fp32 origin the coordinates are generated from
        self._generated = False   # voxel coordinates follow origin + index * voxel_size exactly

    @classmethod
    def from_bounds(cls, bounds: dict, voxel_size: float, device="cuda"):
        """Creates a TSDF volume with bounds at a specific voxel size (tsdf.py:69-97): values -1, weights 0."""
        expected_keys = ['xmin', 'xmax', 'ymin', 'ymax', 'zmin', 'zmax']
        for key in expected_keys:
            if key not in bounds.keys():
                raise KeyError("Provided bounds dict need to have keys"
                               "'xmin', 'xmax', 'ymin', 'ymax', 'zmin', 'zmax'!")
        dims = tuple(int(np.ceil((bounds[a + 'max'] - bounds[a + 'min']) / voxel_size / cls.VOX_MOD)) * cls.VOX_MOD
                     for a in "xyz")
        origin = torch.FloatTensor([bounds['xmin'], bounds['ymin'], bounds['zmin']])
        values = -torch.ones(dims, dtype=torch.float16, device=device)
        weights = torch.zeros(dims, dtype=torch.float16, device=device)
        vol = cls(None, values, weights, voxel_size, origin)
        vol._origin_f32 = origin.clone()
        vol._generated = True
        return vol

    @classmethod
    def from_mesh(cls, mesh: TriangleMesh, voxel_size: float, device="cuda"):
        """A volume over the mesh's vertex bounds padded by 3 voxels on every side (tsdf.py:51-67): bounds computed in
        fp64 from the vertices, then from_bounds."""
        v = mesh.vertices.detach().cpu().double().numpy().reshape(-1, 3)
        if len(v) == 0:
            raise ValueError("TSDF.from_mesh: the mesh has no vertices")
        if not np.isfinite(v).all():
            raise ValueError("TSDF.from_mesh: the mesh has non-finite vertices")
        lo, hi = v.min(0), v.max(0)
        bounds = {}
        for i, a in enumerate("xyz"):
            bounds[a + "min"] = float(lo[i] - 3 * voxel_size)
            bounds[a + "max"] = float(hi[i] + 3 * voxel_size)
        return cls.from_bounds(bounds, voxel_size, device=device)

    @classmethod
    def generate_voxel_coords(cls, origin: torch.Tensor, volume_dims: Tuple[int, int, int], voxel_size: float):
        """World coordinates of every voxel, fp32 [3,X,Y,Z] (tsdf.py:99-111)."""
        grid = torch.meshgrid([torch.arange(vd, device=origin.device) for vd in volume_dims], indexing="ij")
        return origin.view(3, 1, 1, 1) + torch.stack(grid, 0) * voxel_size

    @property
    def voxel_coords(self):
        if self._voxel_coords is None:
            dev = self.tsdf_values.device
            self._voxel_coords = self.generate_voxel_coords(self._origin_f32.to(dev), tuple(self.tsdf_values.shape),
                                                            self.voxel_size).half()
        return self._voxel_coords

    def cuda(self):
        self.tsdf_values = self.tsdf_values.cuda()
        self.tsdf_weights = self.tsdf_weights.cuda()
        if self._voxel_coords is not None:
            self._voxel_coords = self._voxel_coords.cuda()

    def cpu(self):
        """Moves the volume to host memory (for export); `integrate_depth` needs it on the GPU again."""
        self.tsdf_values = self.tsdf_values.cpu()
        self.tsdf_weights = self.tsdf_weights.cpu()
        if self._voxel_coords is not None:
            self._voxel_coords = self._voxel_coords.cpu()

    def to_mesh(self, scale_to_world=True, export_single_mesh=False):
        raise NotImplementedError("to_mesh returns a trimesh.Trimesh in the reference (tsdf.py:128-156), which is not "
                                  "available here: use TSDF.extract_mesh (a TriangleMesh on the GPU) or TSDF.save (PLY)")

    def extract_mesh(self, level=0.0, scale_to_world=True, compute_normals=True) -> TriangleMesh:
        """Marching cubes on the GPU (the reference's to_mesh settings: level 0, values clamped to [-1, 1], no
        degenerate triangles).  scale_to_world: vertices in world coordinates, float(fp16 origin) + index * voxel_size
        (as the reference adds its fp16 origin, tsdf.py:147-148); else in voxel units."""
        if scale_to_world:
            origin, scale = [float(o) for o in self.origin.float()], float(self.voxel_size)
        else:
            origin, scale = (0.0, 0.0, 0.0), 1.0
        return marching_cubes(self.tsdf_values, level=level, origin=origin, scale=scale, compute_normals=compute_normals)

    def save(self, savepath, filename, save_mesh=True):
        """Saves the mesh as `filename` with .bin replaced by .ply under `savepath` (reference tsdf.py:158-168).  Like
        the reference, the volume is on the host afterwards; a volume already on the host is meshed from a copy on the
        current GPU."""
        mesh = None
        if save_mesh:
            if self.tsdf_values.is_cuda:
                mesh = self.extract_mesh()
            else:
                dev = torch.device("cuda", torch.cuda.current_device())
                copy = TSDF(None, self.tsdf_values.to(dev), self.tsdf_weights, self.voxel_size, self.origin)
                mesh = copy.extract_mesh()
        self.cpu()
        os.makedirs(savepath, exist_ok=True)
        if mesh is not None:
            mesh.write_ply(os.path.join(savepath, filename).replace(".bin", ".ply"))


class TSDFFuser:
    """Fuses depth maps into a TSDF volume (reference tools/tsdf.py:176-320)."""
    MAX_FRAMES_PER_CALL = 1024  # sr_tsdf_integrate_fwd refuses more; integrate_depth splits longer batches

    def __init__(self, tsdf, min_depth=0.5, max_depth=5.0, use_gpu=True):
        if not use_gpu:
            raise _lib.HipLibraryError("the HIP fuser has no CPU path (use_gpu=False)")
        self.tsdf = tsdf
        self.min_depth = min_depth
        self.max_depth = max_depth
        self.use_gpu = use_gpu
        self.truncation_size = 3.0
        self.maxW = 100.0

    @property
    def voxel_coords(self):
        return self.tsdf.voxel_coords

    @property
    def tsdf_values(self):
        return self.tsdf.tsdf_values

    @property
    def tsdf_weights(self):
        return self.tsdf.tsdf_weights

    @property
    def voxel_size(self):
        return self.tsdf.voxel_size

    @property
    def shape(self):
        return self.tsdf.tsdf_values.shape

    @property
    def truncation(self):
        return self.truncation_size * self.voxel_size

    def integrate_depth(self, depth_b1hw, cam_T_world_T_b44, K_b44, depth_mask_b1hw=None):
        """Integrates depth maps into the volume, frame after frame (tsdf.py:238-320).

        depth_b1hw: fp16 depth maps; cam_T_world_T_b44: fp16 extrinsics (not poses!); K_b44: fp16 intrinsics;
        depth_mask_b1hw: optional boolean mask of valid depth pixels.  The reference's arithmetic is fp16 throughout
        (its voxel coordinates are fp16, so fp32 inputs fail in its matmul); fp32 inputs are refused here as well."""
        vol = self.tsdf
        for name, t in (("depth_b1hw", depth_b1hw), ("cam_T_world_T_b44", cam_T_world_T_b44), ("K_b44", K_b44)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} must be a torch.Tensor")
            if t.dtype != torch.float16:
                raise TypeError(f"{name} must be float16 (the reference fuses in fp16: pass .half()), got {t.dtype}")
        dev = vol.tsdf_values.device
        if dev.type != "cuda":
            raise _lib.HipLibraryError("the TSDF volume lives on the host: call tsdf.cuda() (no CPU fallback)")
        if depth_b1hw.dim() != 4 or depth_b1hw.shape[1] != 1:
            raise ValueError(f"depth_b1hw must be [B,1,H,W], got {tuple(depth_b1hw.shape)}")
        b, _, h, w = depth_b1hw.shape
        if tuple(cam_T_world_T_b44.shape) != (b, 4, 4) or tuple(K_b44.shape) != (b, 4, 4):
            raise ValueError("cam_T_world_T_b44 and K_b44 must be [B,4,4]")
        depth = depth_b1hw.to(dev).contiguous()   # the reference moves its inputs to the GPU as well (:257-260)
        T = cam_T_world_T_b44.to(dev).contiguous()
        K = K_b44.to(dev).contiguous()
        mask = None
        if depth_mask_b1hw is not None:
            if depth_mask_b1hw.dtype != torch.bool or tuple(depth_mask_b1hw.shape) != tuple(depth_b1hw.shape):
                raise ValueError("depth_mask_b1hw must be a boolean tensor shaped like depth_b1hw")
            mask = depth_mask_b1hw.to(dev).contiguous()
        X, Y, Z = vol.tsdf_values.shape
        if not (vol.tsdf_values.is_contiguous() and vol.tsdf_weights.is_contiguous()):
            raise ValueError("tsdf_values / tsdf_weights must be contiguous")
        if vol._generated:
            coords, o = None, vol._origin_f32
            ox, oy, oz = float(o[0]), float(o[1]), float(o[2])
        else:
            coords = vol.voxel_coords.to(dev).contiguous()
            ox = oy = oz = 0.0
        if b == 0:
            return
        # one launch takes at most MAX_FRAMES_PER_CALL frames (its per-frame state lives in LDS); the update is sequential
        # per voxel, so consecutive calls over consecutive frames give exactly the result of one long batch
        for b0 in range(0, b, self.MAX_FRAMES_PER_CALL):
            b1 = min(b0 + self.MAX_FRAMES_PER_CALL, b)
            _lib.call("sr_tsdf_integrate_fwd", dev, vol.tsdf_values, vol.tsdf_weights, coords, X, Y, Z, ox, oy, oz,
                      float(vol.voxel_size), depth[b0:b1], None if mask is None else mask[b0:b1], K[b0:b1], T[b0:b1],
                      b1 - b0, h, w, float(self.min_depth), float(self.max_depth),
                      float(self.max_depth - self.min_depth), float(self.truncation), float(self.maxW))


class OurFuser:
    """The fuser behind `--depth_fuser ours` (reference tools/fusers_helper.py:25-83): a dense TSDF over the bounds of
    the ground-truth mesh at `gt_path` (a PLY file, padded by 3 voxels: TSDF.from_mesh), else over the given bounds
    (default: the reference's +-10 m cube)."""

    def __init__(self, gt_path=None, fusion_resolution=0.04, max_fusion_depth=3, fuse_color=False, bounds=None,
                 device="cuda"):
        self.fusion_resolution = fusion_resolution
        self.max_fusion_depth = max_fusion_depth
        if gt_path:
            from .ply import read_ply
            gt_mesh = read_ply(gt_path)
            if not isinstance(gt_mesh, TriangleMesh):
                raise ValueError(f"{gt_path} holds a point cloud, not a mesh")
            tsdf_pred = TSDF.from_mesh(gt_mesh, voxel_size=fusion_resolution, device=device)
        else:
            if bounds is None:
                bounds = dict(xmin=-10.0, xmax=10.0, ymin=-10.0, ymax=10.0, zmin=-10.0, zmax=10.0)
            tsdf_pred = TSDF.from_bounds(bounds, voxel_size=fusion_resolution, device=device)
        self.tsdf_fuser_pred = TSDFFuser(tsdf_pred, max_depth=max_fusion_depth)

    def fuse_frames(self, depths_b1hw, K_b44, cam_T_world_b44, color_b3hw=None):
        self.tsdf_fuser_pred.integrate_depth(depth_b1hw=depths_b1hw.half(), cam_T_world_T_b44=cam_T_world_b44.half(),
                                             K_b44=K_b44.half())

    def get_mesh(self, export_single_mesh=True, convert_to_trimesh=True) -> TriangleMesh:
        """The fused surface as a `TriangleMesh` on the GPU (not a trimesh object: trimesh is not a dependency).  The
        output is always one mesh, so `export_single_mesh` changes nothing; `convert_to_trimesh` is accepted for the
        reference's signature (fusers_helper.py:79-81) and ignored."""
        return self.tsdf_fuser_pred.tsdf.extract_mesh()

    def export_mesh(self, path, export_single_mesh=True):
        """Writes the fused surface to `path` as binary PLY (reference fusers_helper.py:72-77, which lets trimesh pick
        the format from the extension: only .ply is written here).  `export_single_mesh` changes nothing."""
        if not str(path).lower().endswith(".ply"):
            raise ValueError(f"export_mesh writes PLY only, got {path!r}")
        self.get_mesh(export_single_mesh=export_single_mesh).write_ply(path)
