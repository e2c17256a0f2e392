"""Sparse colour TSDF fusion -- the reference's second depth fuser, `--depth_fuser open3d` (tools/fusers_helper.py,
`Open3DFuser`, on Open3D's legacy `ScalableTSDFVolume` with RGB8 colour), on HIP kernels (csrc/sr_sparse_tsdf.hip).

The volume is unbounded: blocks of 16^3 voxels are allocated where the depth maps land, so no ground-truth mesh or
bounds are needed, and it is the reference's only fuser that keeps colour.  The rules (touch, integration, extraction)
are stated in include/simplerecon_hip.h, section "sparse TSDF"; they restate Open3D's algorithm from memory of it, so bit
parity with Open3D itself is unpinned.  tests/sparse_tsdf_oracle.py restates them in numpy.

State on the GPU: a sorted int64 table of block keys, a parallel table of pool slots and a voxel pool [capacity, 5,
4096] fp32 (tsdf, weight, red, green, blue) that doubles when it runs out.  `integrate` per batch of up to 64 frames:
the touch kernel writes candidate block keys, torch.unique groups them, a kernel ORs each frame's bit into its block's
uint64 mask, torch merges the new keys into the sorted table, and one integrate kernel updates every touched block once.
It synchronises with the host three times: to invert the poses in fp64, to size torch.unique's output and to read the
number of new blocks.  `extract_mesh` reads the vertex and face totals once.

    vol = ScalableTSDFVolume(voxel_length=0.04, sdf_trunc=0.12, max_depth=3.0)
    vol.integrate(depth_b1hw, K_b44, cam_T_world_b44, color_b3hw_uint8)   # device tensors
    mesh = vol.extract_mesh()                                             # TriangleMesh with colors

There is no CPU fallback: inputs must live on the GPU."""

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .tsdf import TriangleMesh

BLOCK = 16
VOXELS = BLOCK ** 3
MAX_FRAMES = 64                    # frames per kernel call: the per-block touch mask is a uint64
KEY_NONE = -1                      # SR_STSDF_KEY_NONE: an empty candidate
KEY_OFFSET = 1 << 20               # block coordinates lie in [-2^20, 2^20)
GREY = 178                         # uint8(0.7 * 255): the colour of every pixel without fuse_color
_FRAME_FLOATS = 16

# reference utils/generic_utils.py reverse_imagenet_normalize: TF.normalize with these mean / std
_REV_MEAN = (-2.11790393, -2.03571429, -1.80444444)
_REV_STD = (4.36681223, 4.46428571, 4.44444444)


def pack_keys(coords):
    """Block coordinates [n,3] (integers in [-2^20, 2^20)) -> int64 keys, x-major: ascending keys are (x, y, z)
    lexicographic order."""
    b = np.asarray(coords, dtype=np.int64).reshape(-1, 3) + KEY_OFFSET
    if (b < 0).any() or (b >= 2 * KEY_OFFSET).any():
        raise ValueError("block coordinates must lie in [-2^20, 2^20)")
    return (b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]


def unpack_keys(keys):
    """int64 keys -> block coordinates [n,3] int64."""
    k = np.asarray(keys, dtype=np.int64).reshape(-1)
    m = (1 << 21) - 1
    return np.stack([(k >> 42) & m, (k >> 21) & m, k & m], 1) - KEY_OFFSET


def reverse_imagenet_normalize(image):
    """Undoes ImageNet normalisation (the reference's utils/generic_utils.py helper): (x - mean) / std per channel with
    the reference's inverted constants, in the image's dtype."""
    mean = torch.tensor(_REV_MEAN, dtype=image.dtype, device=image.device).view(-1, 1, 1)
    std = torch.tensor(_REV_STD, dtype=image.dtype, device=image.device).view(-1, 1, 1)
    return image.sub(mean).div(std)


def _require_cuda(name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise _lib.HipLibraryError(f"{name} lives on {t.device}: the sparse TSDF needs device tensors (no CPU fallback)")


class ScalableTSDFVolume:
    """A sparse TSDF with colour on 16^3-voxel blocks (Open3D's ScalableTSDFVolume, legacy integrate /
    extract_triangle_mesh; rules: include/simplerecon_hip.h, "sparse TSDF").

    `keys`, `tsdf`, `weights`, `colors` are copies in ascending key order: [N] int64, [N,16,16,16] fp32 (twice) and
    [N,3,16,16,16] fp32 in 0..255; voxel (i, j, k) of block b is the global voxel 16 b + (i, j, k), centred at
    (g + 0.5) * voxel_length."""

    def __init__(self, voxel_length, sdf_trunc, max_depth, device="cuda", initial_capacity=256):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.HipLibraryError(f"the sparse TSDF lives on the GPU, got device {device!r} (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.voxel_length = float(voxel_length)
        self.sdf_trunc = float(sdf_trunc)
        self.max_depth = float(max_depth)
        self.unit = BLOCK * self.voxel_length
        if not (self.voxel_length > 0 and 0 < 2 * self.sdf_trunc < self.unit):
            raise ValueError(f"need voxel_length > 0 and 0 < 2 * sdf_trunc < 16 * voxel_length, got {voxel_length}, "
                             f"{sdf_trunc}")
        if int(initial_capacity) < 1:
            raise ValueError("initial_capacity must be >= 1")
        self._keys = torch.empty(0, dtype=torch.int64, device=self.device)
        self._slots = torch.empty(0, dtype=torch.int64, device=self.device)
        self._pool = torch.zeros((int(initial_capacity), 5, VOXELS), dtype=torch.float32, device=self.device)

    # ---------------------------------------------------------------------------------------------------- views
    @property
    def num_blocks(self):
        return int(self._keys.numel())

    @property
    def capacity(self):
        return int(self._pool.shape[0])

    @property
    def keys(self):
        return self._keys.clone()

    @property
    def tsdf(self):
        return self._pool[self._slots, 0].view(-1, BLOCK, BLOCK, BLOCK)

    @property
    def weights(self):
        return self._pool[self._slots, 1].view(-1, BLOCK, BLOCK, BLOCK)

    @property
    def colors(self):
        return self._pool[self._slots, 2:5].view(-1, 3, BLOCK, BLOCK, BLOCK)

    # ------------------------------------------------------------------------------------------------ integrate
    def integrate(self, depth_b1hw, K_b44, cam_T_world_b44, color_b3hw_uint8=None):
        """Integrates a batch of frames in batch order (the same volume as one call per frame).  depth [B,1,H,W] (any
        float dtype, used as fp32; values above max_depth count as 0, values <= 0 and NaN as missing), K [B,4,4],
        cam_T_world [B,4,4] (used as fp32), colour [B,3,H,W] uint8 or None (grey 178)."""
        _require_cuda("depth_b1hw", depth_b1hw)
        _require_cuda("K_b44", K_b44)
        _require_cuda("cam_T_world_b44", cam_T_world_b44)
        if depth_b1hw.dim() != 4 or depth_b1hw.shape[1] != 1:
            raise ValueError(f"depth_b1hw must be [B,1,H,W], got {tuple(depth_b1hw.shape)}")
        B, _, h, w = depth_b1hw.shape
        if tuple(K_b44.shape) != (B, 4, 4) or tuple(cam_T_world_b44.shape) != (B, 4, 4):
            raise ValueError(f"K_b44 and cam_T_world_b44 must be [{B},4,4], got {tuple(K_b44.shape)} and "
                             f"{tuple(cam_T_world_b44.shape)}")
        if color_b3hw_uint8 is not None:
            _require_cuda("color_b3hw_uint8", color_b3hw_uint8)
            if tuple(color_b3hw_uint8.shape) != (B, 3, h, w) or color_b3hw_uint8.dtype != torch.uint8:
                raise ValueError(f"color_b3hw_uint8 must be uint8 [{B},3,{h},{w}], got {color_b3hw_uint8.dtype} "
                                 f"{tuple(color_b3hw_uint8.shape)}")
        if h > 1 << 15 or w > 1 << 15:
            raise ValueError(f"depth maps up to 32768 x 32768, got {h} x {w}")
        if B == 0 or h == 0 or w == 0:
            return
        with _lib.on_device(self.device):
            depth = depth_b1hw.to(self.device)[:, 0].float()
            depth = torch.where(depth > self.max_depth, torch.zeros_like(depth), depth).contiguous()
            K = K_b44.to(self.device).float()
            T = cam_T_world_b44.to(self.device).float()
            color = None if color_b3hw_uint8 is None else color_b3hw_uint8.to(self.device).contiguous()
            for s in range(0, B, MAX_FRAMES):
                e = min(B, s + MAX_FRAMES)
                self._integrate_chunk(depth[s:e], K[s:e], T[s:e], None if color is None else color[s:e])

    def _frames(self, K, T):
        """Host side: frame constants for the touch kernel (fp64 inverse poses) and the integrate kernel (fp32)."""
        host = torch.cat([K.reshape(-1, 16), T.reshape(-1, 16)], 1).cpu().numpy()   # fp32
        Kh, Th = host[:, :16].reshape(-1, 4, 4), host[:, 16:].reshape(-1, 4, 4)
        intr = np.stack([Kh[:, 0, 0], Kh[:, 1, 1], Kh[:, 0, 2], Kh[:, 1, 2]], 1)
        inv = np.linalg.inv(Th.astype(np.float64))
        f64 = np.concatenate([inv[:, :3, :4].reshape(-1, 12), intr.astype(np.float64)], 1)
        f32 = np.concatenate([Th[:, :3, :3].reshape(-1, 9), Th[:, :3, 3], intr], 1).astype(np.float32)
        return (torch.from_numpy(np.ascontiguousarray(f64)).to(self.device),
                torch.from_numpy(np.ascontiguousarray(f32)).to(self.device))

    def _grow(self, needed):
        cap = self.capacity
        if needed <= cap:
            return
        new_cap = max(needed, 2 * cap)
        pool = torch.zeros((new_cap, 5, VOXELS), dtype=torch.float32, device=self.device)
        n = self.num_blocks   # slots 0 .. n-1 are in use
        pool[:n] = self._pool[:n]
        self._pool = pool

    def _integrate_chunk(self, depth, K, T, color):
        b, h, w = depth.shape
        frames_inv, frames = self._frames(K, T)
        S = ((h + 3) // 4) * ((w + 3) // 4)
        cand = torch.empty(b * S * 8, dtype=torch.int64, device=self.device)
        _lib.call("sr_stsdf_touch", self.device, depth, b, h, w, frames_inv, self.sdf_trunc, self.unit, cand)
        ukeys, inverse = torch.unique(cand, sorted=True, return_inverse=True)
        masks = torch.zeros(ukeys.numel(), dtype=torch.int64, device=self.device)
        _lib.call("sr_stsdf_block_masks", self.device, cand, inverse, cand.numel(), S * 8, masks)
        n = self.num_blocks
        valid = ukeys != KEY_NONE
        if n:
            pos = torch.searchsorted(self._keys, ukeys).clamp_(max=n - 1)
            found = valid & (self._keys[pos] == ukeys)
            old_slot = self._slots[pos]
        else:
            found = torch.zeros_like(valid)
            old_slot = torch.zeros_like(ukeys)
        new = valid & ~found
        n_new = int(new.sum())   # the one readback of the merge: the pool may have to grow
        self._grow(n + n_new)
        new_slot = n + torch.cumsum(new, 0) - 1
        slots = torch.where(found, old_slot, torch.where(new, new_slot, torch.full_like(new_slot, -1))).contiguous()
        _lib.call("sr_stsdf_integrate", self.device, self._pool, self.capacity, ukeys, slots, masks, ukeys.numel(), frames,
                  depth, color, b, h, w, self.voxel_length, self.sdf_trunc)
        if n_new:
            keys = torch.cat([self._keys, ukeys[new]])
            slots_all = torch.cat([self._slots, slots[new]])
            keys, order = torch.sort(keys)
            self._keys, self._slots = keys.contiguous(), slots_all[order].contiguous()

    # --------------------------------------------------------------------------------------------------- extract
    def extract_mesh(self) -> TriangleMesh:
        """Marching cubes over the blocks (sr_stsdf_mesh_count + sr_stsdf_mesh_emit): world-space vertices [V,3] fp32,
        faces [F,3] int32 and vertex colours [V,3] fp32 in [0, 1]; no normals.  The output depends only on the block
        set and the voxel data."""
        dev = self.device
        n = self.num_blocks
        empty = TriangleMesh(torch.zeros((0, 3), dtype=torch.float32, device=dev),
                             torch.zeros((0, 3), dtype=torch.int32, device=dev), None,
                             torch.zeros((0, 3), dtype=torch.float32, device=dev))
        if n == 0:
            return empty
        with _lib.on_device(dev):
            counts = torch.empty((2, n), dtype=torch.int32, device=dev)
            _lib.call("sr_stsdf_mesh_count", dev, self._pool, self.capacity, self._keys, self._slots, n, counts)
            c64 = counts.long()
            incl = torch.cumsum(c64, 1)
            offsets = (incl - c64).contiguous()
            nv, nf = (int(x) for x in incl[:, -1].tolist())
            if nv >= 2 ** 31 or nf >= 2 ** 31:
                raise _lib.HipLibraryError(f"mesh of {nv} vertices / {nf} faces: int32 face indices cannot address it")
            if nv == 0:
                return empty
            vtab = torch.empty(n * 3 * VOXELS, dtype=torch.int32, device=dev)
            verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
            colors = torch.empty((nv, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
            _lib.call("sr_stsdf_mesh_emit", dev, self._pool, self.capacity, self._keys, self._slots, n, self.voxel_length,
                      offsets, nv, nf, vtab, verts, colors, faces)
        return TriangleMesh(verts, faces, None, colors)


class Open3DFuser:
    """The fuser behind `--depth_fuser open3d` (reference tools/fusers_helper.py:84-186): a ScalableTSDFVolume with
    voxel_length = fusion_resolution, sdf_trunc = 3 * voxel_length (computed as the reference does, through
    fusion_resolution * 100) and depth above max_fusion_depth ignored.  With fuse_color the frames' ImageNet-normalised
    colour images are resized to the depth size (nearest), un-normalised, scaled by 255, clamped to [0, 255] and
    truncated to uint8 (the clamp is ours: the reference's cast of out-of-range values is undefined); without it the mesh
    is grey (178).  `gt_path` and `use_upsample_depth` are accepted for the reference's signature and, as there, unused."""
    depth_fuser = "open3d"

    def __init__(self, gt_path="", fusion_resolution=0.04, max_fusion_depth=3, fuse_color=False,
                 use_upsample_depth=False, device="cuda"):
        self.gt_path = gt_path
        self.fusion_resolution = fusion_resolution
        self.max_fusion_depth = max_fusion_depth
        self.fusion_max_depth = max_fusion_depth
        self.fuse_color = fuse_color
        self.use_upsample_depth = use_upsample_depth
        voxel_size = fusion_resolution * 100
        self.volume = ScalableTSDFVolume(voxel_length=float(voxel_size) / 100, sdf_trunc=3 * float(voxel_size) / 100,
                                         max_depth=max_fusion_depth, device=device)

    def fuse_frames(self, depths_b1hw, K_b44, cam_T_world_b44, color_b3hw=None):
        color8 = None
        if self.fuse_color:
            if color_b3hw is None:
                raise ValueError("fuse_color is set but no colour images were given")
            _require_cuda("color_b3hw", color_b3hw)
            if color_b3hw.dim() != 4 or color_b3hw.shape[1] != 3 or color_b3hw.shape[0] != depths_b1hw.shape[0]:
                raise ValueError(f"color_b3hw must be [B,3,h,w], got {tuple(color_b3hw.shape)}")
            color = F.interpolate(color_b3hw.float(), size=tuple(depths_b1hw.shape[-2:]))
            color = reverse_imagenet_normalize(color)
            color8 = (color * 255).clamp(0, 255).to(torch.uint8)
        self.volume.integrate(depths_b1hw, K_b44, cam_T_world_b44, color8)

    def get_mesh(self, export_single_mesh=None, convert_to_trimesh=False) -> TriangleMesh:
        """The fused surface as a `TriangleMesh` with vertex colours, on the GPU (`convert_to_trimesh` is accepted for
        the reference's signature and ignored: trimesh is not a dependency)."""
        return self.volume.extract_mesh()

    def export_mesh(self, path, use_marching_cubes_mask=None):
        """Writes the fused surface with vertex colours to `path` as binary PLY (only .ply is written)."""
        if not str(path).lower().endswith(".ply"):
            raise ValueError(f"export_mesh writes PLY only, got {path!r}")
        self.get_mesh().write_ply(path)
