"""Depth and face-id renders of a `TriangleMesh` on HIP kernels (csrc/sr_raster.hip), and the visibility culling they
give.  Geometry only: no shading, materials or colour.  The rules are stated in include/simplerecon_hip.h, section
"mesh rasteriser".

    render_depth(mesh, K_b44, cam_T_world_b44, height, width, ...) -> depth [B,1,H,W] (, face [B,H,W])
    visible_faces(mesh, K_b44, cam_T_world_b44, height, width, min_views=1, ...) -> bool [F]
    cull_to_visible(mesh, K_b44, cam_T_world_b44, height, width, ...) -> TriangleMesh
    Renderer(height, width).render_mesh(meshes, height, width, world_T_cam, K) -> numpy depth [H,W]

There is no CPU path: host tensors raise HipLibraryError."""
import numpy as np
import torch

from . import _lib
from .tsdf import TriangleMesh

CULL_MODES = {"none": 0, "back": 1}   # SR_RASTER_CULL_*
MAX_SIDE = 32768                      # SR_RASTER_MAX_SIDE
RECORD_BYTES = 80                     # SR_RASTER_RECORD_BYTES
MASK_VIEWS = 64                       # SR_RASTER_MASK_VIEWS
MAX_THREADS = 0xffffff00              # SR_RASTER_MAX_THREADS: pixels of one call, and 64 x its (large triangle, tile) items
MAX_PAIRS = 1 << 30                   # SR_RASTER_MAX_PAIRS: (view, face) pairs of one call


def _check_mesh(mesh):
    if not isinstance(mesh, TriangleMesh):
        raise TypeError(f"mesh must be a TriangleMesh, got {type(mesh)}")
    v, f = mesh.vertices, mesh.faces
    if not isinstance(v, torch.Tensor) or not isinstance(f, torch.Tensor):
        raise TypeError("mesh.vertices and mesh.faces must be torch tensors")
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"a mesh has vertices [V,3] and faces [F,3], got {tuple(v.shape)} and {tuple(f.shape)}")
    if v.dtype != torch.float32:
        raise TypeError(f"mesh.vertices must be float32, got {v.dtype}")
    if f.dtype != torch.int32:
        raise TypeError(f"mesh.faces must be int32, got {f.dtype}")
    if v.shape[0] >= 2 ** 31 or f.shape[0] >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 vertices and faces are supported")
    if not v.is_cuda or not f.is_cuda:
        raise _lib.HipLibraryError("the mesh lives on the host: the rasteriser runs on the GPU only (no CPU fallback)")
    if f.device != v.device:
        raise ValueError(f"vertices on {v.device}, faces on {f.device}")
    return v.detach().contiguous(), f.detach().contiguous()


def _check_cameras(K_b44, cam_T_world_b44, device):
    for name, t in (("K_b44", K_b44), ("cam_T_world_b44", cam_T_world_b44)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
        if t.dim() != 3 or tuple(t.shape[1:]) != (4, 4):
            raise ValueError(f"{name} must be [B,4,4], got {tuple(t.shape)}")
        _lib.require_device_f32(name, t)
        if t.device != device:
            raise ValueError(f"{name} on {t.device}, the mesh on {device}")
    if K_b44.shape[0] != cam_T_world_b44.shape[0]:
        raise ValueError(f"{K_b44.shape[0]} intrinsics for {cam_T_world_b44.shape[0]} extrinsics")
    if K_b44.shape[0] < 1:
        raise ValueError("at least one view is needed")
    return K_b44.detach().contiguous(), cam_T_world_b44.detach().contiguous()


def _check_options(height, width, znear, pixel_offset, cull):
    if cull not in CULL_MODES:
        raise ValueError(f"cull must be one of {sorted(CULL_MODES)}, got {cull!r}")
    H, W = int(height), int(width)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"height and width must be in [1, {MAX_SIDE}], got {height} x {width}")
    zn, off = float(znear), float(pixel_offset)
    if not (zn > 0 and np.isfinite(zn)):
        raise ValueError(f"znear must be positive and finite, got {znear}")
    if not -1.0 <= off <= 1.0:
        raise ValueError(f"pixel_offset must be in [-1, 1], got {pixel_offset}")
    return H, W, zn, off, CULL_MODES[cull]


def _check_values(v, f, K):
    """The checks that need the data: face indices inside [0, V) and no skew in K.  One host synchronisation."""
    V = int(v.shape[0])
    if f.shape[0] == 0:
        return
    if V == 0:
        raise ValueError("the mesh has faces but no vertices")
    lo, hi, skew = torch.stack([f.min().double(), f.max().double(),
                                torch.maximum(K[:, 0, 1].abs().max(), K[:, 1, 0].abs().max()).double()]).cpu().tolist()
    if lo < 0 or hi >= V:
        raise ValueError(f"face indices outside [0, {V}) (min {int(lo)}, max {int(hi)})")
    if skew != 0:
        raise ValueError("K_b44 has skew (K[0,1] or K[1,0] is not zero): only fx, fy, cx, cy are supported")


def _launch(v, f, K, T, H, W, zn, off, cull_id, want_depth, want_faces):
    """The kernels, on checked inputs.  One host synchronisation (the number of large triangles), two with any."""
    dev = v.device
    B, V, F = int(K.shape[0]), int(v.shape[0]), int(f.shape[0])
    if B * H * W > MAX_THREADS or B * F > MAX_PAIRS:
        raise ValueError(f"{B} views of {H} x {W} pixels and {F} faces are too many for one call (at most {MAX_THREADS} "
                         f"pixels and {MAX_PAIRS} (view, face) pairs): render the views in groups")
    with _lib.on_device(dev):
        depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if want_depth else None
        face = torch.empty((B, H, W), dtype=torch.int32, device=dev) if want_faces else None
        if F == 0:
            if depth is not None:
                depth.zero_()
            if face is not None:
                face.fill_(-1)
            return depth, face
        keys = torch.empty((B, H, W), dtype=torch.int64, device=dev)
        counters = torch.empty(2, dtype=torch.int32, device=dev)
        scene = (v, V, f, F, K, T, B, H, W, zn, off, cull_id)
        _lib.call("sr_raster_small", dev, *scene, keys, counters)
        n_large = int(counters[0].item())
        if n_large:
            records = torch.empty(n_large * RECORD_BYTES // 8, dtype=torch.float64, device=dev)
            tile_counts = torch.zeros(n_large, dtype=torch.int32, device=dev)
            _lib.call("sr_raster_large_setup", dev, *scene, n_large, counters, records, tile_counts)
            tile_ends = torch.cumsum(tile_counts, 0, dtype=torch.int64)
            n_items = int(tile_ends[-1].item())
            if n_items * 64 > MAX_THREADS:
                raise ValueError(f"{n_items} tiles of large triangles are too many for one call: render the views in groups")
            if n_items:
                _lib.call("sr_raster_large", dev, records, tile_ends, n_large, n_items, K, B, H, W, zn, off, keys)
        _lib.call("sr_raster_resolve", dev, keys, B * H * W, depth, face)
    return depth, face


def _render(mesh, K_b44, cam_T_world_b44, height, width, znear, pixel_offset, cull, want_depth, want_faces):
    H, W, zn, off, cull_id = _check_options(height, width, znear, pixel_offset, cull)
    v, f = _check_mesh(mesh)
    K, T = _check_cameras(K_b44, cam_T_world_b44, v.device)
    with _lib.on_device(v.device):
        _check_values(v, f, K)          # before anything is launched
    return _launch(v, f, K, T, H, W, zn, off, cull_id, want_depth, want_faces)


def render_depth(mesh, K_b44, cam_T_world_b44, height, width, znear=0.05, pixel_offset=0.0, cull="none",
                 return_faces=False):
    """Renders `mesh` (a TriangleMesh on the GPU: vertices fp32, faces int32) into the B cameras K_b44 /
    cam_T_world_b44 ([B,4,4] fp32 device tensors) at height x width.

    Returns depth_b1hw fp32: z along the optical axis of the nearest surface along each pixel's ray, 0 where nothing
    is hit (what pyrender returns for depth).  With return_faces also face_bhw int32: the face seen, -1 where empty;
    among faces at exactly the same depth, the lowest index.  Surface nearer than `znear` is not seen.

    pixel_offset: pixel (u, v) looks along the ray K^-1 (u + pixel_offset, v + pixel_offset, 1).  0.0 is this
    project's convention (BackprojectDepth, the TSDF fusers): backprojecting a render lands on the mesh.  0.5 is the
    OpenGL convention of pixel centres at half-integers, which is what pyrender's IntrinsicsCamera uses as far as its
    projection matrix reads; pyrender could not be run next to this code, so that reading is unverified.
    cull: "none" renders both sides; "back" drops faces whose normal (v1 - v0) x (v2 - v0) points away from the
    camera centre (TriangleMesh's winding: counter-clockwise seen from free space).
    K_b44 must have no skew.  Faces with non-finite vertices or zero area are ignored.

    The result is the same bits on every run and does not depend on how views are grouped into calls.  Host
    synchronisations: one for the checks that read data (face index range, skew), before anything is launched; one for
    the number of triangles whose box is larger than 256 pixels, and a third when there are any.  visible_faces
    checks the mesh once for all its groups of views."""
    depth, face = _render(mesh, K_b44, cam_T_world_b44, height, width, znear, pixel_offset, cull, True,
                          bool(return_faces))
    return (depth, face) if return_faces else depth


def visible_faces(mesh, K_b44, cam_T_world_b44, height, width, min_views=1, znear=0.05, pixel_offset=0.0, cull="none"):
    """bool [F]: the faces that win at least one pixel in at least `min_views` of the views (the views are rendered in
    groups of 64)."""
    mv = int(min_views)
    if mv < 1:
        raise ValueError(f"min_views must be at least 1, got {min_views}")
    H, W, zn, off, cull_id = _check_options(height, width, znear, pixel_offset, cull)
    v, f = _check_mesh(mesh)
    dev = v.device
    K, T = _check_cameras(K_b44, cam_T_world_b44, dev)
    B, F = int(K.shape[0]), int(f.shape[0])
    visible = torch.zeros(F, dtype=torch.uint8, device=dev)
    if F == 0:
        return visible.bool()
    with _lib.on_device(dev):
        _check_values(v, f, K)          # once, not per group of views
        masks = torch.zeros(F, dtype=torch.int64, device=dev)
        counts = torch.zeros(F, dtype=torch.int32, device=dev)
        for b0 in range(0, B, MASK_VIEWS):
            _, face = _launch(v, f, K[b0:b0 + MASK_VIEWS], T[b0:b0 + MASK_VIEWS], H, W, zn, off, cull_id, False, True)
            _lib.call("sr_raster_visibility_mask", dev, face, int(face.shape[0]), H * W, F, masks)
            _lib.call("sr_raster_visibility_count", dev, masks, F, counts, mv, visible)
    return visible.bool()


def cull_to_visible(mesh, K_b44, cam_T_world_b44, height, width, min_views=1, znear=0.05, pixel_offset=0.0, cull="none"):
    """The mesh restricted to its visible faces (visible_faces), with the unreferenced vertices removed; normals and
    colours are carried along.  Vertex and face order are kept.

    Scoring only what the cameras saw, as TransformerFusion's protocol does:

        gt_seen = cull_to_visible(gt, K_b44, cam_T_world_b44, 480, 640)
        scores = mesh_metrics(pred, gt_seen, sampling="surface")
    """
    keep = visible_faces(mesh, K_b44, cam_T_world_b44, height, width, min_views, znear, pixel_offset, cull)
    faces = mesh.faces[keep].long()
    used = torch.zeros(mesh.vertices.shape[0], dtype=torch.bool, device=faces.device)
    used[faces.reshape(-1)] = True
    remap = torch.cumsum(used, 0) - 1
    return TriangleMesh(mesh.vertices[used].contiguous(), remap[faces].to(torch.int32).contiguous(),
                        None if mesh.normals is None else mesh.normals[used].contiguous(),
                        None if mesh.colors is None else mesh.colors[used].contiguous())


class Renderer:
    """The geometry part of the reference's tools/mesh_renderer.py Renderer: depth renders of meshes, on the GPU
    instead of pyrender."""

    def __init__(self, height=480, width=640, device=None):
        self.height, self.width = height, width
        self.device = device

    def render_mesh(self, meshes, height, width, world_T_cam, K, get_colour=False, znear=0.05):
        """Depth [H,W] fp32 (numpy) of the list of TriangleMesh `meshes` seen from the camera pose world_T_cam (4x4,
        numpy or torch) with intrinsics K (3x3 or 4x4).  Pixel centres at half-integers and back-face culling, which
        is how pyrender draws single-sided materials (see render_depth on what is unverified about that).  Colour
        renders are not provided."""
        if get_colour:
            raise NotImplementedError("the rasteriser renders geometry only (depth, face ids): no colour or shading")
        if isinstance(meshes, TriangleMesh):
            meshes = [meshes]
        meshes = list(meshes)
        if not meshes or not all(isinstance(m, TriangleMesh) for m in meshes):
            raise TypeError("meshes must be a non-empty list of TriangleMesh")
        dev = self.device
        if dev is None:
            dev = next((m.vertices.device for m in meshes if m.vertices.is_cuda), None)
        if dev is None:
            if not _lib.cuda_available():
                raise _lib.HipLibraryError("the rasteriser runs on the GPU only and no GPU is visible (no CPU fallback)")
            dev = torch.device("cuda", torch.cuda.current_device())
        dev = torch.device(dev)
        pose = torch.as_tensor(np.asarray(world_T_cam.detach().cpu() if isinstance(world_T_cam, torch.Tensor)
                                          else world_T_cam), dtype=torch.float64).reshape(4, 4)
        k = torch.as_tensor(np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K), dtype=torch.float64)
        K44 = torch.eye(4, dtype=torch.float64)
        if tuple(k.shape) == (3, 3):
            K44[:3, :3] = k
        elif tuple(k.shape) == (4, 4):
            K44 = k
        else:
            raise ValueError(f"K must be 3x3 or 4x4, got {tuple(k.shape)}")
        cam_T_world = torch.linalg.inv(pose)
        verts, faces, base = [], [], 0
        for m in meshes:
            verts.append(m.vertices.detach().to(dev, torch.float32))
            faces.append(m.faces.detach().to(dev, torch.int32) + base)
            base += int(m.vertices.shape[0])
        mesh = TriangleMesh(torch.cat(verts).contiguous(), torch.cat(faces).contiguous())
        depth = render_depth(mesh, K44.float()[None].to(dev), cam_T_world.float()[None].to(dev), height, width,
                             znear=znear, pixel_offset=0.5, cull="back")
        return depth[0, 0].cpu().numpy()
