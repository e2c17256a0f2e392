"""Renders of a `TriangleMesh` on HIP kernels: depth and face ids (csrc/sr_raster.hip), the visibility culling they
give, and colour, shaded and normal pictures shaded from the face-id image, with the vertex normals that needs
(csrc/sr_shade.hip).  The rules are stated in include/simplerecon_hip.h, sections "mesh rasteriser" and "mesh shading".

    render_depth(mesh, K_b44, cam_T_world_b44, height, width, ...) -> depth [B,1,H,W] (, face [B,H,W])
    visible_faces(mesh, K_b44, cam_T_world_b44, height, width, min_views=1, ...) -> bool [F]
    cull_to_visible(mesh, K_b44, cam_T_world_b44, height, width, ...) -> TriangleMesh
    vertex_normals(mesh) -> [V,3];  with_vertex_normals(mesh), normals_as_colors(mesh) -> TriangleMesh
    render_color(mesh, K_b44, cam_T_world_b44, height, width, shading="lambert", ...) -> [B,3,H,W] fp32 / [B,H,W,3] uint8
    render_normals(mesh, K_b44, cam_T_world_b44, height, width, ...) -> unit normals [B,3,H,W], camera frame
    directional_light, point_light, headlight, light_array -> [L,8] fp32 light records
    Renderer(height, width).render_mesh(meshes, height, width, world_T_cam, K) -> numpy depth [H,W]
                           .render_colour(meshes, height, width, world_T_cam, K) -> numpy uint8 [H,W,3]
                           .render_mesh_cull_composite(alpha, ...) -> numpy float [H,W,3]

The shading model is a stated one, ambient plus Lambert, checked against its float64 restatement
(tests/shade_oracle.py).  It is not pyrender's metallic-roughness shader, which the reference draws with: pyrender could
not be run next to this code, so its pictures are not matched and no claim about them is made.

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
SHADING_MODES = {"unlit": 0, "normals": 1, "lambert": 2}            # SR_SHADE_*
NORMAL_MODES = {"smooth": 0, "flat": 1}                             # SR_SHADE_NORMAL_*
LIGHT_KINDS = {"directional": 0, "point": 1, "headlight": 2}        # SR_SHADE_LIGHT_*
MAX_LIGHTS = 32                       # SR_SHADE_MAX_LIGHTS
LIGHT_FLOATS = 8                      # SR_SHADE_LIGHT_FLOATS: kind, xyz, rgb intensity, unused
OUTPUTS = ("f32", "u8", "both")
SHADE_BLOCK = 256                     # pixels of one view that a workgroup of sr_raster_shade owns


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


def vertex_normals(mesh):
    """Area-weighted vertex normals [V,3] fp32 of a TriangleMesh on the GPU: normalise(sum over the faces at a vertex
    of (x1 - x0) x (x2 - x0)), Open3D's compute_vertex_normals rule, summed in float64 in ascending face order -- the
    same bits on every run.  Faces with an index outside [0, V) or non-finite vertices are skipped; a vertex that no
    usable face touches, or whose sum is zero, gets (0, 0, 0).  No host synchronisation."""
    v, f = _check_mesh(mesh)
    dev = v.device
    V, F = int(v.shape[0]), int(f.shape[0])
    with _lib.on_device(dev):
        if V == 0 or F == 0:
            return torch.zeros((V, 3), dtype=torch.float32, device=dev)
        ids = f.reshape(-1).long()
        keys = torch.where((ids >= 0) & (ids < V), ids, torch.full_like(ids, V))
        keys, order = torch.sort(keys, stable=True)       # a vertex's corners in ascending face order
        offsets = torch.searchsorted(keys, torch.arange(V + 1, device=dev))
        out = torch.empty((V, 3), dtype=torch.float32, device=dev)
        _lib.call("sr_mesh_vertex_normals", dev, v, V, f, F, order.contiguous(), offsets.contiguous(), out)
    return out


def with_vertex_normals(mesh):
    """The same mesh with `normals` set to vertex_normals(mesh)."""
    n = vertex_normals(mesh)
    return TriangleMesh(mesh.vertices, mesh.faces, n, mesh.colors)


def normals_as_colors(mesh):
    """The mesh with its vertex normals n and (1 + n) / 2 as vertex colours (the reference's
    visualization_scripts/load_meshes_and_include_normals.py)."""
    n = vertex_normals(mesh)
    return TriangleMesh(mesh.vertices, mesh.faces, n, (1.0 + n) / 2.0)


def _vec3(name, value, unit=False):
    try:
        c = np.asarray(value.detach().cpu() if isinstance(value, torch.Tensor) else value, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise TypeError(f"{name} must be three numbers, got {value!r}") from None
    if c.shape != (3,) or not np.isfinite(c).all():
        raise ValueError(f"{name} must be three finite numbers, got {value!r}")
    if unit and (c.min() < 0 or c.max() > 1):
        raise ValueError(f"{name} must lie in [0, 1], got {value!r}")
    return c


def _light(kind, xyz, color, intensity):
    rgb = _vec3("color", color)
    if rgb.min() < 0:
        raise ValueError(f"color must not be negative, got {color!r}")
    s = float(intensity)
    if not (s >= 0 and np.isfinite(s)):
        raise ValueError(f"intensity must be finite and not negative, got {intensity!r}")
    rec = np.zeros((1, LIGHT_FLOATS), np.float32)
    rec[0, 0] = LIGHT_KINDS[kind]
    rec[0, 1:4] = xyz
    rec[0, 4:7] = rgb * s
    return rec


def directional_light(direction, color=(1.0, 1.0, 1.0), intensity=1.0):
    """[1,8] light record: light travelling along `direction` (world frame; any length but zero)."""
    d = _vec3("direction", direction)
    if not np.linalg.norm(d) > 0:
        raise ValueError("direction must not be zero")
    return _light("directional", d, color, intensity)


def point_light(position, color=(1.0, 1.0, 1.0), intensity=1.0):
    """[1,8] light record: a point light at `position` (world frame), falling off with the squared distance."""
    return _light("point", _vec3("position", position), color, intensity)


def headlight(color=(1.0, 1.0, 1.0), intensity=1.0):
    """[1,8] light record: a light at the camera centre of every view, without fall-off."""
    return _light("headlight", np.zeros(3), color, intensity)


def light_array(center_xyz, x_length=10.0, y_length=10.0, num_x=5, num_y=5, color=(1.0, 1.0, 1.0), intensity=1.0):
    """[num_x * num_y, 8] light records: a grid of point lights in world x / y around `center_xyz`, from -x_length to
    x_length and -y_length to y_length (the reference's create_light_array)."""
    c = _vec3("center_xyz", center_xyz)
    nx, ny = int(num_x), int(num_y)
    if nx < 1 or ny < 1:
        raise ValueError(f"num_x and num_y must be at least 1, got {num_x} and {num_y}")
    X, Y = np.meshgrid(np.linspace(-float(x_length), float(x_length), nx), np.linspace(-float(y_length), float(y_length), ny))
    return np.concatenate([point_light(c + (x, y, 0.0), color, intensity) for x, y in zip(X.ravel(), Y.ravel())])


def _check_lights(lights):
    """`lights` (None, one [L,8] array or a list of them) as one [L,8] fp32 host array."""
    if lights is None:
        return headlight(intensity=0.6)
    parts = list(lights) if isinstance(lights, (list, tuple)) else [lights]
    recs = []
    for part in parts:
        try:
            r = np.asarray(part.detach().cpu() if isinstance(part, torch.Tensor) else part, dtype=np.float32)
        except (TypeError, ValueError):
            raise TypeError(f"lights must be [L,{LIGHT_FLOATS}] arrays, got {type(part)}") from None
        if r.ndim != 2 or r.shape[1] != LIGHT_FLOATS:
            raise ValueError(f"a light array is [L,{LIGHT_FLOATS}], got {tuple(r.shape)}")
        recs.append(r)
    recs = np.concatenate(recs) if recs else np.zeros((0, LIGHT_FLOATS), np.float32)
    if len(recs) > MAX_LIGHTS:
        raise ValueError(f"at most {MAX_LIGHTS} lights, got {len(recs)}")
    if not np.isfinite(recs).all():
        raise ValueError("light records must be finite")
    if not np.isin(recs[:, 0], list(LIGHT_KINDS.values())).all():
        raise ValueError(f"unknown light kind: the first entry of a record is one of {LIGHT_KINDS}")
    return np.ascontiguousarray(recs)


def _check_attribute(name, t, v):
    """Per-vertex colours or normals: [V,3] fp32 on the mesh's device, or None."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if tuple(t.shape) != (v.shape[0], 3):
        raise ValueError(f"{name} must be [{v.shape[0]},3], got {tuple(t.shape)}")
    t = _lib.device_f32(name, t, "the shading kernel reads fp32 attributes")
    if t.device != v.device:
        raise ValueError(f"{name} on {t.device}, the vertices on {v.device}")
    return t.detach()


def _shade(mesh, K_b44, cam_T_world_b44, height, width, shading, normals, lights, ambient, base_color, background,
           znear, pixel_offset, cull, want_f32, want_u8, want_normals, want_depth):
    """Checks, one rasterisation, one deferred pass.  Returns (f32, u8, normals, depth), None where not wanted."""
    if shading not in SHADING_MODES:
        raise ValueError(f"shading must be one of {sorted(SHADING_MODES)}, got {shading!r}")
    if normals not in NORMAL_MODES:
        raise ValueError(f"normals must be one of {sorted(NORMAL_MODES)}, got {normals!r}")
    H, W, zn, off, cull_id = _check_options(height, width, znear, pixel_offset, cull)
    recs = _check_lights(lights)
    amb = float(ambient)
    if not (amb >= 0 and np.isfinite(amb)):
        raise ValueError(f"ambient must be finite and not negative, got {ambient!r}")
    base = torch.from_numpy(_vec3("base_color", base_color, unit=True).astype(np.float32))
    bg = torch.from_numpy(_vec3("background", background, unit=True).astype(np.float32))
    v, f = _check_mesh(mesh)
    colors = _check_attribute("mesh.colors", mesh.colors, v)
    vn = _check_attribute("mesh.normals", mesh.normals, v)
    dev = v.device
    K, T = _check_cameras(K_b44, cam_T_world_b44, dev)
    B, V, F = int(K.shape[0]), int(v.shape[0]), int(f.shape[0])
    if B * (-(-H * W // SHADE_BLOCK) * SHADE_BLOCK) > MAX_THREADS:
        raise ValueError(f"{B} views of {H} x {W} pixels are too many for one call: render the views in groups")
    with _lib.on_device(dev):
        _check_values(v, f, K)          # before anything is launched
    smooth = normals == "smooth" and (shading != "unlit" or want_normals)
    if smooth and vn is None and F:
        vn = vertex_normals(mesh)
    depth, face = _launch(v, f, K, T, H, W, zn, off, cull_id, want_depth, True)
    with _lib.on_device(dev):
        f32 = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if want_f32 else None
        u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) if want_u8 else None
        nrm = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if want_normals else None
        if F == 0:                      # nothing to shade: the background
            if f32 is not None:
                f32.copy_(bg.to(dev).view(1, 3, 1, 1).expand_as(f32))
            if u8 is not None:
                u8.copy_((bg * 255.0).to(torch.uint8).to(dev).view(1, 1, 1, 3).expand_as(u8))
            if nrm is not None:
                nrm.zero_()
        else:
            lights_t = torch.from_numpy(recs) if len(recs) else None
            _lib.call("sr_raster_shade", dev, v, V, f, F, K, T, B, H, W, off, face, colors, vn if smooth else None,
                      base, bg, amb, lights_t, len(recs), SHADING_MODES[shading], NORMAL_MODES[normals], f32, u8, nrm)
    return f32, u8, nrm, depth


def render_color(mesh, K_b44, cam_T_world_b44, height, width, shading="lambert", normals="smooth", lights=None,
                 ambient=0.4, base_color=(0.6, 0.6, 0.6), background=(1.0, 1.0, 1.0), znear=0.05, pixel_offset=0.0,
                 cull="none", output="f32", return_depth=False):
    """A colour picture of `mesh` in each of the B cameras (render_depth's arguments and conventions): the mesh is
    rasterised once and every pixel is shaded from the face it shows.

    shading: "unlit" is the base colour c -- mesh.colors ([V,3] fp32 in [0, 1]) interpolated perspective-correctly,
    or base_color; "normals" is 0.5 (1 + n) with n in the camera frame, the look of the normal maps; "lambert" is
    c (ambient + sum over the lights of intensity max(0, n . l) attenuation).
    normals: "flat" uses the face's normal, "smooth" the interpolated mesh.normals ([V,3] fp32, world frame;
    vertex_normals(mesh) when the mesh has none).  Both sides of a face are lit: n always faces the viewer.
    lights: an [L,8] array from directional_light / point_light / headlight / light_array, or a list of them, at most
    32 records; None is one white headlight of intensity 0.6.
    output: "f32" -> [B,3,H,W] fp32 in [0, 1]; "u8" -> [B,H,W,3] uint8 = (uint8)(f32 * 255); "both" -> the two.
    Empty pixels get `background`.  With return_depth the depth [B,1,H,W] of render_depth follows.

    A stated model, not pyrender's metallic-roughness shader (see the module docstring).  Same bits on every run."""
    if output not in OUTPUTS:
        raise ValueError(f"output must be one of {OUTPUTS}, got {output!r}")
    f32, u8, _, depth = _shade(mesh, K_b44, cam_T_world_b44, height, width, shading, normals, lights, ambient, base_color,
                               background, znear, pixel_offset, cull, output != "u8", output != "f32", False,
                               bool(return_depth))
    res = [t for t in (f32, u8, depth) if t is not None]
    return res[0] if len(res) == 1 else tuple(res)


def render_normals(mesh, K_b44, cam_T_world_b44, height, width, normals="smooth", znear=0.05, pixel_offset=0.0,
                   cull="none", return_depth=False):
    """Unit normals [B,3,H,W] fp32 of the surface each pixel shows, in the camera frame and facing the viewer; 0 where
    the pixel is empty.  normals as in render_color."""
    _, _, nrm, depth = _shade(mesh, K_b44, cam_T_world_b44, height, width, "unlit", normals, [], 0.0, (0.0, 0.0, 0.0),
                              (0.0, 0.0, 0.0), znear, pixel_offset, cull, False, False, True, bool(return_depth))
    return (nrm, depth) if return_depth else nrm


class Renderer:
    """The reference's tools/mesh_renderer.py Renderer on the GPU instead of pyrender: depth renders of meshes, and
    colour renders under this module's shading model (not pyrender's)."""

    def __init__(self, height=480, width=640, device=None):
        self.height, self.width = height, width
        self.device = device

    def _scene(self, meshes, world_T_cam, K):
        """The device, the list of meshes and the camera (K [4,4], cam_T_world [4,4], float64 on the host)."""
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
        return dev, meshes, K44, torch.linalg.inv(pose)

    def render_colour(self, meshes, height, width, world_T_cam, K, lights=None, mesh_colors=None, cull="back",
                      znear=0.05):
        """Colour picture [H,W,3] uint8 (numpy) of the list of TriangleMesh `meshes` (concatenated) seen from the
        camera pose world_T_cam with intrinsics K, as render_mesh takes them: render_color's lambert shading with smooth
        normals, pixel centres at half-integers.  A mesh without vertex colours gets its entry of `mesh_colors` (a list
        of rgb triples in [0, 1], one per mesh; None entries allowed), or the 0.6 grey."""
        if mesh_colors is not None:
            n = len(meshes) if isinstance(meshes, (list, tuple)) else 1
            mesh_colors = list(mesh_colors)
            if len(mesh_colors) != n:
                raise ValueError(f"{len(mesh_colors)} mesh_colors for {n} meshes")
            mesh_colors = [None if c is None else _vec3("mesh_colors", c, unit=True) for c in mesh_colors]
        if cull not in CULL_MODES:
            raise ValueError(f"cull must be one of {sorted(CULL_MODES)}, got {cull!r}")
        lights = _check_lights(lights)
        dev, meshes, K44, cam_T_world = self._scene(meshes, world_T_cam, K)
        coloured = mesh_colors is not None or any(m.colors is not None for m in meshes)
        verts, faces, colors, normals, base = [], [], [], [], 0
        for i, m in enumerate(meshes):
            nv = int(m.vertices.shape[0])
            verts.append(m.vertices.detach().to(dev, torch.float32))
            faces.append(m.faces.detach().to(dev, torch.int32) + base)
            base += nv
            if m.colors is not None:
                colors.append(m.colors.detach().to(dev, torch.float32))
            elif coloured:
                c = mesh_colors[i] if mesh_colors is not None and mesh_colors[i] is not None else (0.6, 0.6, 0.6)
                colors.append(torch.tensor(c, dtype=torch.float32, device=dev).expand(nv, 3))
            if m.normals is not None:
                normals.append(m.normals.detach().to(dev, torch.float32))
        mesh = TriangleMesh(torch.cat(verts).contiguous(), torch.cat(faces).contiguous(),
                            torch.cat(normals).contiguous() if len(normals) == len(meshes) else None,
                            torch.cat(colors).contiguous() if coloured else None)
        picture = render_color(mesh, K44.float()[None].to(dev), cam_T_world.float()[None].to(dev), height, width,
                               lights=lights, znear=znear, pixel_offset=0.5, cull=cull, output="u8")
        return picture[0].cpu().numpy()

    def render_mesh_cull_composite(self, alpha, **kwargs):
        """culled * (1 - alpha) + non_culled * alpha as float64 [H,W,3]: render_colour (its arguments, but `cull`)
        with back faces culled, blended with the picture that shows them."""
        if "cull" in kwargs:
            raise TypeError("render_mesh_cull_composite renders with both cull modes: cull cannot be given")
        a = float(alpha)
        culled = self.render_colour(cull="back", **kwargs).astype(np.float64)
        non_culled = self.render_colour(cull="none", **kwargs).astype(np.float64)
        return culled * (1.0 - a) + non_culled * a

    def render_mesh(self, meshes, height, width, world_T_cam, K, get_colour=False, znear=0.05):
        """Depth [H,W] fp32 (numpy) of the list of TriangleMesh `meshes` seen from the camera pose world_T_cam (4x4,
        numpy or torch) with intrinsics K (3x3 or 4x4).  Pixel centres at half-integers and back-face culling, which
        is how pyrender draws single-sided materials (see render_depth on what is unverified about that).  Colour
        renders come from render_colour, not from get_colour."""
        if get_colour:
            raise NotImplementedError("render_mesh returns depth only: colour pictures come from Renderer.render_colour "
                                      "(this module's shading model, not pyrender's)")
        dev, meshes, K44, cam_T_world = self._scene(meshes, world_T_cam, K)
        verts, faces, base = [], [], 0
        for m in meshes:
            verts.append(m.vertices.detach().to(dev, torch.float32))
            faces.append(m.faces.detach().to(dev, torch.int32) + base)
            base += int(m.vertices.shape[0])
        mesh = TriangleMesh(torch.cat(verts).contiguous(), torch.cat(faces).contiguous())
        depth = render_depth(mesh, K44.float()[None].to(dev), cam_T_world.float()[None].to(dev), height, width,
                             znear=znear, pixel_offset=0.5, cull="back")
        return depth[0, 0].cpu().numpy()
