"""Deterministic synthetic inputs for the plane-sweep hot path.

ScanNet-shaped geometry: intrinsics fx = fy = 577.87 * (w / 640) with the
principal point at the image centre (cf. reference datasets/scannet_dataset.py:
448-470, K scaled by the feature-map width), the reference camera at the
identity, source view k rotated 0.05*(k+1) rad about y and translated
(0.10, -0.03, 0.02)*(k+1) m (DVMVS-like baselines, reference
tools/keyframe_buffer.py:12-22), N(0,1) matching features (InstanceNorm output,
reference modules/networks.py:201) and 0.25 m .. 5.0 m matching depths
(reference options.py:133-134).

Everything is generated with numpy so that the same seed gives the same bytes on
the build container, the GPU box and inside the golden-vector generator.
"""
import zlib

import numpy as np
import torch

MIN_DEPTH = 0.25
MAX_DEPTH = 5.0


def intrinsics(h, w, dtype=np.float32):
    """4x4 pinhole K at feature-map resolution h x w (and its inverse)."""
    K = np.eye(4, dtype=np.float64)
    f = 577.87 * (w / 640.0)
    K[0, 0] = f
    K[1, 1] = f
    K[0, 2] = w / 2.0
    K[1, 2] = h / 2.0
    return K.astype(dtype), np.linalg.inv(K).astype(dtype)


def _rot_y(theta):
    c, s = np.cos(theta), np.sin(theta)
    R = np.eye(4)
    R[0, 0], R[0, 2], R[2, 0], R[2, 2] = c, s, -s, c
    return R


def _small_rot(rng, scale):
    """Random small rotation (Rodrigues) for per-batch jitter."""
    v = rng.normal(size=3) * scale
    th = np.linalg.norm(v)
    if th < 1e-12:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def poses(B, K, seed=0, jitter=0.02):
    """Returns (src_poses = cur_cam_T_src_cam, src_extrinsics = src_cam_T_cur_cam), [B,K,4,4] fp32.

    Batch element 0 is the exact §8d layout; further elements add a seeded jitter so
    that a batch is not B copies of the same geometry."""
    rng = np.random.default_rng(1000 + seed)
    src_poses = np.zeros((B, K, 4, 4))
    for b in range(B):
        for k in range(K):
            T = _rot_y(0.05 * (k + 1))
            T[:3, 3] = np.array([0.10, -0.03, 0.02]) * (k + 1)
            if b > 0 and jitter > 0:
                J = np.eye(4)
                J[:3, :3] = _small_rot(rng, jitter)
                J[:3, 3] = rng.normal(size=3) * jitter
                T = J @ T
            src_poses[b, k] = T
    src_extr = np.linalg.inv(src_poses)
    return src_poses.astype(np.float32), src_extr.astype(np.float32)


def keyframe_poses(ids, K, jitter=0.02):
    """Poses of the keyframes of a STREAM: a function of the keyframe id alone (so that a keyframe gets the same
    cameras whatever rank / batch it lands in): the §8d layout composed with a small rigid jitter seeded by the id.
    Returns (src_poses, src_extrinsics), [len(ids),K,4,4] fp32."""
    base = np.zeros((K, 4, 4))
    for k in range(K):
        T = _rot_y(0.05 * (k + 1))
        T[:3, 3] = np.array([0.10, -0.03, 0.02]) * (k + 1)
        base[k] = T
    src_poses = np.zeros((len(ids), K, 4, 4))
    for j, i in enumerate(ids):
        rng = np.random.default_rng(500000 + int(i))
        for k in range(K):
            J = np.eye(4)
            J[:3, :3] = _small_rot(rng, jitter)
            J[:3, 3] = rng.normal(size=3) * jitter
            src_poses[j, k] = J @ base[k]
    src_extr = np.linalg.inv(src_poses)
    return src_poses.astype(np.float32), src_extr.astype(np.float32)


def cost_volume_inputs(B, K, C, h, w, seed=0, device="cpu", jitter=0.02):
    """Keyword arguments of CostVolumeManager.forward (reference cost_volume.py:345-357)."""
    rng = np.random.default_rng(seed)
    cur = rng.standard_normal((B, C, h, w), dtype=np.float32)
    src = rng.standard_normal((B, K, C, h, w), dtype=np.float32)
    Kmat, invK = intrinsics(h, w)
    src_poses, src_extr = poses(B, K, seed, jitter)
    out = dict(
        cur_feats=torch.from_numpy(cur),
        src_feats=torch.from_numpy(src),
        src_extrinsics=torch.from_numpy(src_extr),
        src_poses=torch.from_numpy(src_poses),
        src_Ks=torch.from_numpy(np.broadcast_to(Kmat, (B, K, 4, 4)).copy()),
        cur_invK=torch.from_numpy(np.broadcast_to(invK, (B, 4, 4)).copy()),
        min_depth=torch.tensor(MIN_DEPTH, dtype=torch.float32).view(1, 1, 1, 1),
        max_depth=torch.tensor(MAX_DEPTH, dtype=torch.float32).view(1, 1, 1, 1),
    )
    return {k: v.to(device) for k, v in out.items()}


def image_prior_pyramid(B, h, w, chans=(24, 48, 64, 160, 256), seed=0, device="cpu"):
    """Stand-in for the image-prior encoder's 5-scale pyramid (reference depth_model.py:346:
    EfficientNetV2-S features, channels [24,48,64,160,256] at 1/2 .. 1/32 of the image).
    (h, w) is the MATCHING resolution (= image / 4): scales are 2h, h, h/2, h/4, h/8."""
    rng = np.random.default_rng(77 + seed)
    feats = []
    for i, c in enumerate(chans):
        hh, ww = (2 * h) >> i, (2 * w) >> i
        feats.append(torch.from_numpy(rng.standard_normal((B, c, hh, ww), dtype=np.float32)).to(device))
    return feats


def seeded_fill_(module, seed=0, gain=1.0):
    """Deterministically (re)initialises every parameter of `module` from a numpy RNG keyed
    by the parameter NAME, so two modules with the same state-dict layout (ours and the
    reference's) get bit-identical weights without shipping them.  Weights ~ U(-a, a) with
    a = gain*sqrt(3/fan_in) (variance-preserving), biases ~ U(-0.1, 0.1).  BatchNorm layers get
    non-trivial statistics: weight, running_var ~ U(0.5, 1.5); bias, running_mean ~ U(-0.2, 0.2)."""
    bn_scale, bn_shift = set(), set()
    for mname, m in module.named_modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            pre = mname + "." if mname else ""
            bn_scale.update({pre + "weight", pre + "running_var"})
            bn_shift.update({pre + "bias", pre + "running_mean"})
    with torch.no_grad():
        named = list(module.named_parameters())
        named += [(n, b) for n, b in module.named_buffers() if n in bn_scale or n in bn_shift]
        for name, p in named:
            rng = np.random.default_rng((zlib.crc32(name.encode()) + 7919 * seed) & 0x7FFFFFFF)
            if name in bn_scale:
                v = rng.uniform(0.5, 1.5, size=tuple(p.shape)).astype(np.float32)
            elif name in bn_shift:
                v = rng.uniform(-0.2, 0.2, size=tuple(p.shape)).astype(np.float32)
            elif p.dim() > 1:
                fan_in = int(np.prod(p.shape[1:]))
                a = gain * np.sqrt(3.0 / fan_in)
                v = rng.uniform(-a, a, size=tuple(p.shape)).astype(np.float32)
            else:
                v = rng.uniform(-0.1, 0.1, size=tuple(p.shape)).astype(np.float32)
            p.copy_(torch.from_numpy(v).to(p.device))
    return module


def _scene_layout(rng):
    """raycast_scene's room and primitives, drawn from `rng` (the draws come first, so the camera path that follows them
    is unchanged): room [2,3] (min, max corner) and [(kind, params, base colour)] for three boxes ((lo, hi) corners)
    and two spheres ((centre, radius))."""
    room = np.array([[-2.5, -1.5, -2.5], [2.5, 1.5, 2.5]])
    prims = []   # (kind, params, base colour)
    for k in range(3):
        a = 2 * np.pi * (k / 3.0) + rng.uniform(-0.4, 0.4)
        c = np.array([1.85 * np.cos(a), rng.uniform(0.2, 1.0), 1.85 * np.sin(a)])
        half = rng.uniform(0.2, 0.4, size=3)
        prims.append(("box", (c - half, c + half), rng.uniform(40, 215, size=3)))
    for k in range(2):
        a = 2 * np.pi * (k / 2.0 + 0.25) + rng.uniform(-0.3, 0.3)
        c = np.array([1.6 * np.cos(a), rng.uniform(-0.6, 0.4), 1.6 * np.sin(a)])
        prims.append(("sphere", (c, rng.uniform(0.25, 0.4)), rng.uniform(40, 215, size=3)))
    return room, prims


def _box_faces(lo, hi, spacing, inward):
    """The six faces of an axis-aligned box as quad grids of about `spacing`, two triangles per quad; normals point
    out of the box (into it when inward)."""
    verts, tris, base = [], [], 0
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        nb = max(1, int(np.ceil((hi[b] - lo[b]) / spacing)))
        nc = max(1, int(np.ceil((hi[c] - lo[c]) / spacing)))
        ub = np.linspace(lo[b], hi[b], nb + 1)
        uc = np.linspace(lo[c], hi[c], nc + 1)
        gb, gc = np.meshgrid(ub, uc, indexing="ij")
        i = np.arange(nb)[:, None] * (nc + 1) + np.arange(nc)[None, :]
        q = np.stack([i, i + nc + 1, i + nc + 2, i + 1], -1).reshape(-1, 4)   # counter-clockwise about e_b x e_c = e_a
        for side, val in ((-1, lo[a]), (1, hi[a])):
            v = np.empty((gb.size, 3))
            v[:, a], v[:, b], v[:, c] = val, gb.ravel(), gc.ravel()
            t = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 0)
            if (side < 0) != inward:
                t = t[:, ::-1]
            verts.append(v)
            tris.append(t + base)
            base += len(v)
    return verts, tris


def _sphere_faces(centre, radius, spacing):
    n_lat = max(4, int(np.ceil(np.pi * radius / spacing)))
    n_lon = max(8, int(np.ceil(2 * np.pi * radius / spacing)))
    th = np.linspace(0.0, np.pi, n_lat + 1)[:, None]
    ph = np.linspace(0.0, 2 * np.pi, n_lon + 1)[None, :]
    v = np.stack([np.sin(th) * np.cos(ph), np.cos(th) + 0 * ph, np.sin(th) * np.sin(ph)], -1).reshape(-1, 3)
    i = np.arange(n_lat)[:, None] * (n_lon + 1) + np.arange(n_lon)[None, :]
    q = np.stack([i, i + 1, i + n_lon + 2, i + n_lon + 1], -1).reshape(-1, 4)
    t = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 0)
    return np.asarray(centre) + radius * v, t


def raycast_scene_mesh(seed=0, spacing=0.02):
    """The analytic ground truth of raycast_scene(seed=seed) as a CPU TriangleMesh: the room's walls (normals inward),
    the three boxes and the two spheres (normals outward), tessellated at about `spacing` metres.  Primitives are
    tessellated whole: parts inside another primitive are kept, pole triangles of the spheres have zero area."""
    from .tsdf import TriangleMesh
    room, prims = _scene_layout(np.random.default_rng(7000 + seed))
    verts, tris = _box_faces(room[0], room[1], spacing, inward=True)
    base = sum(len(v) for v in verts)
    for kind, par, _ in prims:
        if kind == "box":
            vs, ts = _box_faces(par[0], par[1], spacing, inward=False)
        else:
            v, t = _sphere_faces(par[0], par[1], spacing)
            vs, ts = [v], [t]
        for v, t in zip(vs, ts):
            verts.append(v)
            tris.append(t + base)
            base += len(v)
    v = torch.from_numpy(np.concatenate(verts, 0).astype(np.float32))
    f = torch.from_numpy(np.concatenate(tris, 0).astype(np.int32))
    return TriangleMesh(v, f)


def raycast_scene(N, h, w, seed=0, noise=0.0, holes=0.0, device="cpu"):
    """A ray-cast indoor scene for point-cloud fusion: a 5 x 3 x 5 m box room with three boxes and two spheres, seen
    by N cameras on a slow loop inside it.  Depth is exact (up to fp32), so it is multi-view consistent except at
    occlusions; `noise` adds N(0, noise) relative depth error and `holes` zeroes that fraction of the pixels.

    Returns depths [N,h,w] fp32 (z along the optical axis), images [N,h,w,3] uint8, cam_T_world [N,4,4] fp32 and
    K [N,3,3] fp32.  The layout, the camera path and the noise come from numpy's generator (the same seed gives the
    same scene everywhere); the rays are cast in fp64 torch on `device`."""
    rng = np.random.default_rng(7000 + seed)
    room, prims = _scene_layout(rng)

    f = 577.87 * (w / 640.0)
    K = np.array([[f, 0.0, (w - 1) / 2.0 + 0.3], [0.0, f, (h - 1) / 2.0 - 0.2], [0.0, 0.0, 1.0]])
    cam_T_world = np.zeros((N, 4, 4))
    for i in range(N):
        th = 0.05 * i + rng.uniform(-0.01, 0.01)
        pos = np.array([0.8 * np.cos(th), 0.1 * np.sin(0.07 * i), 0.8 * np.sin(th)])
        yaw = th + np.pi / 2 + 0.3 * np.sin(0.11 * i)
        pitch = 0.1 * np.sin(0.05 * i)
        fwd = np.array([np.cos(yaw) * np.cos(pitch), np.sin(pitch), np.sin(yaw) * np.cos(pitch)])
        down = np.array([0.0, 1.0, 0.0]) - fwd[1] * fwd
        down /= np.linalg.norm(down)
        right = np.cross(down, fwd)
        T = np.eye(4)
        T[:3, :3] = np.stack([right, down, fwd], 1)   # world_T_cam: camera x right, y down, z forward
        T[:3, 3] = pos
        cam_T_world[i] = np.linalg.inv(T)

    dt = dict(dtype=torch.float64, device=device)
    vv, uu = torch.meshgrid(torch.arange(h, **dt), torch.arange(w, **dt), indexing="ij")
    pix = torch.stack([uu, vv, torch.ones_like(uu)], -1).reshape(-1, 3)
    dir_cam = pix @ torch.as_tensor(np.linalg.inv(K), **dt).T           # z = 1: the hit distance t is the depth
    wTc = torch.as_tensor(np.linalg.inv(cam_T_world), **dt)
    d = torch.einsum("nij,pj->npi", wTc[:, :3, :3], dir_cam)            # [N,P,3], not normalised
    o = wTc[:, None, :3, 3].expand_as(d)
    inf = torch.tensor(float("inf"), **dt)
    lo, hi = torch.as_tensor(room[0], **dt), torch.as_tensor(room[1], **dt)
    t_wall = torch.where(d > 0, (hi - o) / d, (lo - o) / d)
    t_wall = torch.where(d == 0, inf, t_wall)
    best, axis = t_wall.min(-1)
    obj = axis                                                     # 0..2: the wall's axis
    for pi, (kind, par, _) in enumerate(prims):
        if kind == "box":
            blo, bhi = torch.as_tensor(par[0], **dt), torch.as_tensor(par[1], **dt)
            t1, t2 = (blo - o) / d, (bhi - o) / d
            tmin = torch.minimum(t1, t2).nan_to_num(nan=-float("inf")).max(-1).values
            tmax = torch.maximum(t1, t2).nan_to_num(nan=float("inf")).min(-1).values
            hit = (tmax >= tmin) & (tmin > 0)
            t = torch.where(hit, tmin, inf)
        else:
            c, r = torch.as_tensor(par[0], **dt), par[1]
            oc = o - c
            a = (d * d).sum(-1)
            b = (d * oc).sum(-1)
            disc = b * b - a * ((oc * oc).sum(-1) - r * r)
            t = (-b - disc.clamp(min=0).sqrt()) / a
            t = torch.where((disc >= 0) & (t > 0), t, inf)
        closer = t < best
        best = torch.where(closer, t, best)
        obj = torch.where(closer, torch.full_like(obj, 3 + pi), obj)
    hitp = o + best[..., None] * d
    checker = (torch.floor(hitp * 4.0).sum(-1).remainder(2.0))             # 0 / 1
    base = torch.as_tensor(np.concatenate([np.array([[200, 180, 150], [120, 140, 170], [160, 200, 140]]),
                                           np.stack([p[2] for p in prims])]), **dt)
    rgb = base[obj] * (0.7 + 0.3 * checker)[..., None]
    depth = best.reshape(N, h, w)
    if noise > 0:
        depth = depth * (1.0 + torch.as_tensor(rng.standard_normal((N, h, w)) * noise, **dt))
    if holes > 0:
        depth = torch.where(torch.as_tensor(rng.random((N, h, w)) < holes, device=device), 0.0, depth)
    return dict(depths=depth.float().contiguous(),
                images=rgb.round().clamp(0, 255).to(torch.uint8).reshape(N, h, w, 3).contiguous(),
                cam_T_world=torch.as_tensor(cam_T_world, dtype=torch.float32, device=device),
                K=torch.as_tensor(np.repeat(K[None], N, 0), dtype=torch.float32, device=device))


def training_batch(B, K, h, w, seed=0, device="cpu", holes=0.003, matching_scale=1):
    """A (cur_data, src_data) training batch with the reference's keys, from raycast_scene: gt depths [B,1,h,w] and
    source depths [B,K,1,h,w] with NaN holes (random pixels and one rectangle per map, some touching the border),
    `mask_b_b1hw` / `mask_b1hw` (finite depth inside [MIN_DEPTH, MAX_DEPTH]), images at 2h x 2w, K / invK at scale 0
    (the depth map) and at `matching_scale`, and the poses.  Frame b * (K + 1) is the current view of batch item b,
    the K frames after it its sources."""
    n = B * (K + 1)
    sc = raycast_scene(n, h, w, seed=seed, holes=holes, device="cpu")
    img = raycast_scene(n, 2 * h, 2 * w, seed=seed, device="cpu")["images"]
    rng = np.random.default_rng(9100 + seed)
    depth = sc["depths"].clone()
    depth[depth == 0] = float("nan")
    for i in range(n):
        rh, rw = int(rng.integers(2, max(3, h // 4))), int(rng.integers(2, max(3, w // 4)))
        y0, x0 = int(rng.integers(0, h - rh + 1)), int(rng.integers(0, w - rw + 1))
        if i % 2 == 0:
            x0 = 0 if i % 4 == 0 else w - rw   # touch the border
        depth[i, y0:y0 + rh, x0:x0 + rw] = float("nan")
    images = (img.permute(0, 3, 1, 2).float() / 255.0 - 0.45) / 0.225
    Ks = torch.eye(4).repeat(n, 1, 1)
    Ks[:, :3, :3] = sc["K"]
    cTw = sc["cam_T_world"]
    wTc = torch.linalg.inv(cTw.double()).float()
    cur = torch.arange(B) * (K + 1)
    src = cur[:, None] + 1 + torch.arange(K)[None]
    mask = torch.isfinite(depth) & (depth > MIN_DEPTH) & (depth < MAX_DEPTH)
    cur_data = {"image_b3hw": images[cur], "depth_b1hw": depth[cur].unsqueeze(1),
                "mask_b_b1hw": mask[cur].unsqueeze(1), "mask_b1hw": mask[cur].unsqueeze(1).float(),
                "cam_T_world_b44": cTw[cur], "world_T_cam_b44": wTc[cur]}
    src_data = {"image_b3hw": images[src], "depth_b1hw": depth[src].unsqueeze(2),
                "cam_T_world_b44": cTw[src], "world_T_cam_b44": wTc[src]}
    for s in sorted({0, matching_scale}):
        Kx = Ks.clone()
        Kx[:, :2] /= 2 ** s
        invK = torch.linalg.inv(Kx.double()).float()
        cur_data[f"K_s{s}_b44"], cur_data[f"invK_s{s}_b44"] = Kx[cur], invK[cur]
        src_data[f"K_s{s}_b44"], src_data[f"invK_s{s}_b44"] = Kx[src], invK[src]
    return ({k: v.to(device) for k, v in cur_data.items()}, {k: v.to(device) for k, v in src_data.items()})
