"""Mesh and point-cloud metrics on HIP kernels (csrc/sr_meshmetrics.hip): exact nearest neighbours, area-weighted
surface sampling and the Acc / Comp / Chamfer / Precision / Recall / F-score table of the reference README's "Mesh
Fusion" results.  The rules are stated in include/simplerecon_hip.h, section "mesh metrics".

    nearest_distances(query [M,3], target [N,3], return_index=False) -> dist [M] (, index [M])   device tensors
    sample_surface(mesh, n_points, seed=0)                           -> PointCloud               area-weighted
    mesh_metrics(pred, gt, threshold=0.05, sampling="vertices", ...) -> dict of the six metrics, in metres

There is no CPU path: host tensors raise HipLibraryError."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .point_cloud import PointCloud
from .tsdf import TriangleMesh

MAX_CELLS = 1 << 26        # SR_NN_MAX_CELLS
MAX_COORD = 1e18           # SR_NN_MAX_COORD
METRIC_KEYS = ("acc", "comp", "chamfer", "precision", "recall", "f_score")
# Surface samples per mesh for sampling="surface".  A ScanNet room has 50 to 100 m^2 of surface; 200k samples put them
# about 2 cm apart, the voxel size of the vertex protocol's downsampling, so the two protocols score a surface at a
# similar density.  It is our choice, not a count taken from TransformerFusion's evaluation.
DEFAULT_SURFACE_POINTS = 200_000


def _points(name, t):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be [n,3], got {tuple(t.shape)}")
    _lib.require_device_f32(name, t)
    if t.shape[0] >= 2 ** 31:
        raise ValueError(f"{name}: {t.shape[0]} points; at most 2^31 - 1 are supported")
    return t.contiguous()


def _boxes(*pts):
    """fp64 boxes [k,6] (min xyz, max xyz) of non-empty point sets, read back in ONE host synchronisation; refuses
    non-finite coordinates and coordinates beyond MAX_COORD."""
    rows = torch.stack([torch.cat([p.amin(0), p.amax(0)]) for p in pts]).double().cpu().numpy()
    if not np.isfinite(rows).all() or (np.abs(rows) > MAX_COORD).any():
        raise ValueError(f"nearest neighbours need finite coordinates with |x| <= {MAX_COORD:g}")
    return rows


class _TargetGrid:
    """The sorted targets and the cell-start table of one target set (sr_nn_grid_plan, sr_nn_keys, torch.sort,
    sr_nn_build)."""

    def __init__(self, target, box, max_cells=MAX_CELLS):
        lib = _lib.lib()
        n = int(target.shape[0])
        b = (C.c_double * 6)(*[float(x) for x in box])
        cell, dims, entries = C.c_double(), (C.c_int * 3)(), C.c_int64()
        rc = lib.sr_nn_grid_plan(n, C.addressof(b), int(max_cells), C.addressof(cell), C.addressof(dims), C.addressof(entries))
        if rc != 0:   # (a host-side query: no launch, no stream)
            raise _lib.HipLibraryError(f"sr_nn_grid_plan failed: error {rc}")
        self.n = n
        self.origin = [float(x) for x in box[:3]]
        self.cell = cell.value
        self.dims = [int(d) for d in dims]
        self.entries = int(entries.value)
        dev = target.device
        keys = self.keys(target)
        skeys, order = torch.sort(keys, stable=True)
        self.sorted = torch.empty((n, 4), dtype=torch.float32, device=dev)
        self.start = torch.empty(self.entries, dtype=torch.int32, device=dev)
        _lib.call("sr_nn_build", dev, target, n, skeys, order, self.entries, self.sorted, self.start)

    def _grid_args(self):
        return [*self.origin, self.cell, *self.dims]

    def keys(self, pts):
        keys = torch.empty(int(pts.shape[0]), dtype=torch.int32, device=pts.device)
        _lib.call("sr_nn_keys", pts.device, pts, int(pts.shape[0]), *self._grid_args(), keys)
        return keys

    def query(self, q, want_d2=False, want_dist=True, want_index=False):
        M, dev = int(q.shape[0]), q.device
        d2 = torch.empty(M, dtype=torch.float32, device=dev) if want_d2 else None
        dist = torch.empty(M, dtype=torch.float32, device=dev) if want_dist else None
        idx = torch.empty(M, dtype=torch.int32, device=dev) if want_index else None
        if M:
            _, order = torch.sort(self.keys(q))   # neighbouring queries in neighbouring lanes; results do not depend on it
            _lib.call("sr_nn_query", dev, q, M, order, self.sorted, self.n, self.start, self.entries, *self._grid_args(), d2,
                      dist, idx)
        return d2, dist, idx


def _nearest(query, target, want_d2=False, want_dist=True, want_index=False, max_cells=MAX_CELLS, target_box=None):
    """(d2, dist, index) of every query (None where not wanted).  One host synchronisation (the boxes) unless
    target_box is given."""
    q, t = _points("query", query), _points("target", target)
    if t.shape[0] == 0:
        raise ValueError("nearest neighbours need at least one target point")
    if q.device != t.device:
        raise ValueError(f"query on {q.device}, target on {t.device}")
    with _lib.on_device(t.device):
        if target_box is None:
            boxes = _boxes(t, q) if q.shape[0] else _boxes(t)
            target_box = boxes[0]
        return _TargetGrid(t, target_box, max_cells).query(q, want_d2, want_dist, want_index)


def nearest_distances(query, target, return_index=False):
    """Distance from every query point [M,3] to its nearest target point [N,3] (fp32 device tensors): exact, bit for
    bit sqrtf of the minimum fp32 d2 = (dx*dx + dy*dy) + dz*dz over all targets.  With return_index, also the int32
    index of that target (the smallest among equal d2).  One host synchronisation (the two sets' boxes, which also
    refuses non-finite coordinates)."""
    _, dist, idx = _nearest(query, target, want_index=return_index)
    return (dist, idx) if return_index else dist


def _mesh_on(mesh, device):
    v = mesh.vertices.detach().to(device, torch.float32).contiguous()
    f = mesh.faces.detach().to(device, torch.int32).contiguous()
    return v, f


def _sample(mesh, n_points, seed=0, device=None):
    """(points [n,3] fp32, face [n] int32) on the device."""
    if not isinstance(mesh, TriangleMesh):
        raise TypeError(f"sample_surface takes a TriangleMesh, got {type(mesh)}")
    n = int(n_points)
    if n < 0 or n >= 2 ** 31:
        raise ValueError(f"n_points must be in [0, 2^31), got {n_points}")
    dev = torch.device(device) if device is not None else mesh.vertices.device
    if dev.type != "cuda":
        raise _lib.HipLibraryError("the mesh lives on the host: sample_surface runs on the GPU only (pass device=)")
    v, f = _mesh_on(mesh, dev)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError("a mesh has vertices [V,3] and faces [F,3]")
    V, F = int(v.shape[0]), int(f.shape[0])
    if V == 0 or F == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    if seed < 0 or seed >= 2 ** 64:
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    lib = _lib.lib()
    with _lib.on_device(dev):
        nbytes = lib.sr_sample_surface_workspace_bytes(F)
        scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
        cdf = torch.empty(F, dtype=torch.float64, device=dev)
        _lib.call("sr_sample_surface_cdf", dev, v, V, f, F, cdf, scratch, nbytes)
        lo, hi, total = torch.stack([f.min().double(), f.max().double(), cdf[-1]]).cpu().tolist()   # one sync
        if lo < 0 or hi >= V:
            raise ValueError(f"sample_surface: face indices outside [0, {V}) (min {int(lo)}, max {int(hi)})")
        if not (total > 0 and np.isfinite(total)):
            raise ValueError(f"sample_surface: the mesh's total area is {total} (zero or non-finite)")
        pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
        face = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.call("sr_sample_surface", dev, v, V, f, F, cdf, n, int(seed), pts, face)
    return pts, face


def sample_surface(mesh, n_points, seed=0, device=None) -> PointCloud:
    """n_points points on the mesh surface: a face with probability proportional to its area (zero-area faces never),
    then uniform in the face, p = (1 - sqrt(u)) A + sqrt(u) (1 - v) B + sqrt(u) v C.  The generator is a counter-based
    hash of (seed, sample index) stated in the header: the same (mesh, n, seed) gives the same bits on every run.  One
    host synchronisation (face index range and total area, both checked: a zero total area raises ValueError)."""
    pts, _ = _sample(mesh, n_points, seed, device)
    return PointCloud(pts)


def _as_points(x, name, sampling, down_sample, n_points, seed, device):
    if isinstance(x, (str, bytes)) or hasattr(x, "__fspath__"):
        from .ply import read_ply
        x = read_ply(x)
    if isinstance(x, PointCloud):
        return _points(name, x.points.detach().to(device, torch.float32))
    if not isinstance(x, TriangleMesh):
        raise TypeError(f"{name} must be a TriangleMesh, a PointCloud or a PLY path, got {type(x)}")
    if sampling == "surface":
        if x.faces.shape[0] == 0:   # an empty reconstruction scores as an empty prediction
            return torch.empty((0, 3), dtype=torch.float32, device=device)
        return _sample(x, n_points, seed, device)[0]
    pts = x.vertices.detach().to(device, torch.float32).contiguous()
    if down_sample is not None and pts.shape[0]:
        pts = PointCloud(pts).voxel_down_sample(down_sample).points
    return _points(name, pts)


def mesh_metrics(pred, gt, threshold=0.05, sampling="vertices", down_sample=0.02, n_points=DEFAULT_SURFACE_POINTS,
                 seed=0, device=None):
    """Scores a reconstruction against a ground truth: {acc, comp, chamfer, precision, recall, f_score}, distances in
    metres (the reference README's tables quote cm: multiply acc, comp and chamfer by 100).

    pred, gt: each a TriangleMesh, a PointCloud or a PLY path.  A mesh becomes points by `sampling`:
      "vertices": its vertices, then PointCloud.voxel_down_sample(down_sample) (None: no downsampling) -- the vertex
                  protocol of NeuralRecon's evaluation;
      "surface":  n_points area-weighted samples with the fixed `seed` (sample_surface) -- the protocol of
                  TransformerFusion's evaluation, not bit-matched to its random samples.
    A PointCloud is used as it is.  acc = mean pred->gt distance, comp = mean gt->pred distance, chamfer = (acc +
    comp) / 2, precision / recall = the fraction of pred / gt points closer than `threshold` (strict) to the other
    set, f_score = 2PR / (P + R) (0 when P + R = 0).  An empty prediction gives recall 0, f_score 0, precision and
    acc NaN, comp and chamfer inf; an empty ground truth raises ValueError.

    Host synchronisations: the voxel downsampling's (vertex protocol), the sampler's one per mesh (surface protocol),
    one for the two boxes and the final copy of the result."""
    if sampling not in ("vertices", "surface"):
        raise ValueError(f"sampling must be 'vertices' or 'surface', got {sampling!r}")
    thr = float(threshold)
    if not (thr > 0 and np.isfinite(thr)):
        raise ValueError(f"threshold must be positive and finite, got {threshold}")
    if device is None:
        for x in (pred, gt):
            for t in (getattr(x, "points", None), getattr(x, "vertices", None)):
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    device = t.device
                    break
            if device is not None:
                break
    if device is None:
        if not _lib.cuda_available():
            raise _lib.HipLibraryError("mesh metrics run on the GPU only and no GPU is visible (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    p = _as_points(pred, "pred", sampling, down_sample, n_points, seed, device)
    g = _as_points(gt, "gt", sampling, down_sample, n_points, seed, device)
    m, n = int(p.shape[0]), int(g.shape[0])
    if n == 0:
        raise ValueError("mesh_metrics: the ground truth has no points")
    lib = _lib.lib()
    with _lib.on_device(device):
        boxes = _boxes(g, p) if m else _boxes(g)
        _, d_pg, _ = _TargetGrid(g, boxes[0]).query(p)
        d_gp = _TargetGrid(p, boxes[1]).query(g)[1] if m else None
        nbytes = lib.sr_mesh_metrics_workspace_bytes(m, n)
        scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=device)
        out = torch.empty(8, dtype=torch.float64, device=device)
        _lib.call("sr_mesh_metrics", device, d_pg, m, d_gp, n, thr, out, scratch, nbytes)
        vals = out.cpu().tolist()
    return {k: vals[i] for i, k in enumerate(METRIC_KEYS)}
