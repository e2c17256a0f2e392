"""Float64 brute-force ray caster: the yardstick of the mesh rasteriser (simplerecon_amd/render.py).  numpy only.

For every pixel ray and every triangle it solves the ray / plane hit and the barycentrics; a hit counts when
t * r_z >= znear (r_z = 1, so t is the depth along the optical axis).  Nothing is clipped or projected: a triangle
that crosses the camera plane needs no special case.

Which pixels may be compared.  A rasteriser working from fp32 data puts projected edges a small fraction of a pixel
away from where float64 puts them, so pixels on a silhouette cannot be required to agree.  Every pixel is therefore
cast five times: through its sample point and through the four diagonal offsets (+-tau, +-tau), tau = 1/32 px.  Sample
point k sees d_k, the nearest triangle covering it, with that triangle's depth always taken along the CENTRE ray (the
depth a rasteriser would write for the pixel if it drew that triangle there).  Then

    depth   = d_0       what the pixel shows
    d_loose = min_k d_k the nearest triangle covered at ANY of the five points
    d_firm  = max_k d_k the farthest of the five points' answers (no hit counts as farthest)

A pixel is contested when d_firm and d_loose differ by more than the depth tolerance, when one is a hit and the other
is not, or when a winning triangle is seen at under 3 degrees of grazing (|n . r| < 0.05 for unit n, r).

d_firm is deliberately not "the nearest triangle covered at ALL five points": inside a mesh of pixel-sized triangles
hardly any triangle covers all five points of a pixel, so that rule calls a fifth of the pixels of a smooth surface
contested, although every one of the five rays hits the surface at the same depth.  The farthest of the five answers
is never farther than the nearest triangle covering all five (such a triangle bounds every d_k), so the contested
set used here is a subset of that rule's: every pixel that rule would compare is still compared, and more."""
import numpy as np

TAU = 1.0 / 32.0
DEPTH_RTOL = 1e-4
GRAZING = 0.05
MAX_CONTESTED_SHARE = 0.03


def rays(K, H, W, pixel_offset, dx=0.0, dy=0.0):
    """[H*W,3] float64 rays K^-1 (u + pixel_offset + dx, v + pixel_offset + dy, 1), row-major over (v, u)."""
    Ki = np.linalg.inv(np.asarray(K, np.float64)[:3, :3])
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    p = np.stack([u.ravel() + pixel_offset + dx, v.ravel() + pixel_offset + dy, np.ones(H * W)], -1)
    return p @ Ki.T


def camera_triangles(verts, faces, cam_T_world):
    """The faces as camera-frame float64 corner triples [F,3,3] and the mask of usable faces (finite, non-zero area)."""
    T = np.asarray(cam_T_world, np.float64)
    with np.errstate(all="ignore"):
        vc = np.asarray(verts, np.float64) @ T[:3, :3].T + T[:3, 3]
        tri = vc[np.asarray(faces, np.int64)]
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        ok = np.isfinite(tri).all((1, 2)) & (np.linalg.norm(n, axis=1) > 0)
    return tri, ok


def _cast_points(tri, ids, r_centre, r_points, znear, chunk):
    """Per sample-point set (r_points: list of [P,3]) the nearest covering triangle, with depth along r_centre.
    Returns depth [k,P] (inf: none) and face [k,P] (-1: none)."""
    P = len(r_centre)
    best = np.full((len(r_points), P), np.inf)
    face = np.full((len(r_points), P), -1, np.int64)
    for c0 in range(0, len(tri), chunk):
        t = tri[c0:c0 + chunk]
        a, e1, e2 = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
        n = np.cross(e1, e2)
        a2, a1 = np.cross(a, e2), np.cross(e1, a)
        an = (a * n).sum(1)
        with np.errstate(all="ignore"):
            depth = an[None, :] / (r_centre @ n.T)               # [P,T] along the centre ray (r_z = 1)
            valid = depth >= znear
            for k, r in enumerate(r_points):
                d = r @ n.T
                u = -(r @ a2.T) / d
                v = -(r @ a1.T) / d
                cov = valid & (u >= 0) & (v >= 0) & (u + v <= 1)
                dk = np.where(cov, depth, np.inf)
                j = dk.argmin(1)
                m = dk[np.arange(P), j]
                better = m < best[k]
                best[k] = np.where(better, m, best[k])
                face[k] = np.where(better, ids[c0:c0 + chunk][j], face[k])
    return best, face


def cast(verts, faces, K, cam_T_world, H, W, znear=0.05, pixel_offset=0.0, tau=TAU, rtol=DEPTH_RTOL, chunk=256):
    """Casts one view.  Returns a dict of [H,W] arrays: depth (0 where nothing is hit), face (-1 where empty; the
    lowest index among the nearest), d_loose, d_firm (0 = no hit) and contested (bool)."""
    tri, ok = camera_triangles(verts, faces, cam_T_world)
    ids = np.nonzero(ok)[0]
    tri = tri[ok]
    r0 = rays(K, H, W, pixel_offset)
    pts = [r0] + [rays(K, H, W, pixel_offset, sx * tau, sy * tau) for sx in (-1, 1) for sy in (-1, 1)]
    best, face = _cast_points(tri, ids, r0, pts, znear, chunk)
    hit = np.isfinite(best)
    d_loose, d_firm = best.min(0), best.max(0)
    any_hit, all_hit = hit.any(0), hit.all(0)
    contested = any_hit != all_hit
    both = any_hit & all_hit
    with np.errstate(all="ignore"):
        contested |= both & (np.abs(d_firm - d_loose) > rtol * d_loose)
    # grazing winners (any of the five points' winners)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    nfull = np.zeros((len(faces), 3))
    nfull[ids] = n
    rhat = r0 / np.linalg.norm(r0, axis=1, keepdims=True)
    for k in range(len(pts)):
        cosang = np.abs((nfull[np.maximum(face[k], 0)] * rhat).sum(1))
        contested |= hit[k] & (cosang < GRAZING)
    z = lambda x, m: np.where(m, x, 0.0).reshape(H, W)   # noqa: E731
    return dict(depth=z(best[0], hit[0]), face=face[0].reshape(H, W), d_loose=z(d_loose, any_hit),
                d_firm=z(d_firm, all_hit), contested=contested.reshape(H, W))


def face_depths(verts, faces, K, cam_T_world, H, W, face_hw, znear=0.05, pixel_offset=0.0, tau=TAU):
    """For a face-id image (-1 = empty): the depth of the named face along each pixel's centre ray [H,W] (NaN where
    empty) and whether that face covers the pixel at any of the five sample points [H,W] bool."""
    tri, _ = camera_triangles(verts, faces, cam_T_world)
    f = np.asarray(face_hw, np.int64).ravel()
    named = f >= 0
    t = tri[np.maximum(f, 0)]
    a, e1, e2 = t[:, 0], t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    n = np.cross(e1, e2)
    a2, a1 = np.cross(a, e2), np.cross(e1, a)
    r0 = rays(K, H, W, pixel_offset)
    with np.errstate(all="ignore"):
        depth = (a * n).sum(1) / (r0 * n).sum(1)
        cov = np.zeros(len(f), bool)
        for sx, sy in ((0, 0), (-1, -1), (-1, 1), (1, -1), (1, 1)):
            r = rays(K, H, W, pixel_offset, sx * tau, sy * tau)
            d = (r * n).sum(1)
            u, v = -(r * a2).sum(1) / d, -(r * a1).sum(1) / d
            cov |= (u >= 0) & (v >= 0) & (u + v <= 1)
    return np.where(named, depth, np.nan).reshape(H, W), (cov & named & (depth >= znear)).reshape(H, W)
