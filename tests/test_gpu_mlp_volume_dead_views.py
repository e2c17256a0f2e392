"""The metadata-MLP sweep skips, per (64-pixel wave, plane), the feature k-steps, tap loads and interpolation of every
source view none of whose taps lies inside the source image ("dead" view).  These cases build poses by hand so that every
combination of dead and live views occurs, prove on the CPU (numpy, the projection of csrc/sr_common.h in fp64) that it
does, and only then compare the GPU volume with the CPU oracle: same bounds as test_gpu_mlp_volume.py."""
import numpy as np
import pytest
import torch

import oracle
from parity import assert_close, mismatch_fraction
from simplerecon_amd import synthetic
from simplerecon_amd.cost_volume import FeatureVolumeManager

DEV = "cuda:0"
B, C, D = 2, 16, 9            # D = 9: one full 8-plane unit and one partial one
MAPS = [(8, 32), (10, 12)]    # 4 waves of two whole rows each; 120 pixels = one full wave and a ragged one (56 lanes)
PLANES = np.geomspace(0.25, 5.0, D)
MARGIN = 1e-3                 # texels between any sampling position and the edge of the region that has a tap


def _translation(tx, ty, tz=0.0):
    T = np.eye(4)
    T[:3, 3] = (tx, ty, tz)
    return T


def _view(kind, f, h, w, i):
    """src_cam_T_cur_cam of one view.  With R = I and t = (tx, ty, 0) a plane at depth d samples at (x + f tx / d,
    y + f ty / d): shifts below are texels at d = 1.  `i` makes views of one kind differ a little."""
    e = 0.013 * i
    if kind == "a":   # near identity: every pixel has a tap at every plane (shift <= 0.8 texel at d = 0.25)
        return _translation((0.11 + e) / f, (-0.13 + e) / f)
    if kind == "b":   # large lateral offset: >= 6 w + 1 texels at the far plane: every wave dead at every plane
        return _translation((30.3 * w + 7 * i) / f, 0.0)
    if kind == "c":   # lateral shift of 1.43 w texels at d = 1: dead at the near planes, live at the far ones
        return _translation((1.43 * w + e) / f, 0.0)
    if kind == "d":   # shift upwards, about -3.6 rows at plane 4: top rows without a tap, bottom rows with one
        return _translation(0.0, (-3.63 * PLANES[4] - e) / f)
    if kind == "e":   # behind the camera (z' = -d <= 0, mask 0), looking back: the mirrored taps are inside the image
        T = np.diag([-1.0, 1.0, -1.0, 1.0])   # rotation by pi about y
        T[:3, 3] = ((0.17 + e) / f, 0.11 / f, 0.0)
        return T
    raise KeyError(kind)


# one string per batch element, one letter per view
CASES = {
    "k7_dead_first_last__two_consecutive": ("bacdeab", "abbacde"),
    "k7_alternating__all_dead": ("ebabdba", "bbbbbbb"),
    "k7_none_dead__dead_first_last": ("aaeaaaa", "bdacbeb"),
    "k3_dead_first_last__mixed": ("bcb", "dea"),
    "k3_all_dead__none_dead": ("bbb", "aed"),
}


def _inputs(views, h, w, seed):
    K = len(views[0])
    f = 0.625 * w
    Kmat = np.eye(4)
    Kmat[0, 0] = Kmat[1, 1] = f
    Kmat[0, 2], Kmat[1, 2] = w / 2.0, h / 2.0
    extr = np.stack([np.stack([_view(kind, f, h, w, i) for i, kind in enumerate(v)]) for v in views])
    rng = np.random.default_rng(seed)
    planes = np.broadcast_to(PLANES.astype(np.float32)[None, :, None, None], (B, D, h, w)).copy()
    return dict(
        cur_feats=torch.from_numpy(rng.standard_normal((B, C, h, w), dtype=np.float32)),
        src_feats=torch.from_numpy(rng.standard_normal((B, K, C, h, w), dtype=np.float32)),
        src_extrinsics=torch.from_numpy(extr.astype(np.float32)),
        src_poses=torch.from_numpy(np.linalg.inv(extr).astype(np.float32)),
        src_Ks=torch.from_numpy(np.broadcast_to(Kmat.astype(np.float32), (B, K, 4, 4)).copy()),
        cur_invK=torch.from_numpy(np.broadcast_to(np.linalg.inv(Kmat).astype(np.float32), (B, 4, 4)).copy()),
        min_depth=torch.tensor(synthetic.MIN_DEPTH).view(1, 1, 1, 1),
        max_depth=torch.tensor(synthetic.MAX_DEPTH).view(1, 1, 1, 1),
        depth_planes_bdhw=torch.from_numpy(planes),
    )


def wave_states(inp):
    """Per (batch, wave, plane, view): 0 = no pixel of the wave has a tap in the image (dead), 2 = every pixel has one,
    1 = mixed; also whether some pixel with z' <= 0 has a tap, and the smallest distance (texels) of any sampling
    position from the edge of the region that has a tap.  fp64 from the fp32 inputs, the steps of sr_project_sample_xy
    and sr_bilinear_taps: a tap (x0 or x0 + 1, y0 or y0 + 1) is inside iff -1 <= ix < w and -1 <= iy < h."""
    n = {k: v.numpy().astype(np.float64) for k, v in inp.items()}
    _, K, _, h, w = n["src_feats"].shape
    N = h * w
    ys, xs = np.divmod(np.arange(N), w)
    pix = np.stack([xs + 0.5, ys + 0.5, np.ones(N)])                      # [3, N]
    waves = (N + 63) // 64
    state = np.zeros((B, waves, D, K), dtype=np.int64)
    behind_with_tap, margin = False, np.inf
    for b in range(B):
        rays = n["cur_invK"][b, :3, :3] @ pix
        for k in range(K):
            P = (n["src_Ks"][b, k] @ n["src_extrinsics"][b, k])[:3]
            for j in range(D):
                X = n["depth_planes_bdhw"][b, j].reshape(N) * rays
                q = P[:, :3] @ X + P[:, 3:4]
                zp = q[2] + 1e-8
                sc = np.where(np.abs(q[2]) > 1e-8, 1.0 / zp, 1.0)
                ix = ((2.0 * q[0] * sc / w - 1.0 + 1.0) * w - 1.0) / 2.0
                iy = ((2.0 * q[1] * sc / h - 1.0 + 1.0) * h - 1.0) / 2.0
                inside = np.minimum(np.minimum(ix + 1.0, w - ix), np.minimum(iy + 1.0, h - iy))
                # inside > 0: has a tap, and `inside` is the distance to the edge; inside <= 0: none, -inside is a
                # lower bound of the distance (Chebyshev) to the region
                tap = inside > 0.0
                margin = min(margin, float(np.abs(inside).min()))
                behind_with_tap |= bool((tap & (zp <= 0.0)).any())
                for t in range(waves):
                    lanes = tap[t * 64:min(N, t * 64 + 64)]           # lanes past the image (pix >= N) do not vote
                    state[b, t, j, k] = 0 if not lanes.any() else (2 if lanes.all() else 1)
    return state, behind_with_tap, margin


def check_patterns(name, views, state, behind_with_tap, margin):
    """What the case was built for really occurs, and robustly so in fp32."""
    assert margin > MARGIN, f"{name}: a sampling position lies {margin:.2e} texel from the tap-validity boundary"
    assert (state == 0).any() and (state == 2).any() and (state == 1).any(), f"{name}: dead / live / mixed waves"
    assert behind_with_tap, f"{name}: no pixel behind the camera with a tap inside the image"
    for b, v in enumerate(views):
        for k, kind in enumerate(v):
            s = state[b, :, :, k]
            if kind == "a":
                assert (s == 2).all(), f"{name}: view {k} of frame {b} is not live everywhere"
            if kind == "b":
                assert (s == 0).all(), f"{name}: view {k} of frame {b} is not dead everywhere"
            if kind == "c":   # dead near, live far, inside the first 8-plane unit
                assert (s[:, 0] == 0).all() and (s[:, 7] > 0).all(), f"{name}: view {k} of frame {b}: near / far"
            if kind == "d":   # at one plane: a dead wave above a live one
                assert ((s[0] == 0) & (s[-1] > 0)).any(), f"{name}: view {k} of frame {b}: top dead, bottom live"
            if kind == "e":
                assert (s > 0).all(), f"{name}: view {k} of frame {b}: behind the camera, but live"
    dead = state == 0                                                    # [B, waves, D, K]
    if any(v[0] == "b" for v in views):
        assert dead[..., 0].any(), f"{name}: dead view 0"
    if any(v[-1] == "b" for v in views):
        assert dead[..., -1].any(), f"{name}: dead last view"
    if any("bb" in v for v in views):
        assert (dead[..., 1:] & dead[..., :-1]).any(), f"{name}: two consecutive dead views"
    if any(set(v) == {"b"} for v in views):
        assert dead.all(-1).any(), f"{name}: all views dead"
    if any(set(v) <= {"a", "e"} for v in views):
        assert (~dead).all(-1).all(1).all(1).any(), f"{name}: a frame with no dead view anywhere"


def _manager(K, h, w, seed):
    mgr = FeatureVolumeManager(h, w, num_depth_bins=D, matching_dim_size=C, num_source_views=K)
    synthetic.seeded_fill_(mgr.mlp, seed=seed)
    return mgr.to(DEV)


def _run(mgr, inp):
    with torch.inference_mode():
        out = mgr(return_mask=True, **{k: v.to(DEV) for k, v in inp.items()})
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("hw", MAPS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("name", list(CASES))
def test_dead_views_match_oracle(name, hw):
    h, w = hw
    views = CASES[name]
    K = len(views[0])
    inp = _inputs(views, h, w, seed=300 + K + h)
    check_patterns(name, views, *wave_states(inp))                       # before any GPU output is looked at

    mgr = _manager(K, h, w, seed=40 + K)
    vol, lowest, planes, mask = _run(mgr, inp)
    n = {k: v.numpy() for k, v in inp.items()}
    sd = {k: v.cpu().numpy() for k, v in mgr.mlp.state_dict().items()}
    mlp = dict(W1=sd["net.0.weight"], b1=sd["net.0.bias"], W2=sd["net.2.weight"], b2=sd["net.2.bias"],
               W3=sd["net.4.weight"], b3=sd["net.4.bias"])
    planes_np = np.broadcast_to(PLANES.astype(np.float32), (B, D)).copy()
    cv_o, _, mask_o = oracle.mlp_volume(n["cur_feats"], n["src_feats"], n["src_Ks"], n["src_extrinsics"], n["src_poses"],
                                        n["cur_invK"], planes_np, mlp, want_mask=True)
    assert_close(vol, cv_o, tol=2e-5, what=f"{name} {h}x{w} vs oracle")
    assert mismatch_fraction(mask, mask_o) == 0.0

    # the channels-last volume is the same volume
    mgr.volume_memory_format = torch.channels_last
    vol_cl = _run(mgr, inp)[0]
    assert vol_cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(vol_cl.contiguous(), vol)
    # frames of a batch are independent
    mgr.volume_memory_format = torch.contiguous_format
    one = {k: (v[1:2].contiguous() if v.dim() > 0 and v.shape[0] == B else v) for k, v in inp.items()}
    assert torch.equal(_run(mgr, one)[0][0], vol[1])
