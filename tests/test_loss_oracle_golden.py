"""The fp64 loss oracle (tests/loss_oracle.py) against the reference's own fp32 outputs (tests/golden/loss_<case>.npz,
written by tests/golden/make_loss_golden.py): every term, both normal maps and every gradient (CPU only)."""
import os

import numpy as np
import pytest

import loss_cases
import loss_oracle as lo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4
# the multi-view gradient carries the fp32 reference's cancellation in T_wc / P products (one pixel of near01 is off
# by 2.7e-4 of the map's largest gradient); everything else meets TOL
TOL_MV_GRAD = 5e-4


def load(name):
    g = np.load(os.path.join(GOLDEN, f"loss_{name}.npz"))
    inputs = {k: g[k] for k in g.files if not k.startswith(("term/", "grad/", "normals_"))}
    return g, inputs


@pytest.mark.parametrize("name", loss_cases.CASES)
def test_oracle_matches_reference(name):
    g, inputs = load(name)
    r = lo.run(inputs)
    for k in lo.KEYS:
        assert lo.rel_err(r["terms"][k], g[f"term/{k}"]) < TOL, (name, k, float(r["terms"][k]), float(g[f"term/{k}"]))
    for k in ("normals_gt", "normals_pred"):
        assert lo.rel_err(r[k], g[k]) < TOL, (name, k)
    keys = [k[len("grad/"):] for k in g.files if k.startswith("grad/")]
    assert set(keys) == set(r["grads"])
    for k in keys:
        tol = TOL_MV_GRAD if k.split("/")[0] in ("mv_loss", "loss") else TOL
        assert lo.rel_err(r["grads"][k], g[f"grad/{k}"]) < tol, (name, k, lo.rel_err(r["grads"][k], g[f"grad/{k}"]))


def test_cases_cover_the_edges():
    terms = {n: {k: float(np.load(os.path.join(GOLDEN, f"loss_{n}.npz"))[f"term/{k}"]) for k in lo.KEYS}
             for n in loss_cases.CASES}
    assert np.isnan(terms["blind"]["mv_loss"])              # a source that sees nothing: NaN, as the reference
    assert all(np.isfinite(terms[n]["loss"]) for n in ("holes", "odd", "room7", "s0only"))
    assert terms["s0only"]["ms_loss"] == pytest.approx(terms["s0only"]["log_l1_loss"], rel=1e-6)
    inputs = load("behind")[1]
    import torch
    k = 1
    _, _, zp = lo.mv_project(torch.as_tensor(inputs["depth_pred_s0_b1hw"]).double(), torch.as_tensor(inputs["invK_s0_b44"]),
                             torch.as_tensor(inputs["world_T_cam_b44"]), torch.as_tensor(inputs["src_K_s0_bk44"])[:, k],
                             torch.as_tensor(inputs["src_cam_T_world_bk44"])[:, k])
    assert (zp <= 0).any()
    near = inputs["depth_pred_s0_b1hw"]
    near01 = load("near01")[1]["depth_pred_s0_b1hw"]
    assert ((near01 > 0.1) & (near01 < 0.12)).any() and (near01 <= 0.1).any()
    assert near.shape[-2:] == (48, 64)
