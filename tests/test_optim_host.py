"""Host side of the optimiser step (simplerecon_amd.optim, simplerecon_amd.training): the LR schedule, the chunk plan of the
streaming launch and every refusal.  Runs without a GPU."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

from simplerecon_amd import depth_model as dm
from simplerecon_amd import optim, training
from simplerecon_amd._lib import HipLibraryError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lr_factor_equals_the_reference_schedule():
    """The reference's lambda (experiment_modules/depth_model.py:624-630, restated) driven through LambdaLR on a CPU torch
    optimiser, at both edges of both steps."""
    lr_steps, base = (70000, 80000), 1e-4

    def lr_lambda(step):
        if step < lr_steps[0]:
            return 1
        elif step < lr_steps[1]:
            return .1
        else:
            return .01
    opt = torch.optim.AdamW([torch.zeros(1, requires_grad=True)], lr=base)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda)
    assert dm.default_options().lr_steps == lr_steps and training.DEFAULT_LR_STEPS == lr_steps
    assert dm.default_options().lr == base and dm.default_options().wd == 1e-4
    for step, want in ((0, 1), (69999, 1), (70000, .1), (79999, .1), (80000, .01)):
        sched.last_epoch = step - 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")     # (no optimizer.step() in between: only the schedule is looked at)
            sched.step()
        assert sched.last_epoch == step
        assert training.lr_factor(step, lr_steps) == want
        assert opt.param_groups[0]["lr"] == base * training.lr_factor(step, lr_steps)
    assert training.lr_factor(5, (5, 9)) == 0.1 and training.lr_factor(9, (5, 9)) == 0.01


def test_chunk_plan_covers_every_element_once():
    header = open(os.path.join(ROOT, "include", "simplerecon_hip.h")).read()
    chunk = int(re.search(r"#define SR_ADAMW_CHUNK (\d+)", header).group(1))
    assert chunk == optim.CHUNK and int(re.search(r"#define SR_ADAMW_MAX_GROUPS (\d+)", header).group(1)) == optim.MAX_GROUPS
    sizes = [0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 3 * chunk + 2]
    for numels in (sizes, sizes[::-1], [0, 0, 7, 0], [chunk], [0, chunk + 1, 0]):
        starts = optim.chunk_plan(numels, chunk)
        assert len(starts) == len(numels) + 1 and starts[0] == 0
        assert starts[-1] == sum(-(-n // chunk) for n in numels)
        seen = [np.zeros(n, dtype=np.int32) for n in numels]
        for c in range(starts[-1]):
            t, off, cnt = optim.chunk_of(starts, c, numels, chunk)
            assert 0 < cnt <= chunk and off % chunk == 0 and off + cnt <= numels[t]
            seen[t][off:off + cnt] += 1
        assert all(bool((s == 1).all()) for s in seen)


def _param(*shape, dtype=torch.float32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device, requires_grad=True)


@pytest.mark.parametrize("flag", ["amsgrad", "maximize", "differentiable", "capturable", "foreach", "fused"])
def test_unsupported_variants_are_refused(flag):
    with pytest.raises(NotImplementedError):
        optim.AdamW([_param(4)], **{flag: True})


def test_parameters_the_step_cannot_take_are_refused():
    with pytest.raises(HipLibraryError):                       # CPU tensors: no fallback
        optim.AdamW([_param(4)])
    with pytest.raises(HipLibraryError):
        dm.DepthModel(dm.default_options(image_width=128, image_height=96, model_num_views=3,
                                         matching_num_depth_bins=8)).configure_optimizers()
    with pytest.raises(TypeError):
        optim.AdamW([_param(4, dtype=torch.float16)])
    with pytest.raises(TypeError):
        optim.AdamW([_param(4, dtype=torch.float64)])
    with pytest.raises(ValueError):                            # not contiguous
        optim.AdamW([torch.zeros(4, 6).t().requires_grad_()])
    with pytest.raises(ValueError, match="more than one device"):
        optim.AdamW([_param(4), _param(4, device="meta")])
    with pytest.raises(ValueError):
        optim.AdamW([_param(4)], lr=-1.0)
    with pytest.raises(ValueError):
        optim.AdamW([_param(4)], betas=(0.9, 1.0))


def test_gradients_the_step_cannot_take_are_refused():
    dev = torch.device("cpu")
    p = _param(4, 6)
    optim._refuse_grad(torch.zeros(4, 6), p, dev)              # a good one passes
    with pytest.raises(RuntimeError, match="sparse"):
        optim._refuse_grad(torch.zeros(4, 6).to_sparse(), p, dev)
    with pytest.raises(TypeError):
        optim._refuse_grad(torch.zeros(4, 6, dtype=torch.float16), p, dev)
    with pytest.raises(TypeError):
        optim._refuse_grad(torch.zeros(6, 4).t(), p, dev)      # not contiguous
    with pytest.raises(TypeError):
        optim._refuse_grad(torch.zeros(4, 6, device="meta"), p, dev)


def test_train_step_argument_rules():
    with pytest.raises(ValueError):
        training.train_step(None, None, None, mfma16=2)
    assert training.fit(None, iter(()), 0, optimizer=object()) == 0
