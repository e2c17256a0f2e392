"""Seeded point-cloud fusion cases shared by tests/golden/make_pc_golden.py and the tests: the inputs are regenerated
from these seeds (simplerecon_amd.synthetic.raycast_scene on the CPU), only the reference's outputs are stored."""
from simplerecon_amd import synthetic

# name -> (raycast_scene arguments, z_thresh, n_consistent_thresh)
CASES = {
    "small": (dict(N=6, h=60, w=80, seed=1), 0.04, 3),
    "holes": (dict(N=8, h=60, w=80, seed=2, noise=0.002, holes=0.01), 0.04, 3),
    "thresh1": (dict(N=6, h=60, w=80, seed=3, noise=0.004), 0.04, 1),
}


def scene(name):
    args, zt, nt = CASES[name]
    return synthetic.raycast_scene(**args), zt, nt
