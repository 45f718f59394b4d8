"""``GanStep`` on the GPU: two iterations of the alternation (engines/base_gan.py:86-147) with a tiny generator (GRL-Tiny cut to
depths [1], windows 8 x 8, scale 2, a 16 x 16 LQ, batch 2) and the num_feat-8 discriminator of tests/golden/gan/disc.npz, against the
same two iterations through the CPU composite in float64 with ``torch.optim.Adam`` (the reference's optimizer).

Tolerance: 5e-4 absolute on every logged scalar -- what tests/test_gpu_train_step.py::
test_training_gradients_other_geometries_vs_oracle_autograd allows between the GPU's loss and the CPU oracle's.
"""
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["loss_g_pix", "loss_g_gan", "loss_d_real", "loss_d_fake", "out_d_real", "out_d_fake"]
TOL = 5e-4
LR = 2e-4


def _build(device, dtype):
    from grl_image_restoration_amd import GRL
    from grl_image_restoration_amd.discriminator import UNetDiscriminatorSN
    from oracle import grl_oracle as O

    z = np.load(os.path.join(HERE, "golden", "gan", "disc.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    g = GRL(**dict(meta["g_cfg"], img_size=16))
    g.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in g.state_dict().items()}, meta["g_weight_seed"]), strict=True)
    d = UNetDiscriminatorSN(3, 8, True)
    sd = {k[len("d__p__"):]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("d__p__")}
    for i in range(1, 9):
        sd[f"conv{i}.weight_u"], sd[f"conv{i}.weight_v"] = torch.from_numpy(z[f"d__u0__conv{i}"]), torch.from_numpy(z[f"d__v0__conv{i}"])
    d.load_state_dict(sd, strict=True)
    return g.to(device=device, dtype=dtype).train(), d.to(device=device, dtype=dtype).train()


def _run(device, dtype, make_opt):
    from grl_image_restoration_amd.gan import GanStep

    g, d = _build(device, dtype)
    opt_g, opt_d = make_opt(g.parameters()), make_opt(d.parameters())
    seen = []
    step_g = opt_g.step

    def checked_step(*a, **kw):
        seen.append(all(p.grad is None for p in d.parameters()))
        return step_g(*a, **kw)

    opt_g.step = checked_step
    step = GanStep(g, d, opt_g, opt_d, lambda y, t: (y - t).abs().mean(), usm_pixel=True, usm_gan=False)
    gen = torch.Generator().manual_seed(5)
    lq, gt, gt_usm = torch.rand(2, 3, 16, 16, generator=gen), torch.rand(2, 3, 32, 32, generator=gen), torch.rand(2, 3, 32, 32, generator=gen)
    rows = []
    for _ in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = step(*(t.to(device=device, dtype=dtype) for t in (lq, gt, gt_usm)))
        rows.append([float(out[n]) for n in NAMES])
    del opt_g.step                                    # (the wrapper refers to the optimizer: no cycle may keep the networks alive)
    assert seen == [True, True]                       # no discriminator gradient at the generator's step
    return rows, d


def test_gan_step_matches_the_cpu_composite():
    from grl_image_restoration_amd import FusedAdamW

    want, d_cpu = _run("cpu", torch.float64, lambda p: torch.optim.Adam(p, lr=LR))
    got, d_gpu = _run("cuda", torch.float32, lambda p: FusedAdamW(p, lr=LR, weight_decay=0))
    for it in range(2):
        for j, n in enumerate(NAMES):
            print(f"iteration {it} {n}: gpu {got[it][j]:.7f} cpu {want[it][j]:.7f} |d| {abs(got[it][j] - want[it][j]):.2e}")
    worst = max(abs(got[it][j] - want[it][j]) for it in range(2) for j in range(6))
    assert worst <= TOL, worst
    z = np.load(os.path.join(HERE, "golden", "gan", "disc.npz"), allow_pickle=False)
    for i in range(1, 9):                             # the power iteration ran on the device's buffers
        u = getattr(d_gpu, f"conv{i}").weight_u
        assert u.is_cuda and not torch.equal(u.cpu().double(), torch.from_numpy(z[f"d__u0__conv{i}"]))
