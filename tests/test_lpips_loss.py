"""LPIPS as a training loss on the CPU: the differentiable float64 composite of ``lpips.LPIPSLoss``, the closed form of the tap
backward, the scale rule, ``GanStep`` with the term on and the command line.

Bounds.  Value against ``LPIPS.composite(...).mean()``: 1e-14 relative (the same float64 arithmetic).  Gradients of two float64
evaluations of the same expression: 1e-9 * max|g| (the sums run in another order; the closed form against autograd agrees to about
1e-16 * max|g|).  ``GanStep``: the term is recomputed in float64 on the restored image the step handed over, 1e-12 relative."""
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from grl_image_restoration_amd import _lib, lpips as LP
from grl_image_restoration_amd.gan import GanStep
from tests.test_gpu_lpips import _tap_inputs
from tests.test_perceptual import NAMES, _gan_setup, disc, folders  # noqa: F401  (fixtures)

SEED = 7
NAMES_L = ["loss_g_pix", "loss_g_lpips", "loss_g_gan", "loss_d_real", "loss_d_fake", "out_d_real", "out_d_fake"]


def _pair(shape, seed=21):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g)
    return (gt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1), gt


@pytest.fixture(scope="module")
def loss():
    return LP.LPIPSLoss(LP.LPIPS(*LP.seeded_weights(SEED)))


def _written(m, x, gt):
    """The definition as written: relu, ``lpips_term`` with the plain root, the mean over the batch."""
    B = x.shape[0]
    z = torch.cat([x, gt.double()])
    z = ((2 * z - 1) - m.shift.double()) / m.scale.double()
    total, ci, tap = 0, 0, 0
    for pos, name in enumerate(LP.NAMES[: LP.TAP_INDEX[-1] + 1]):
        if name.startswith("conv"):
            z = F.conv2d(z, m.weights[ci].double(), m.biases[ci].double(), padding=1)
            ci += 1
        elif name.startswith("relu"):
            z = F.relu(z)
        else:
            z = F.max_pool2d(z, 2, 2)
        if pos == LP.TAP_INDEX[tap]:
            total = total + LP.lpips_term(z[:B], z[B:], m.lins[tap].double())
            tap += 1
    return total.mean()


@pytest.mark.parametrize("shape", [(1, 3, 16, 16), (1, 3, 35, 50)])
def test_composite_value_gradient_and_own_decisions(loss, shape):
    x, gt = _pair(shape)
    a = x.double().requires_grad_(True)
    trace = []
    v = loss.composite(a, gt, trace=trace)
    v.backward()
    want = float(loss.lpips.composite(x, gt).mean())
    v = v.detach()
    assert v.dim() == 0 and v.dtype == torch.float64 and abs(float(v) - want) <= 1e-14 * want
    assert len(trace) == 13 and float(loss(x, gt)) == float(v)         # CPU tensors: forward is the composite
    b = x.double().requires_grad_(True)
    _written(loss.lpips, b, gt).backward()
    gmax = float(b.grad.abs().max())
    err = float((a.grad - b.grad).abs().max())
    print(f"{shape}: max|g_composite - g_written| {err:.3e}, max|g| {gmax:.3e}")
    assert gmax > 0 and err <= 1e-9 * gmax
    dec = LP.decisions_from_trace(trace, shape[0])
    assert len(dec["masks"]) == 13 and len(dec["pool_idx"]) == 4
    c = x.double().requires_grad_(True)
    v2 = loss.composite(c, gt, decisions=dec)
    v2.backward()
    assert abs(float(v2.detach()) - float(v)) <= 1e-14 * want and float((c.grad - a.grad).abs().max()) <= 1e-9 * gmax
    gt_r = gt.clone().requires_grad_(True)                                      # the target and the weights get no gradient
    loss.composite(x.double().requires_grad_(True), gt_r).backward()
    assert gt_r.grad is None and all(p.grad is None for p in loss.parameters())


def test_zero_pixel_under_multiplied_masks_has_a_finite_zero_gradient():
    """An all-negative pixel at the first tap: with ReLU applied as x * mask the plain root would give sqrt'(0) * 0 = NaN there."""
    f, w = _tap_inputs(1, 64, 5, 7, seed=69)
    pre = f[:1].double().requires_grad_(True)
    mask = (pre > 0).double()
    LP._safe_term(pre * mask, F.relu(f[1:].double()), w.double()).sum().backward()
    assert bool(torch.isfinite(pre.grad).all()) and float(pre.grad[0, :, 1, 2].abs().max()) == 0.0 and float(pre.grad.abs().max()) > 0
    bad = f[:1].double().requires_grad_(True)
    LP.lpips_term(bad * mask, F.relu(f[1:].double()), w.double()).sum().backward()
    assert bool(torch.isnan(bad.grad[0, :, 1, 2]).all())                        # what the safe norm is there for


@pytest.mark.parametrize("pooled", [True, False])
@pytest.mark.parametrize("H,W", [(5, 7), (4, 4)])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_tap_backward_reference_against_autograd(C, H, W, pooled):
    B = 2
    f, w = _tap_inputs(B, C, H, W, seed=C + H)
    up = 0.37
    dpool = torch.randn(B, C, H // 2, W // 2, generator=torch.Generator().manual_seed(C), dtype=torch.float64) * 1e-3 if pooled else None
    pre = f.double().requires_grad_(True)
    r = F.relu(pre)
    total = LP.lpips_term(r[:B], r[B:], w.double()).mean() * up
    if pooled:
        total = total + (F.max_pool2d(r[:B], 2, 2) * dpool).sum()
    total.backward()
    g, A = LP.tap_backward_reference(f, w, B, up / (B * H * W), dpool)
    gmax = float(g.abs().max())
    err = float((g - pre.grad[:B]).abs().max())
    print(f"C {C} {H}x{W} dpool {pooled}: max|closed form - autograd| {err:.3e}, max|g| {gmax:.3e}")
    assert err <= 1e-12 * gmax and bool((A >= g.abs() * (1 - 1e-12)).all())
    assert float(g[0, :, 1, 2].abs().max()) == 0.0 and float(g[f[:B] <= 0].abs().max()) == 0.0
    G, Gbar = LP.tap_bound_reference(f, w, B)
    g1, _ = LP.tap_backward_reference(f, w, B, 1.0)
    assert G == float(g1.abs().max()) and Gbar >= G > 0


def test_scale_rule():
    for t in (1e-9, 3.7e-5, 0.125, 1.0, 77.0, 2.0 ** -20):
        S = LP.loss_scale([t * 0.01, t, t * 0.5])
        assert math.frexp(S)[0] == 0.5 and 2.0 ** -4 < S * t <= 2.0 ** -3, (t, S)
    for bad in ([0.0], [0.0, 0.0], [float("inf"), 1.0], [1.0, float("nan")], []):
        assert LP.loss_scale(bad) == 1.0


def test_gan_step_carries_the_term_in_order(disc, loss):
    g, d, (opt_g, opt_d), batch, kw = _gan_setup(disc)
    lq, gt, gt_usm = batch
    assert min(gt.shape[2:]) >= 16
    seen = []

    def term(y, t):
        seen.append((y.detach().clone(), t.detach().clone()))
        return loss(y, t)

    step = GanStep(g, d, opt_g, opt_d, lambda y, t: (y - t).abs().mean(), lpips=term, lpips_weight=0.25, usm_lpips=True, **kw)
    before = [p.detach().clone() for p in g.parameters()]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = step(*batch)
    assert list(out) == NAMES_L
    y, t = seen[0]
    assert torch.equal(t, gt_usm)                                               # usm_lpips: the sharpened target
    want = 0.25 * float(loss.composite(y, t))
    assert want > 0 and abs(float(out["loss_g_lpips"]) - want) <= 1e-12 * want
    assert all(p.grad is None for p in loss.parameters())
    # the term reaches the generator: without it the same step moves the weights elsewhere
    g2, d2, (o2g, o2d), _, _ = _gan_setup(disc)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plain = GanStep(g2, d2, o2g, o2d, lambda y, t: (y - t).abs().mean(), **kw)(*batch)
    assert list(plain) == NAMES and float(plain["loss_g_pix"]) == float(out["loss_g_pix"])
    moved = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(g.parameters(), g2.parameters()))
    assert moved > 0 and any(float((p.detach() - q).abs().max()) > 0 for p, q in zip(g.parameters(), before))
    with pytest.raises(ValueError, match="usm_lpips"):
        GanStep(g, d, opt_g, opt_d, lambda y, t: (y - t).abs().mean(), lpips=term, usm_lpips=True)(lq, gt)


def test_gan_step_without_the_term_returns_todays_keys(disc):
    g, d, (opt_g, opt_d), batch, kw = _gan_setup(disc)
    want = disc[1]["s__scalars"]
    step = GanStep(g, d, opt_g, opt_d, lambda y, t: (y - t).abs().mean(), lpips=None, usm_lpips=True, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = step(*batch)
    assert list(out) == NAMES
    for j, n in enumerate(NAMES):
        assert abs(float(out[n]) - want[0, j]) / abs(want[0, j]) <= 1e-8, n


GAN_ARGS = ["--task", "sr", "--scale", "2", "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--patch", "8", "--batch", "2",
            "--gan", "--disc-feat", "8", "--usm", "--device", "cpu", "--lr", "1e-3", "--seed", "3"]


def _weight_files(tmp_path):
    sd, lin = LP.seeded_weights(SEED)
    vgg, lp = tmp_path / "vgg16-397923af.pth", tmp_path / "vgg.pth"
    torch.save(sd, vgg)
    torch.save(lin, lp)
    return str(vgg), str(lp)


def test_command_line_refusals(folders, tmp_path, capsys):
    from grl_image_restoration_amd import evaluate, train

    gt, lq = folders
    vgg, lp = _weight_files(tmp_path)
    files = ["--lpips-vgg", vgg, "--lpips-lin", lp]
    data = ["--gt", gt, "--lq", lq, "--steps", "1"]
    small = [a if a != "8" or GAN_ARGS[i - 1] != "--patch" else "4" for i, a in enumerate(GAN_ARGS)]
    cases = [
        (["--task", "sr", "--scale", "2", "--device", "cpu"] + data + ["--lpips-weight", "1"] + files, "belongs to --gan"),
        (GAN_ARGS + data + ["--lpips-weight", "1", "--lpips-lin", lp], "--lpips-vgg"),
        (GAN_ARGS + data + ["--lpips-weight", "1", "--lpips-vgg", vgg], "--lpips-lin"),
        (GAN_ARGS + data + ["--lpips-weight", "0"] + files, "positive"),
        (GAN_ARGS + data + ["--lpips-weight", "-1"] + files, "positive"),
        (GAN_ARGS + data + ["--usm-lpips"], "needs --lpips-weight"),
        (small + data + ["--lpips-weight", "1"] + files, "at least 16"),
        (GAN_ARGS + data + files, "belong to --metric restorer_perceptual"),     # the files alone still belong to the metric
    ]
    for argv, word in cases:
        with pytest.raises(SystemExit) as e:
            train.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    with pytest.raises(SystemExit) as e:                                        # evaluate keeps refusing the files without the group
        evaluate.main(["--model", "small", "--geometry", "dn_df4", "--lq", lq, "--gt", gt, "--device", "cpu", "--metric", "restorer"] + files)
    assert e.value.code == 2 and "belong to --metric restorer_perceptual" in capsys.readouterr().err


def test_gan_command_line_with_the_term(folders, tmp_path):
    from grl_image_restoration_amd import train

    gt, lq = folders
    vgg, lp = _weight_files(tmp_path)
    torch.manual_seed(0)
    res = train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "1", "--lpips-weight", "0.5", "--usm-lpips", "--lpips-vgg", vgg,
                                 "--lpips-lin", lp, "--out", str(tmp_path / "run")])
    r = res["gan"][0]
    assert list(r) == NAMES_L and np.isfinite(list(r.values())).all() and r["loss_g_lpips"] > 0
    assert res["losses"][0] == pytest.approx(r["loss_g_pix"] + r["loss_g_lpips"] + r["loss_g_gan"], rel=1e-6)
    obj = torch.load(res["checkpoint"], map_location="cpu", weights_only=False)
    assert obj["args"]["lpips_weight"] == 0.5 and obj["args"]["usm_lpips"] is True
    assert all(k.startswith(("model.model_g.", "model.model_d.")) for k in obj["state_dict"])      # the frozen trunk stays out


def test_exports_and_abi():
    assert "grl_lpips_tap_bwd" in _lib.EXPORTS and "grl_lpips_prep_bwd" in _lib.EXPORTS and _lib.ABI_VERSION >= 43
