"""LPIPS as a training loss on the GPU (csrc/lpips.hip, lpips.LPIPSLoss): the tap backward and the gradient bound against the float64
closed form on the same fp32 values, the prep backward against autograd, the whole chain's gradient against the float64 CPU
composite, the measured scale S, and ``GanStep`` with the term on.

Bounds.
  Tap backward, elementwise: |d / S - g_64| <= 4 * (C + 8) * 2^-24 * A, A = ``lpips.tap_backward_reference``'s second result: the
    closed form with every term replaced by its absolute value (ebar_c = 2 |w_c| (u0_c + u1_c)) plus |routed pool gradient| -- the
    first-order bound of an fp32 evaluation whose sums have at most C + 8 terms, the rule of tests/test_gpu_lpips.py.  Masked entries
    and the zero-norm pixel: exactly 0.  G_l: |G - G_64| <= 4 * (C + 8) * 2^-24 * Gbar, Gbar the maximum of the same absolute-value
    expression.
  Prep backward: relative error <= 8 * 2^-24 against autograd (the rule of grl_vgg_prep_bwd's test).
  Chain: under the GPU run's ReLU / pool decisions, max|g_gpu - g_64| <= 4 * max|g_emu - g_64|, the emulation with fp16 operands and
    dy rounded to fp16 under the run's own S (the rule of tests/test_gpu_perceptual.py).
  GanStep: |loss_g_lpips - float64 composite on the GPU run's restored image| <= 4 * 1.46e-4 relative (RECORDED_E of
    tests/test_gpu_lpips.py); the six other scalars within that set-up's 5e-4 of the float64 CPU run.

Measured on an MI355X, 2026-10-20 (the tests print every figure next to its bound):
  tap backward, largest elementwise error / bound: 1.13e-02 (C 64), 6.1e-03 (128), 3.9e-03 (256), 2.0e-03 (512), the same with and
    without dpool and at 5 x 7 and 4 x 4; G_l |d| 4.6e-14 .. 2.0e-10 against bounds of 1.3e-08 .. 1.2e-07; prep backward 0
  chain gradient, max|g_gpu - g_64| (bound 4 x max|g_emu - g_64|); max|g|; emulation / max|g|; S
    (2, 3, 32, 32)   4.77e-08 (1.80e-07)   2.32e-05   1.94e-03   2^16
    (1, 3, 35, 50)   5.98e-08 (2.19e-07)   2.95e-05   1.85e-03   2^16
    (1, 3, 16, 16)   2.34e-07 (9.10e-07)   1.55e-04   1.47e-03   2^12
  upstream 1e-6 on (2, 3, 32, 32): S = 2^36, max|g / u - g_1| 5.35e-09 (bound 1.80e-07)
  GanStep: loss_g_lpips 1.35e-06 relative (bound 5.84e-04); loss_g_pix 5.4e-07, loss_g_gan 2.0e-07, loss_d_real 1.6e-07, loss_d_fake
    2.8e-06, out_d_real 3.3e-07, out_d_fake 5.4e-06 against the float64 CPU run (bound 5e-04 each)
"""
import warnings

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import lpips as LP
from tests.test_gpu_lpips import RECORDED_E, SHAPES, _img, _tap_inputs, _tok
from tests.test_gpu_perceptual import LR, TOL, _build, _pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
SEED = 7
NAMES_L = ["loss_g_pix", "loss_g_lpips", "loss_g_gan", "loss_d_real", "loss_d_fake", "out_d_real", "out_d_fake"]


# ---- the tap backward alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", [True, False])
@pytest.mark.parametrize("H,W", [(5, 7), (4, 4)])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_tap_backward_against_the_float64_closed_form(C, H, W, pooled):
    from grl_image_restoration_amd import ops

    B, S, up = 2, 2.0 ** 10, 0.37
    f, w = _tap_inputs(B, C, H, W, seed=C + H)
    k = up / (B * H * W)
    dp = torch.randn(B, C, H // 2, W // 2, generator=torch.Generator().manual_seed(C + 1)) if pooled else None     # carries S already
    tok, wd = _tok(f).to(DEV), w.to(DEV)
    dpd = _tok(dp).to(DEV) if pooled else None
    d = ops.lpips_tap_bwd(tok, wd, B, H, W, S * k, dpd)
    assert d.dtype == torch.float32 and tuple(d.shape) == (B * H * W, C)
    got = _img(d, B, H, W).cpu().double() / S
    g64, A = LP.tap_backward_reference(f, w, B, k, dp.double() / S if pooled else None)
    ratio = float(((got - g64).abs() / (4 * (C + 8) * EPS * A).clamp_min(1e-300)).max())
    print(f"C {C} {H}x{W} dpool {pooled}: max|d/S - g_64| {float((got - g64).abs().max()):.3e}, max|g| {float(g64.abs().max()):.3e}, "
          f"largest error / bound {ratio:.3e} (must be <= 1)")
    assert bool(((got - g64).abs() <= 4 * (C + 8) * EPS * A).all()), ratio
    assert float(got[f[:B] <= 0].abs().max()) == 0.0 and float(got[0, :, 1, 2].abs().max()) == 0.0 and float(got.abs().max()) > 0
    if pooled and (H % 2 or W % 2):                                             # pixels MaxPool's floor drops: the tap term alone
        alone, _ = LP.tap_backward_reference(f, w, B, k, None)
        edge = torch.zeros(H, W, dtype=torch.bool)
        edge[2 * (H // 2):, :] = True
        edge[:, 2 * (W // 2):] = True
        assert bool(((got - alone).abs()[:, :, edge] <= (4 * (C + 8) * EPS * A)[:, :, edge]).all())
    assert torch.equal(d, ops.lpips_tap_bwd(tok, wd, B, H, W, S * k, dpd))      # the same bits on every run


@pytest.mark.parametrize("H,W", [(5, 7), (4, 4)])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_gradient_bound_and_the_forward_it_rides_in(C, H, W):
    from grl_image_restoration_amd import ops

    B = 2
    f, w = _tap_inputs(B, C, H, W, seed=C + H)
    tok, wd = _tok(f).to(DEV), w.to(DEV)
    plain, train = torch.zeros(B, dtype=torch.float64, device=DEV), torch.zeros(B, dtype=torch.float64, device=DEV)
    gmax = torch.full((1,), -1.0, device=DEV)
    p0 = ops.lpips_tap(tok, wd, B, H, W, plain, accumulate=False)
    p1 = ops.lpips_tap(tok, wd, B, H, W, train, accumulate=False, gmax=gmax)
    assert torch.equal(plain, train) and torch.equal(p0, p1)                    # the training instantiation: the same forward bits
    G, Gbar = LP.tap_bound_reference(f, w, B)
    err, bound = abs(float(gmax) - G), 4 * (C + 8) * EPS * Gbar
    print(f"C {C} {H}x{W}: G gpu {float(gmax):.9e} f64 {G:.9e} |d| {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)
    again = torch.full((1,), -1.0, device=DEV)
    ops.lpips_tap(tok, wd, B, H, W, train, accumulate=False, gmax=again)
    assert torch.equal(gmax, again)


def test_tap_backward_refuses_what_it_does_not_cover():
    from grl_image_restoration_amd import ops

    with pytest.raises(RuntimeError, match="unsupported"):
        ops.lpips_tap_bwd(torch.zeros(2 * 16, 96, device=DEV), torch.zeros(96, device=DEV), 1, 4, 4, 1.0)


# ---- prep backward -------------------------------------------------------------------------------------------------------------------
def test_prep_backward_against_autograd():
    from grl_image_restoration_amd import ops

    g = torch.Generator().manual_seed(4)
    B, H, W = 2, 18, 14
    x = torch.rand(B, 3, H, W, generator=g).to(DEV).requires_grad_(True)
    shift = torch.Tensor(LP.SHIFT).view(1, 3, 1, 1).to(DEV)
    scale = torch.Tensor(LP.SCALE).view(1, 3, 1, 1).to(DEV)
    dt = torch.randn(B * H * W, 4, generator=g).to(DEV)
    (want,) = torch.autograd.grad(((((2 * x - 1) - shift) / scale) * _img(dt[:, :3], B, H, W)).sum(), x)
    got = ops.lpips_prep_bwd(dt, B, H, W, scale=2.0 ** -5) * 2.0 ** 5
    err = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
    print(f"prep backward: max relative error {err:.3e} (bound {8 * EPS:.3e})")
    assert tuple(got.shape) == (B, 3, H, W) and err <= 8 * EPS


# ---- the whole chain -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def losses():
    sd, lin = LP.seeded_weights(SEED)
    return LP.LPIPSLoss(LP.LPIPS(sd, lin)).to(DEV), LP.LPIPSLoss(LP.LPIPS(sd, lin))


def _gpu_grad(mod, x, gt, upstream=1.0):
    xg, gg = x.to(DEV).requires_grad_(True), gt.to(DEV).requires_grad_(True)
    loss, taps, layers = mod.forward_traced(xg, gg)
    (loss * upstream).backward()
    assert gg.grad is None and all(p.grad is None for p in mod.parameters())    # frozen trunk, detached target
    return loss.detach(), taps, layers, xg.grad.detach().cpu().double()


@pytest.fixture(scope="module")
def chain(losses):
    """chain(shape): one GPU run of a shape and its CPU yardsticks under that run's decisions, computed once and shared."""
    gpu, cpu = losses
    cache = {}

    def get(shape):
        if shape not in cache:
            x, gt = _pair(shape)
            loss, taps, layers, g_gpu = _gpu_grad(gpu, x, gt)
            S, bounds = gpu.last_scale, list(gpu.last_bounds)
            dec = LP.decisions_from_trace(layers, shape[0])
            grads = []
            for kw in (dict(), dict(operand_dtype=torch.float16, grad_scale=S)):
                a = x.double().requires_grad_(True)
                cpu.composite(a, gt, decisions=dec, **kw).backward()
                grads.append(a.grad)
            cache[shape] = dict(x=x, gt=gt, loss=loss, taps=taps, layers=layers, g_gpu=g_gpu, S=S, bounds=bounds, g64=grads[0], gemu=grads[1])
        return cache[shape]

    yield get
    cache.clear()


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_loss_is_the_metrics_mean_and_the_scale_is_the_rule(losses, chain, shape):
    gpu, _ = losses
    c = chain(shape)
    B, _, H, W = shape
    with torch.no_grad():
        metric = gpu.lpips(c["x"].to(DEV), c["gt"].to(DEV))
        again = gpu(c["x"].to(DEV), c["gt"].to(DEV))
    assert c["loss"].dtype == torch.float32 and c["loss"].dim() == 0
    assert torch.equal(c["loss"], metric.mean().float()) and torch.equal(again, c["loss"])
    assert len(c["taps"]) == 5 and len(c["layers"]) == 13 and tuple(c["taps"][0].shape) == (2 * B, 64, H, W)
    ks = [1.0 / (B * (H >> l) * (W >> l)) for l in range(5)]
    T = max(k * g for k, g in zip(ks, c["bounds"]))
    print(f"{shape}: G_l {[f'{g:.3e}' for g in c['bounds']]}, T {T:.3e}, S = 2^{int(np.log2(c['S']))}, S * T {c['S'] * T:.4f}")
    assert c["S"] == LP.loss_scale([k * g for k, g in zip(ks, c["bounds"])]) and 2.0 ** -4 < c["S"] * T <= 2.0 ** -3


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_gradient_under_the_gpu_runs_decisions(chain, shape):
    c = chain(shape)
    gmax = float(c["g64"].abs().max())
    err, emu = float((c["g_gpu"] - c["g64"]).abs().max()), float((c["gemu"] - c["g64"]).abs().max())
    print(f"{shape} dL/dx: max|g_gpu - g_64| {err:.3e} (bound 4 x {emu:.3e} = {4 * emu:.3e}); max|g| {gmax:.3e}; emulation / max|g| {emu / gmax:.2e}; "
          f"S = 2^{int(np.log2(c['S']))}")
    assert gmax > 0 and err <= 4 * emu, (err, 4 * emu)


def test_chain_is_bit_identical_and_rescales_a_small_upstream(losses, chain):
    gpu, _ = losses
    c = chain(SHAPES[0])
    loss, _, _, g = _gpu_grad(gpu, c["x"], c["gt"])
    assert torch.equal(loss, c["loss"]) and torch.equal(g, c["g_gpu"]) and gpu.last_scale == c["S"]
    _, _, _, small = _gpu_grad(gpu, c["x"], c["gt"], upstream=1e-6)
    small = small / 1e-6
    emu = float((c["gemu"] - c["g64"]).abs().max())
    err = float((small - c["g_gpu"]).abs().max())
    print(f"upstream 1e-6: S = 2^{int(np.log2(gpu.last_scale))} (upstream 1: 2^{int(np.log2(c['S']))}); max|g / u - g_1| {err:.3e} "
          f"(bound {4 * emu:.3e}); max|g| {float(small.abs().max()):.3e}")
    assert gpu.last_scale >= 500 * c["S"] and float(small.abs().max()) > 0 and err <= 4 * emu, (err, 4 * emu)


def test_nothing_is_kept_without_a_gradient(losses):
    gpu, _ = losses
    x, gt = _pair(SHAPES[2])
    v = gpu(x.to(DEV), gt.to(DEV))
    assert v.grad_fn is None and not v.requires_grad
    with torch.no_grad():
        w = gpu(x.to(DEV).requires_grad_(True), gt.to(DEV))
    assert w.grad_fn is None and torch.equal(v, w)


# ---- GanStep -------------------------------------------------------------------------------------------------------------------------
def test_gan_step_with_the_lpips_term(losses):
    """One iteration at the tiny-generator set-up of tests/test_gpu_gan.py, on the GPU and on the CPU in float64.  ``loss_g_lpips`` is
    held against the float64 composite on the very restored image the GPU run handed to the loss; the six other scalars keep that
    set-up's bound against the CPU run."""
    from grl_image_restoration_amd import FusedAdamW
    from grl_image_restoration_amd.gan import GanStep

    gen = torch.Generator().manual_seed(5)
    lq, gt, gt_usm = torch.rand(2, 3, 16, 16, generator=gen), torch.rand(2, 3, 32, 32, generator=gen), torch.rand(2, 3, 32, 32, generator=gen)
    rows, seen = {}, {}
    for device, dtype, make_opt, mod in (("cpu", torch.float64, lambda p: torch.optim.Adam(p, lr=LR), losses[1]),
                                         ("cuda", torch.float32, lambda p: FusedAdamW(p, lr=LR, weight_decay=0), losses[0])):
        g, d = _build(device, dtype)

        def term(y, t, mod=mod, device=device):
            seen[device] = (y.detach().cpu().double(), t.detach().cpu().double())
            return mod(y, t)

        step = GanStep(g, d, make_opt(g.parameters()), make_opt(d.parameters()), lambda y, t: (y - t).abs().mean(), usm_pixel=True, usm_gan=False,
                       lpips=term, lpips_weight=1.0, usm_lpips=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = step(*(t.to(device=device, dtype=dtype) for t in (lq, gt, gt_usm)))
        assert list(out) == NAMES_L
        rows[device] = {n: float(out[n]) for n in NAMES_L}
    y, t = seen["cuda"]
    assert torch.equal(t, gt_usm.double())                                      # usm_lpips: the sharpened target
    want = float(losses[1].composite(y, t))
    rel = abs(rows["cuda"]["loss_g_lpips"] - want) / want
    print(f"loss_g_lpips: gpu {rows['cuda']['loss_g_lpips']:.9f}; float64 composite on the GPU run's restored image {want:.9f}: relative {rel:.3e} "
          f"(bound 4 x {RECORDED_E:.2e} = {4 * RECORDED_E:.2e}); CPU run {rows['cpu']['loss_g_lpips']:.9f}")
    for n in NAMES_L:
        if n != "loss_g_lpips":
            print(f"{n}: gpu {rows['cuda'][n]:.7f} cpu {rows['cpu'][n]:.7f} |d| {abs(rows['cuda'][n] - rows['cpu'][n]):.2e} (bound {TOL:.2e})")
    assert want > 0 and rel <= 4 * RECORDED_E, (rel, 4 * RECORDED_E)
    for n in NAMES_L:
        if n != "loss_g_lpips":
            assert abs(rows["cuda"][n] - rows["cpu"][n]) <= TOL, n
