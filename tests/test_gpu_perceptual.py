"""The VGG19 perceptual loss on the GPU (csrc/vgg.hip, perceptual.py): the tap and prep kernels against torch on the same fp32 values,
the whole chain at full widths against the float64 CPU composite, the chain's own operand scale, and ``GanStep`` with the term on.

Yardstick of the chain tests (as tests/test_gpu_disc.py): 4 x the max-abs error of the composite's own ``operand_dtype=float16``
emulation against the float64 composite on the same case.  Forward: every run under its own ReLU / pool decisions (both are
continuous).  Gradient: the derivative jumps wherever a ReLU, a pool maximum or an L1 sign flips, so the float64 composite and the
emulation (``dy`` rounded to fp16 under the chain's scale S as well) both take the decisions of the GPU run's traced features.

Measured on an MI355X, 2026-10-19 (the tests print every figure next to its bound):

  tap kernels, sum |fx - fg| against float64 (bound n * 2^-24 * max|f|)
    (2, 64, 6, 10)   |d| 4.2e-04  (1.7e-03)        (2, 128, 2, 2)   |d| 8.3e-06  (2.4e-04)
    (1, 64, 5, 7)    |d| 1.6e-05  (5.4e-04)        (1, 512, 2, 3)   |d| 7.2e-05  (7.3e-04)
    pooled outputs and dfx: equal to torch's; prep forward / backward: relative error 0 (bound 8 * 2^-24 = 4.8e-07)

  chain forward, max|f_gpu - f_64| (bound = 4 x the emulation's max|f_emu - f_64|)
                   (2, 3, 32, 32)         (1, 3, 35, 50)         (1, 3, 16, 16)
    conv1_2   2.90e-03 (1.16e-02)    2.81e-03 (1.11e-02)    2.58e-03 (1.03e-02)
    conv2_2   5.13e-03 (2.05e-02)    4.40e-03 (1.76e-02)    3.78e-03 (1.51e-02)
    conv3_4   7.73e-03 (3.16e-02)    7.69e-03 (3.09e-02)    4.96e-03 (2.05e-02)
    conv4_4   7.67e-03 (3.01e-02)    8.07e-03 (3.16e-02)    1.31e-03 (5.05e-03)
    conv5_4   1.71e-03 (6.74e-03)    3.11e-03 (1.16e-02)    3.58e-05 (1.40e-04)
    loss      2.58e-05 (6.78e-05)    1.65e-04 (1.70e-04)    6.04e-05 (7.80e-05)

  chain gradient under the GPU run's decisions, max|g_gpu - g_64| (bound 4 x max|g_emu - g_64|); max|g|; S
    (2, 3, 32, 32)   7.82e-06 (2.98e-05)   1.61e-02   2^9
    (1, 3, 35, 50)   1.24e-05 (5.43e-05)   2.91e-02   2^8
    (1, 3, 16, 16)   1.86e-05 (1.00e-04)   5.28e-02   2^6
    the emulation itself: 4.6e-04 - 4.8e-04 of max|g|

  operand scale on (2, 3, 32, 32), max|g / (weight * upstream) - g_1| (bound 2.98e-05)
    perceptual_weight 1e-6: 1.12e-05 (S = 2^28)      upstream 1e-3: 1.01e-05 (S = 2^18)

  single tap {'conv5_4': 1} on (1, 3, 16, 16): loss |d| 1.10e-06 (1.09e-05); dL/dx 2.69e-07 (8.24e-07)

  GanStep: loss_g_percep against the float64 composite on the GPU run's restored image 8.95e-05 (bound 4 x 5.69e-05 = 2.27e-04);
    against the float64 CPU run: loss_g_pix 5.4e-07, loss_g_gan 2.0e-07, loss_d_real 1.6e-07, loss_d_fake 6.3e-06, out_d_real 3.3e-07,
    out_d_fake 1.2e-05 (bound 5e-04 each); not bounded: loss_g_percep against the CPU run 1.8e-04 at max|restored_gpu - restored_cpu| 9.8e-04
"""
import json
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -24
SEED = 7
TAPS = ["conv1_2", "conv2_2", "conv3_4", "conv4_4", "conv5_4"]


def _tok(t):
    """[B, C, H, W] -> the channels-last token matrix [B*H*W, C] (contiguous)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _img(t, B, H, W):
    return t.view(B, H, W, -1).permute(0, 3, 1, 2)


# ---- tap kernels ----------------------------------------------------------------------------------------------------------------
def _tap_inputs(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    fx, fg = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    fx[:, : C // 2, 0:2, 0:2] = 0.75                 # a window of equal positive values: the tie goes to the first
    c0 = (W // 2 - 1) * 2                            # the last complete pool window of the first two rows (W = 7: columns 4, 5)
    neg = fx[:, :, 0:2, c0:c0 + 2] if W >= 4 else fx[:, C // 2:, 0:2, 0:2]
    neg.copy_(-neg.abs() - 0.1)                      # an all-negative window
    fg[:, 1::3, H - 1, :] = fx[:, 1::3, H - 1, :]    # fx == fg: sign 0
    fg[:, 0, 0, 0] = fx[:, 0, 0, 0]
    return fx.cuda(), fg.cuda()


@pytest.mark.parametrize("B,C,H,W,pool,pool_dtype", [(2, 64, 6, 10, True, torch.float16), (2, 64, 6, 10, True, torch.float32),
                                                     (1, 64, 5, 7, True, torch.float16), (1, 64, 5, 7, True, torch.float32),
                                                     (2, 128, 2, 2, True, torch.float16), (1, 512, 2, 3, False, torch.float16)])
def test_tap_kernels_against_torch(B, C, H, W, pool, pool_dtype):
    from grl_image_restoration_amd import ops

    fx, fg = _tap_inputs(B, C, H, W, seed=C + H)
    tx, tg = _tok(fx), _tok(fg)
    n = fx.numel()
    coef = 0.37 / n

    def forward():
        loss = torch.full((1,), 5.0, device="cuda")
        lsum = torch.zeros(1, device="cuda")
        pooled = ops.vgg_tap(tx, tg, B, H, W, loss, coef, accumulate=False, pool=pool, pool_dtype=pool_dtype, layer_sum=lsum)
        ops.vgg_tap(tx, tg, B, H, W, loss, coef, accumulate=True, pool=pool, pool_dtype=pool_dtype)      # a second layer's share
        return loss, lsum, pooled

    loss, lsum, pooled = forward()
    # (a) the loss: fixed-order sum within n * 2^-24 * max|f| of a float64 sum
    s64 = float((fx.double() - fg.double()).abs().sum())
    fmax = float(torch.maximum(fx.abs().max(), fg.abs().max()))
    bound = n * EPS * fmax
    print(f"({B},{C},{H},{W}) sum|fx-fg| {float(lsum):.6f} against {s64:.6f}: |d| {abs(float(lsum) - s64):.3e} (bound {bound:.3e})")
    assert abs(float(lsum) - s64) <= bound
    assert abs(float(loss) - 2 * coef * s64) <= 2 * coef * bound, (float(loss), 2 * coef * s64)
    # (b) relu + max pool of both halves, floor sizes: exactly torch's, after the same rounding
    if pool:
        hp, wp = H // 2, W // 2
        assert pooled.dtype == pool_dtype and tuple(pooled.shape) == (2 * B * hp * wp, C)
        for half, f in ((pooled[: B * hp * wp], fx), (pooled[B * hp * wp:], fg)):
            want = F.max_pool2d(F.relu(f), 2, 2).to(pool_dtype)
            assert torch.equal(_img(half, B, hp, wp), want)
    else:
        assert pooled is None
    # (c) the backward: torch autograd of coef * |fx - fg|.sum() + <relu-pool(fx), dpool>, one fp32 rounding of the two terms' sum
    k = 3.0 * coef
    a = fx.clone().requires_grad_(True)
    (t1,) = torch.autograd.grad(k * (a - fg).abs().sum(), a)
    want = t1
    dpool = None
    if pool:
        dp = torch.randn(B, C, H // 2, W // 2, generator=torch.Generator().manual_seed(3)).cuda()
        (t2,) = torch.autograd.grad((F.max_pool2d(F.relu(a), 2, 2) * dp).sum(), a)
        want = (t1.double() + t2.double()).float()
        dpool = _tok(dp)
        assert float(t2[:, : C // 2, 0, 0].abs().min()) > 0 and float(t2[:, : C // 2, 0, 1].abs().max()) == 0      # the tie went to the first
    dfx = ops.vgg_tap_bwd(tx, tg, B, H, W, k, dpool)
    got = _img(dfx, B, H, W)
    assert torch.equal(got, want), float((got - want).abs().max())
    if not pool:
        assert float(got[:, 1::3, H - 1, :].abs().max()) == 0                  # fx == fg: sign(0) = 0
    # (d) bit-identical from run to run
    loss2, lsum2, pooled2 = forward()
    assert torch.equal(loss, loss2) and torch.equal(lsum, lsum2) and (pooled is None or torch.equal(pooled, pooled2))
    assert torch.equal(dfx, ops.vgg_tap_bwd(tx, tg, B, H, W, k, dpool))


def test_tap_takes_the_two_halves_of_one_matrix():
    from grl_image_restoration_amd import ops

    B, C, H, W = 1, 64, 4, 6
    fx, fg = _tap_inputs(B, C, H, W, seed=1)
    both = torch.cat([_tok(fx), _tok(fg)])
    n = B * H * W
    l1, l2 = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    p1 = ops.vgg_tap(both[:n], both[n:], B, H, W, l1, 1.0, accumulate=False)
    p2 = ops.vgg_tap(_tok(fx), _tok(fg), B, H, W, l2, 1.0, accumulate=False)
    assert torch.equal(l1, l2) and torch.equal(p1, p2)


def test_tap_kernels_propagate_nan_as_torch_does():
    """A NaN feature (a diverged generator) reaches the pooled output and the loss as through torch's relu / max_pool2d / l1_loss,
    and the gradient is what their autograd gives: sign(NaN) = 0 in the L1 term, and the NaN, which took its window's maximum,
    receives the pool gradient."""
    from grl_image_restoration_amd import ops

    B, C, H, W = 1, 64, 4, 6
    fx, fg = _tap_inputs(B, C, H, W, seed=2)
    fx[0, 5, 1, 3] = float("nan")                    # beside positive values, not first in its window
    fx[0, 9, 2, 0] = float("nan")                    # first in its window
    tx, tg = _tok(fx), _tok(fg)
    loss = torch.zeros(1, device="cuda")
    pooled = ops.vgg_tap(tx, tg, B, H, W, loss, 1.0, accumulate=False, pool_dtype=torch.float32)
    want = F.max_pool2d(F.relu(fx), 2, 2)
    got = _img(pooled[: B * 2 * 3], B, 2, 3)
    assert bool(torch.isnan(loss).all()) and int(torch.isnan(want).sum()) == 2
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))
    dp = torch.randn(B, C, 2, 3, generator=torch.Generator().manual_seed(3)).cuda()
    a = fx.clone().requires_grad_(True)
    (t1,) = torch.autograd.grad(0.25 * (a - fg).abs().sum(), a)
    (t2,) = torch.autograd.grad((F.max_pool2d(F.relu(a), 2, 2) * dp).sum(), a)
    want = (t1.double() + t2.double()).float()
    got = _img(ops.vgg_tap_bwd(tx, tg, B, H, W, 0.25, _tok(dp)), B, H, W)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))
    assert float(got[0, 5, 1, 3]) == float(dp[0, 5, 0, 1]) and float(got[0, 9, 2, 0]) == float(dp[0, 9, 1, 0])


# ---- prep -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_input_norm,range_norm", [(True, False), (True, True), (False, False)])
def test_prep_forward_and_backward_against_torch(use_input_norm, range_norm):
    from grl_image_restoration_amd import ops

    g = torch.Generator().manual_seed(4)
    big = torch.rand(2, 4, 21, 19, generator=g).cuda()
    big = big * 2 - 1 if range_norm else big
    mean = torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1).cuda()
    std = torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1).cuda()
    for x in (big[:, :3].contiguous(), big[:, 1:, 2:-1, 3:-2]):                 # contiguous, and a slice read through its strides
        assert x.dtype == torch.float32
        B, _, H, W = x.shape
        a = x.detach().clone().requires_grad_(True)
        t = (a + 1) / 2 if range_norm else a
        t = (t - mean) / std if use_input_norm else t
        tok = ops.vgg_prep(x, use_input_norm=use_input_norm, range_norm=range_norm)
        assert tuple(tok.shape) == (B * H * W, 4) and float(tok[:, 3].abs().max()) == 0
        got, want = _img(tok[:, :3], B, H, W), t.detach()
        err = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
        print(f"prep forward norm={use_input_norm} range={range_norm} {tuple(x.shape)}: max relative error {err:.3e} (bound {8 * EPS:.3e})")
        assert err <= 8 * EPS
        dt = torch.randn(B * H * W, 4, generator=g).cuda()
        (gw,) = torch.autograd.grad((t * _img(dt[:, :3], B, H, W)).sum(), a)
        gx = ops.vgg_prep_bwd(dt, B, H, W, scale=2.0 ** -5, use_input_norm=use_input_norm, range_norm=range_norm) * 2.0 ** 5
        err = float(((gx - gw).abs() / gw.abs().clamp_min(1e-30)).max())
        print(f"prep backward: max relative error {err:.3e} (bound {8 * EPS:.3e})")
        assert tuple(gx.shape) == (B, 3, H, W) and err <= 8 * EPS


# ---- the whole chain at full widths -----------------------------------------------------------------------------------------------
SHAPES = [(2, 3, 32, 32), (1, 3, 35, 50), (1, 3, 16, 16)]


def _pair(shape, seed=21):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g)
    return (gt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1), gt


def _losses(layer_weights=None, **kw):
    from grl_image_restoration_amd import perceptual as P

    sd = P.seeded_state_dict(SEED)
    lw = layer_weights or P.GAN_LAYER_WEIGHTS
    return P.PerceptualLoss(lw, sd, **kw).cuda(), P.PerceptualLoss(lw, sd, **kw)


def _gpu_grad(pl, x, gt, upstream=1.0):
    xg, gg = x.cuda().requires_grad_(True), gt.cuda().requires_grad_(True)
    loss, trace = pl.forward_traced(xg, gg)
    (loss * upstream).backward()
    assert gg.grad is None and all(p.grad is None for p in pl.parameters())     # frozen VGG, detached target
    return loss.detach(), trace, xg.grad.detach().cpu().double()


def _run_chain(pl_gpu, pl_cpu, shape):
    """One GPU run of a shape and its CPU yardsticks."""
    from grl_image_restoration_amd import perceptual as P

    x, gt = _pair(shape)
    B = shape[0]
    loss, trace, g_gpu = _gpu_grad(pl_gpu, x, gt)
    S = pl_gpu.last_scale
    # forward yardstick: own decisions
    t64, temu = [], []
    l64 = pl_cpu.composite(x, gt, trace=t64).detach()
    lemu = pl_cpu.composite(x, gt, operand_dtype=torch.float16, trace=temu).detach()
    # gradient yardstick: the GPU run's decisions
    dec = P.decisions_from_trace(pl_cpu.vgg, trace, B)
    grads = []
    for kw in (dict(), dict(operand_dtype=torch.float16, grad_scale=S)):
        a = x.double().requires_grad_(True)
        pl_cpu.composite(a, gt, decisions=dec, **kw).backward()
        grads.append(a.grad)
    return dict(pl_gpu=pl_gpu, pl_cpu=pl_cpu, x=x, gt=gt, loss=loss, trace=trace, g_gpu=g_gpu, S=S, t64=t64, temu=temu, l64=l64, lemu=lemu,
                g64=grads[0], gemu=grads[1], dec=dec)


@pytest.fixture(scope="module")
def chain():
    """chain(shape): the run of a shape, computed once and shared by the tests of this module; released with the module."""
    pl_gpu, pl_cpu = _losses()
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = _run_chain(pl_gpu, pl_cpu, shape)
        return cache[shape]

    yield get
    cache.clear()


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_forward_against_the_float64_composite(chain, shape):
    c = chain(shape)
    B = shape[0]
    convs = [n for n, _, _, _ in c["pl_cpu"].vgg.convs]
    for name in TAPS:
        i = convs.index(name)
        got, want, emu = c["trace"][i][:B].cpu().double(), c["t64"][i], c["temu"][i]
        err, bound = float((got - want).abs().max()), 4 * float((emu - want).abs().max())
        print(f"{shape} {name}: max|f_gpu - f_64| {err:.3e} (bound 4 x {bound / 4:.3e} = {bound:.3e}; max|f| {float(want.abs().max()):.3f})")
        assert err <= bound, (name, err, bound)
    err, bound = abs(float(c["loss"]) - float(c["l64"])), 4 * abs(float(c["lemu"]) - float(c["l64"]))
    print(f"{shape} loss: gpu {float(c['loss']):.8f} f64 {float(c['l64']):.8f} |d| {err:.3e} (bound 4 x {bound / 4:.3e} = {bound:.3e})")
    assert err <= bound, (err, bound)
    pl = c["pl_gpu"]                                                           # (the per-layer means are reported, not bounded by the issue)
    pl(c["x"].cuda(), c["gt"].cuda())
    means = pl.layer_means(B, shape[2], shape[3]).cpu().double()
    c["pl_cpu"].composite(c["x"], c["gt"])
    want = torch.stack(c["pl_cpu"].last_layer_means)
    assert float(((means - want).abs() / want).max()) < 1e-2


def test_traced_features_are_pre_relu_and_carry_the_backward_masks(chain):
    """All sixteen traced matrices are pre-ReLU (negative values present), close to the float64 composite's, and for the untapped
    layers relu(trace) is, bit for bit, the activated 16-bit output the chain computes with the ReLU in the epilogue."""
    from grl_image_restoration_amd import ops

    c = chain(SHAPES[2])
    vgg = c["pl_gpu"].vgg
    assert len(c["trace"]) == 16
    for i, (name, _, _, _) in enumerate(vgg.convs):
        got, want, emu = c["trace"][i][:1].cpu().double(), c["t64"][i], c["temu"][i]
        assert float(got.min()) < 0 and tuple(got.shape) == tuple(want.shape), name
        # 16-bit storage of an untapped layer adds one fp16 rounding of the value itself to the emulation's error
        slack = float(want.abs().max()) * 2.0 ** -11 if name not in TAPS else 0.0
        assert float((got - want).abs().max()) <= 4 * float((emu - want).abs().max()) + slack, name
    fw, _ = vgg._hip_packs(torch.device("cuda", torch.cuda.current_device()))
    tok = ops.vgg_prep(c["x"].cuda())
    pre = ops.conv3x3(tok, *fw[0], 1, 16, 16, x_cols=4, out_dtype=torch.float16)
    act = ops.conv3x3(tok, *fw[0], 1, 16, 16, x_cols=4, act=2, slope=0.0, out_dtype=torch.float16)
    assert torch.equal(torch.relu(pre), act) and torch.equal(_img(pre.float(), 1, 16, 16), c["trace"][0][:1])


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_gradient_under_the_gpu_runs_decisions(chain, shape):
    c = chain(shape)
    gmax = float(c["g64"].abs().max())
    err, emu = float((c["g_gpu"] - c["g64"]).abs().max()), float((c["gemu"] - c["g64"]).abs().max())
    print(f"{shape} dL/dx: max|g_gpu - g_64| {err:.3e} (bound 4 x {emu:.3e} = {4 * emu:.3e}); max|g| {gmax:.3e}; emulation / max|g| {emu / gmax:.2e}; "
          f"S = 2^{int(np.log2(c['S']))}")
    assert err <= 4 * emu, (err, 4 * emu)


def test_single_tap_runs_the_untapped_block_closers_through_the_tap_kernel():
    """``{'conv5_4': 1}``: conv1_2 .. conv4_4 close their blocks untapped and go through the tap kernel with coefficient 0.  Same
    yardsticks as the five-tap chain, on (1, 3, 16, 16)."""
    c = _run_chain(*_losses({"conv5_4": 1.0}), SHAPES[2])
    err, bound = abs(float(c["loss"]) - float(c["l64"])), 4 * abs(float(c["lemu"]) - float(c["l64"]))
    print(f"single tap loss: gpu {float(c['loss']):.8f} f64 {float(c['l64']):.8f} |d| {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)
    err, emu = float((c["g_gpu"] - c["g64"]).abs().max()), float((c["gemu"] - c["g64"]).abs().max())
    print(f"single tap dL/dx: max|g_gpu - g_64| {err:.3e} (bound 4 x {emu:.3e}); max|g| {float(c['g64'].abs().max()):.3e}")
    assert float(c["g64"].abs().max()) > 0 and err <= 4 * emu, (err, 4 * emu)


def test_feature_extractor_returns_the_chains_tapped_features(chain):
    """``VGG19Features.forward`` on the GPU: the reference's {name: feature before ReLU}, the very values the loss taps."""
    c = chain(SHAPES[2])
    f = c["pl_gpu"].vgg(c["x"].cuda())
    convs = [n for n, _, _, _ in c["pl_cpu"].vgg.convs]
    assert list(f) == TAPS
    for name in TAPS:
        assert torch.equal(f[name], c["trace"][convs.index(name)][:1]), name
    assert tuple(f["conv5_4"].shape) == (1, 512, 1, 1) and tuple(f["conv1_2"].shape) == (1, 64, 16, 16)


def test_chain_is_bit_identical_from_run_to_run(chain):
    c = chain(SHAPES[0])
    loss, _, g = _gpu_grad(c["pl_gpu"], c["x"], c["gt"])
    assert torch.equal(loss, c["loss"]) and torch.equal(g, c["g_gpu"])


@pytest.fixture
def foreign_grad_scale():
    """The device-wide gradient scale of autograd.GradScaleTop set to 1 as another network's pass might leave it; put back after."""
    from grl_image_restoration_amd import autograd as AG

    key = torch.cuda.current_device()
    had, prev = key in AG._State.scales, AG._State.scales.get(key)
    AG._State.scales[key] = 1.0
    yield
    if had:
        AG._State.scales[key] = prev
    else:
        AG._State.scales.pop(key, None)


@pytest.mark.parametrize("weight,upstream", [(1e-6, 1.0), (1.0, 1e-3)])
def test_operand_scale_belongs_to_the_chain(chain, foreign_grad_scale, weight, upstream):
    """Tap coefficients a million (a thousand) times smaller: the gradient, scaled back, is the gradient at weight 1 within the same
    bound.  Without a scale of the chain's own these coefficients flush to zero on their way to fp16."""
    c = chain(SHAPES[0])
    pl, _ = _losses(perceptual_weight=weight)
    _, _, g = _gpu_grad(pl, c["x"], c["gt"], upstream)
    g = g / (weight * upstream)
    emu = float((c["gemu"] - c["g64"]).abs().max())
    err = float((g - c["g_gpu"]).abs().max())
    print(f"weight {weight} upstream {upstream}: S = 2^{int(np.log2(pl.last_scale))} (weight 1: 2^{int(np.log2(c['S']))}); "
          f"max|g * 1/(w u) - g_1| {err:.3e} (bound {4 * emu:.3e}); max|g| {float(g.abs().max()):.3e}")
    assert pl.last_scale > c["S"] * 500 and float(g.abs().max()) > 0
    assert err <= 4 * emu, (err, 4 * emu)


# ---- GanStep ------------------------------------------------------------------------------------------------------------------------
NAMES_P = ["loss_g_pix", "loss_g_percep", "loss_g_gan", "loss_d_real", "loss_d_fake", "out_d_real", "out_d_fake"]
TOL = 5e-4        # tests/test_gpu_gan.py: what the six scalars of this set-up are allowed between the GPU and the float64 CPU run
LR = 2e-4


def _build(device, dtype):
    """The tiny generator and the num_feat-8 discriminator of tests/golden/gan/disc.npz (the set-up of tests/test_gpu_gan.py)."""
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


def test_gan_step_with_the_perceptual_term():
    """One iteration at the tiny-generator set-up of tests/test_gpu_gan.py, on the GPU and on the CPU in float64.  The six scalars
    of that test keep its bound against the CPU run.  ``loss_g_percep`` is held to the emulation-derived bound with the generator's
    own error kept out of it: the float64 composite and its fp16-operand emulation are evaluated on the very restored image the GPU
    run handed to the loss, and |loss_g_percep_gpu - p_64| <= 4 * |p_emu - p_64|.  (Against the CPU RUN's value the term also carries
    the difference of the two restored images; that figure is printed, not bounded.)"""
    from grl_image_restoration_amd import FusedAdamW
    from grl_image_restoration_amd.gan import GanStep

    gen = torch.Generator().manual_seed(5)
    lq, gt, gt_usm = torch.rand(2, 3, 16, 16, generator=gen), torch.rand(2, 3, 32, 32, generator=gen), torch.rand(2, 3, 32, 32, generator=gen)
    rows, seen = {}, {}
    pl_gpu, pl_cpu = _losses()
    for device, dtype, make_opt in (("cpu", torch.float64, lambda p: torch.optim.Adam(p, lr=LR)),
                                    ("cuda", torch.float32, lambda p: FusedAdamW(p, lr=LR, weight_decay=0))):
        g, d = _build(device, dtype)
        pl = pl_gpu if device == "cuda" else pl_cpu

        def percep(y, t, pl=pl, device=device):
            seen[device] = (y.detach().cpu().double(), t.detach().cpu().double())
            return pl(y, t)

        step = GanStep(g, d, make_opt(g.parameters()), make_opt(d.parameters()), lambda y, t: (y - t).abs().mean(), usm_pixel=True, usm_gan=False,
                       perceptual=percep, perceptual_weight=1.0, usm_percep=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = step(*(t.to(device=device, dtype=dtype) for t in (lq, gt, gt_usm)))
        assert list(out) == NAMES_P
        rows[device] = {n: float(out[n]) for n in NAMES_P}
    y, t = seen["cuda"]
    assert torch.equal(t, gt_usm.double())                                      # usm_percep: the sharpened target
    p64, pemu = float(pl_cpu.composite(y, t)), float(pl_cpu.composite(y, t, operand_dtype=torch.float16))
    err, bound = abs(rows["cuda"]["loss_g_percep"] - p64), 4 * abs(pemu - p64)
    print(f"loss_g_percep: gpu {rows['cuda']['loss_g_percep']:.7f}; float64 composite on the GPU run's restored image {p64:.7f}: |d| {err:.2e} "
          f"(bound 4 x {abs(pemu - p64):.2e} = {bound:.2e}); CPU run {rows['cpu']['loss_g_percep']:.7f}, "
          f"max|restored_gpu - restored_cpu| {float((y - seen['cpu'][0]).abs().max()):.2e}")
    for n in NAMES_P:
        if n != "loss_g_percep":
            print(f"{n}: gpu {rows['cuda'][n]:.7f} cpu {rows['cpu'][n]:.7f} |d| {abs(rows['cuda'][n] - rows['cpu'][n]):.2e} (bound {TOL:.2e})")
    assert rows["cuda"]["loss_g_percep"] > 0 and err <= bound, (err, bound)
    for n in NAMES_P:
        if n != "loss_g_percep":
            assert abs(rows["cuda"][n] - rows["cpu"][n]) <= TOL, n
