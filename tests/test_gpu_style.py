"""The style loss on the GPU (csrc/gram.hip, perceptual.PerceptualStyleLoss): the three Gram kernels on synthetic fp32 features against
float64 torch, the whole chain with both terms against the float64 CPU composite, and ``GanStep`` with both terms on.

Bars.
  Kernels: per matrix max|G_gpu - G_64| <= 4 x max|G_fp32cpu - G_64| with G_fp32cpu torch's own fp32 ``bmm`` of the same F on the CPU
  (4: the margin this package gives a kernel over torch's fp32 arithmetic elsewhere); ``gram_bwd`` under the same bar against
  torch's fp32 ``d0 + k * (F @ sign(D))``.  The loss scalar: the sum is formed in float64 and rounded to fp32 once per launch, so
  4 x 2^-24 relative covers the rounding of the coefficient, of the term and of the accumulating add.
  Chain (the rule of tests/test_gpu_perceptual.py): each D within 4 x the max-abs deviation of the composite's own fp16-operand
  emulation from the float64 composite; the style scalar within 4 x the sum over layers of the emulation's ABSOLUTE per-layer
  deviations (weighted as the loss weights them; their signed sum can cancel); the gradient within 4 x the emulation's deviation, all
  three runs under the GPU run's own decisions -- ReLU masks, pool indices, L1 signs and ``gram_signs``: the smallest |D| entries lie
  at or below fp32's deviation, so signs do flip between arithmetics.

Measured on an MI355X, 2026-10-20 (the tests print every figure next to its bound):

  gram forward, max|G_gpu - G_64| per image (bound 4 x torch's fp32 bmm on the CPU)
    (4, 64, 323)    3.7e-09 - 3.9e-09 (4 x 5.1e-09 - 5.8e-09); the image scaled by 1000: 3.9e-03 (4 x 5.8e-03)
    (2, 512, 1)     4.6e-10, 9.2e-10: torch's own figures to the digit (one product, one rounding on either side)
    (4, 128, 72)    3.4e-09 - 3.6e-09: torch's own figures to the digit (one chunk: the same k-ordered chain)
    (2, 256, 5000)  3.8e-10 - 4.4e-10 (4 x 9.9e-10 - 1.4e-09): forty 128-token chains added in float64 against one long chain
  gram backward, max|d_gpu - d_64| (bound 4 x torch's fp32)
    (2, 64, 323) 4.4e-06 (4 x 3.1e-06)   (1, 512, 33) 2.4e-05 (4 x 1.0e-05)   (2, 128, 72) 6.9e-06 (4 x 7.1e-06)   (1, 256, 1) 5.8e-06 (4 x 6.2e-06)

  chain, max|D_gpu - D_64| (bound = 4 x the emulation's max|D_emu - D_64|): the deviation is the fp16-operand convolutions', which the
  emulation shares -- the GPU sits at 0.8 - 1.1 x the emulation's own figure at every layer
                   (2, 3, 32, 32)         (1, 3, 35, 50)         (1, 3, 16, 16)
    conv1_2   6.26e-06 (2.52e-05)    8.66e-06 (3.44e-05)    1.11e-05 (4.44e-05)
    conv2_2   2.02e-05 (8.19e-05)    1.62e-05 (6.36e-05)    2.75e-05 (1.08e-04)
    conv3_4   3.97e-05 (1.55e-04)    2.43e-05 (1.13e-04)    1.85e-05 (9.24e-05)
    conv4_4   2.74e-05 (1.00e-04)    2.67e-05 (1.34e-04)    2.01e-06 (1.02e-05)
    conv5_4   4.98e-06 (1.81e-05)    1.03e-05 (3.97e-05)    5.08e-08 (2.22e-07)
    style, weight 400    2.84e-04 (1.38e-03)    3.51e-05 (1.34e-03)    8.55e-05 (2.62e-04)      (weight 40 000: both figures x 100)
    smallest |D| of a layer: 1e-13 (conv5_4 at 16 x 16) to 1e-06 (conv1_2)

  chain gradient under the GPU run's decisions, max|g_gpu - g_64| (bound 4 x max|g_emu - g_64|); max|g|; S
    (2, 3, 32, 32)  weight 400: 2.52e-05 (9.52e-05)  6.2e-02  2^7      weight 40 000: 2.09e-03 (1.09e-02)  5.9e+00  2^1
    (1, 3, 35, 50)  weight 400: 4.59e-05 (1.82e-04)  1.2e-01  2^6      weight 40 000: 4.06e-03 (1.41e-02)  1.0e+01  2^0
    (1, 3, 16, 16)  weight 400: 4.44e-05 (2.70e-04)  1.2e-01  2^5      weight 40 000: 2.73e-03 (1.30e-02)  8.0e+00  2^-2
    style only (2, 3, 32, 32), weight 400: 2.05e-05 (8.41e-05)  5.9e-02  2^7  (the perceptual coefficients alone give S = 1)

  GanStep: loss_g_style against the float64 composite on the GPU run's restored image 1.91e-04 (bound 7.30e-04); loss_g_percep 8.95e-05
    (2.27e-04)
"""
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -24
SEED = 7
TAPS = ["conv1_2", "conv2_2", "conv3_4", "conv4_4", "conv5_4"]


# ---- kernels ------------------------------------------------------------------------------------------------------------------------
KSHAPES = [(4, 64, 323), (2, 512, 1), (4, 128, 72), (2, 256, 5000)]        # (images, C, h*w)


def _features(nb, C, hw, seed=3):
    f = torch.randn(nb * hw, C, generator=torch.Generator().manual_seed(seed))
    if (nb, C, hw) == KSHAPES[0]:
        f[2 * hw:3 * hw] *= 1000.0             # one image a thousand times larger: a tile leaking across an image border shows
    return f


def _gram_refs(f, nb, C, hw):
    t = f.view(nb, hw, C)
    g64 = torch.bmm(t.double().transpose(1, 2), t.double()) / (C * hw)
    g32 = torch.bmm(t.transpose(1, 2), t) / (C * hw)
    return g64, g32


@pytest.mark.parametrize("nb,C,hw", KSHAPES)
def test_gram_forward_against_float64(nb, C, hw):
    from grl_image_restoration_amd import ops

    f = _features(nb, C, hw)
    g64, g32 = _gram_refs(f, nb, C, hw)
    fd = f.cuda()
    bound_out = torch.zeros(nb, dtype=torch.float32, device="cuda")
    G = ops.vgg_gram(fd, nb, hw, rowbound=bound_out)
    assert tuple(G.shape) == (nb, C, C) and G.dtype == torch.float32
    for b in range(nb):
        err, ref = float((G[b].cpu().double() - g64[b]).abs().max()), float((g32[b].double() - g64[b]).abs().max())
        print(f"({nb}, {C}, {hw}) image {b}: max|G_gpu - G_64| {err:.3e} (bound 4 x {ref:.3e}); max|G| {float(g64[b].abs().max()):.3e}")
        assert err <= 4 * ref, (b, err, ref)
    assert torch.equal(G, G.transpose(1, 2))                                    # exactly symmetric
    assert torch.equal(G, ops.vgg_gram(fd, nb, hw))                             # the same bits on every run
    # a padded row stride reads the same matrix
    wide = torch.full((nb * hw, C + 8), float("nan"), device="cuda")
    wide[:, :C] = fd
    assert torch.equal(G, ops.vgg_gram(wide[:, :C], nb, hw))
    # rowbound[b] = sum_c max_t |F_b[t, c]|, which is >= max_t sum_c |F_b[t, c]|
    a = f.view(nb, hw, C).abs().double()
    want = a.amax(dim=1).sum(dim=1)
    got = bound_out.cpu().double()
    assert float(((got - want).abs() / want).max()) <= C * EPS and bool((got * (1 + C * EPS) >= a.sum(dim=2).amax(dim=1)).all())


def test_gram_rejects_other_widths():
    from grl_image_restoration_amd import ops

    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.vgg_gram(torch.zeros(2 * 5, 96, device="cuda"), 2, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vgg_gram(torch.zeros(2 * 5, 64), 2, 5)


@pytest.mark.parametrize("nb,C,hw", [KSHAPES[0], KSHAPES[2]])
def test_gram_loss_differences_sum_and_nan(nb, C, hw):
    from grl_image_restoration_amd import ops

    fd = _features(nb, C, hw, seed=5).cuda()
    B = nb // 2
    G = ops.vgg_gram(fd, nb, hw)
    loss, lsum = torch.full((1,), 3.0, device="cuda"), torch.zeros(1, device="cuda")
    coef = 2.0 ** -7
    D = ops.vgg_gram_loss(G, loss, coef, accumulate=False, layer_sum=lsum)
    assert torch.equal(D, G[:B] - G[B:]) and torch.equal(D, D.transpose(1, 2))
    s64 = float(D.double().abs().sum())
    print(f"({nb}, {C}, {hw}) sum|D| {s64:.6e}: loss |d| {abs(float(loss) - coef * s64):.3e}, layer sum |d| {abs(float(lsum) - s64):.3e} "
          f"(bound {4 * EPS * s64:.3e})")
    assert abs(float(loss) - coef * s64) <= 4 * EPS * coef * s64 and abs(float(lsum) - s64) <= 4 * EPS * s64
    first = loss.clone()
    D2 = ops.vgg_gram_loss(G, loss, coef, accumulate=True)                      # a second layer's share
    assert torch.equal(D2, D) and abs(float(loss) - 2 * coef * s64) <= 4 * EPS * 2 * coef * s64
    loss2 = torch.zeros(1, device="cuda")
    ops.vgg_gram_loss(G, loss2, coef, accumulate=False)
    assert torch.equal(loss2, first)                                            # fixed order: the same bits
    # one NaN token gives a NaN loss
    fd[hw + hw // 2, C // 3] = float("nan")
    ops.vgg_gram_loss(ops.vgg_gram(fd, nb, hw), loss2, coef, accumulate=False)
    assert bool(torch.isnan(loss2).all())


@pytest.mark.parametrize("B,C,hw", [(2, 64, 323), (1, 512, 33), (2, 128, 72), (1, 256, 1)])
def test_gram_backward_adds_into_the_gradient_matrix(B, C, hw):
    from grl_image_restoration_amd import ops

    g = torch.Generator().manual_seed(9)
    f = torch.randn((B + 1) * hw, C, generator=g)                               # one more image behind the restored ones
    D = torch.randn(B, C, C, generator=g)                                       # not symmetric: a transposed operand would show
    D[:, ::3, 1::2] = 0.0                                                       # sign(0) = 0
    D[:, 5, :] = 0.0
    d0 = torch.randn((B + 1) * hw, C + 4, generator=g)
    k = 0.37
    sg = torch.sign(D)
    want = d0[: B * hw, :C].double() + k * torch.bmm(f[: B * hw].view(B, hw, C).double(), sg.double()).view(B * hw, C)
    ref32 = d0[: B * hw, :C] + k * torch.bmm(f[: B * hw].view(B, hw, C), sg).view(B * hw, C)
    d = d0.cuda()
    out = ops.vgg_gram_bwd(f.cuda(), D.cuda(), hw, k, d[:, :C])
    assert out.data_ptr() == d.data_ptr()
    got = d.cpu()
    err, ref = float((got[: B * hw, :C].double() - want).abs().max()), float((ref32.double() - want).abs().max())
    print(f"({B}, {C}, {hw}) gram_bwd: max|d_gpu - d_64| {err:.3e} (bound 4 x {ref:.3e}); max|d| {float(want.abs().max()):.3e}")
    assert err <= 4 * ref, (err, ref)
    assert float((got[: B * hw, :C] - d0[: B * hw, :C]).abs().max()) > 1.0      # (it did add)
    assert torch.equal(got[B * hw:], d0[B * hw:]) and torch.equal(got[:, C:], d0[:, C:])      # other rows / columns: the same bits
    d2 = d0.cuda()
    ops.vgg_gram_bwd(f.cuda(), D.cuda(), hw, k, d2[:, :C])
    assert torch.equal(d2, d)
    d3 = d0.cuda()
    ops.vgg_gram_bwd(f.cuda(), torch.zeros(B, C, C, device="cuda"), hw, k, d3[:, :C])       # Sigma = 0: nothing is added
    assert torch.equal(d3.cpu(), d0)


# ---- the whole chain ------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 3, 32, 32), (1, 3, 35, 50), (1, 3, 16, 16)]
WEIGHTS = [400.0, 40000.0]


def _pair(shape, seed=21):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g)
    return (gt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1), gt


def _gpu_run(pl, x, gt):
    xg, gg = x.cuda().requires_grad_(True), gt.cuda().requires_grad_(True)
    (percep, style), trace, diffs = pl.forward_traced(xg, gg)
    (style if percep is None else percep + style).backward()
    assert gg.grad is None and all(p.grad is None for p in pl.parameters())     # frozen VGG, detached target
    return (None if percep is None else percep.detach()), style.detach(), trace, diffs, xg.grad.detach().cpu().double()


@pytest.fixture(scope="module")
def chain():
    """chain(shape, pw, sw): one GPU run and its CPU yardsticks, computed once and shared.  The forward yardsticks (features, D
    matrices, per-layer means) do not depend on the weights and are shared by the runs of a shape, as are the decisions: the
    chain's forward is the same bits for every weight."""
    from grl_image_restoration_amd import perceptual as P

    sd = P.seeded_state_dict(SEED)
    pl_gpu = P.PerceptualStyleLoss(P.GAN_LAYER_WEIGHTS, sd, style_weight=1.0).cuda()
    pl_cpu = P.PerceptualStyleLoss(P.GAN_LAYER_WEIGHTS, sd, style_weight=1.0)
    fwd, runs = {}, {}

    def get(shape, pw, sw):
        if (shape, pw, sw) in runs:
            return runs[(shape, pw, sw)]
        x, gt = _pair(shape)
        for pl in (pl_gpu, pl_cpu):
            pl.perceptual_weight, pl.style_weight = pw, sw
        percep, style, trace, diffs, g_gpu = _gpu_run(pl_gpu, x, gt)
        S = pl_gpu.last_scale
        if shape not in fwd:
            pl_cpu.composite(x, gt)
            d64, m64 = pl_cpu.last_diffs, torch.stack(pl_cpu.last_style_means)
            pl_cpu.composite(x, gt, operand_dtype=torch.float16)
            demu, memu = pl_cpu.last_diffs, torch.stack(pl_cpu.last_style_means)
            dec = P.decisions_from_trace(pl_cpu.vgg, trace, shape[0], diffs=diffs)
            fwd[shape] = dict(d64=d64, m64=m64, demu=demu, memu=memu, dec=dec, diffs={k: v.clone() for k, v in diffs.items()})
        grads = []
        for kw in (dict(), dict(operand_dtype=torch.float16, grad_scale=S)):
            a = x.double().requires_grad_(True)
            p, s = pl_cpu.composite(a, gt, decisions=fwd[shape]["dec"], **kw)
            (p + s).backward()
            grads.append(a.grad)
        runs[(shape, pw, sw)] = dict(fwd[shape], x=x, gt=gt, percep=percep, style=style, run_diffs=diffs, g_gpu=g_gpu, S=S, g64=grads[0], gemu=grads[1],
                                     pl_gpu=pl_gpu, pl_cpu=pl_cpu)
        return runs[(shape, pw, sw)]

    yield get
    fwd.clear()
    runs.clear()


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_gram_differences_against_the_float64_composite(chain, shape):
    from grl_image_restoration_amd import perceptual as P

    c = chain(shape, 1.0, WEIGHTS[0])
    assert list(c["run_diffs"]) == TAPS
    for name in TAPS:
        got, want, emu = c["run_diffs"][name].cpu().double(), c["d64"][name], c["demu"][name]
        err, bound = float((got - want).abs().max()), 4 * float((emu - want).abs().max())
        print(f"{shape} {name}: max|D_gpu - D_64| {err:.3e} (bound 4 x {bound / 4:.3e}); max|D| {float(want.abs().max()):.3e} min|D| {float(want.abs().min()):.3e}")
        assert err <= bound, (name, err, bound)
        assert torch.equal(c["run_diffs"][name], c["run_diffs"][name].transpose(1, 2))
    lw = torch.tensor([P.GAN_LAYER_WEIGHTS[n] for n in TAPS], dtype=torch.float64)
    for W in WEIGHTS:
        r = chain(shape, 1.0, W)
        want = W * float((lw * c["m64"]).sum())
        err, bound = abs(float(r["style"]) - want), 4 * W * float((lw * (c["memu"] - c["m64"]).abs()).sum())
        print(f"{shape} style_weight {W:g}: gpu {float(r['style']):.8f} f64 {want:.8f} |d| {err:.3e} (bound {bound:.3e}); percep {float(r['percep']):.6f}")
        assert err <= bound, (W, err, bound)
    means = c["pl_gpu"].style_layer_means(shape[0]).cpu().double()
    assert float(((means - c["m64"]).abs() / c["m64"]).max()) < 5e-2


@pytest.mark.parametrize("W", WEIGHTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_chain_gradient_under_the_gpu_runs_decisions(chain, shape, W):
    c = chain(shape, 1.0, W)
    gmax = float(c["g64"].abs().max())
    err, emu = float((c["g_gpu"] - c["g64"]).abs().max()), float((c["gemu"] - c["g64"]).abs().max())
    print(f"{shape} style_weight {W:g} d(percep + style)/dx: max|g_gpu - g_64| {err:.3e} (bound 4 x {emu:.3e}); max|g| {gmax:.3e}; "
          f"S = 2^{int(np.log2(c['S']))}")
    assert gmax > 0 and err <= 4 * emu, (err, 4 * emu)


def test_style_only_run_carries_its_gradient_under_the_chains_scale(chain):
    """perceptual_weight 0: the tap kernels get coefficient 0 and every gradient of the chain is the style term's, ~1e-8 at a tap.
    An operand scale taken from the perceptual coefficients alone would be 1 and these gradients would vanish in the fp16 loaders."""
    from grl_image_restoration_amd import perceptual as P

    shape = SHAPES[0]
    c = chain(shape, 0.0, WEIGHTS[0])
    assert c["percep"] is None and float(c["style"]) > 0
    both = chain(shape, 1.0, WEIGHTS[0])
    assert torch.equal(c["style"], both["style"])                                # the same launches on the same features
    gmax = float(c["g64"].abs().max())
    err, emu = float((c["g_gpu"] - c["g64"]).abs().max()), float((c["gemu"] - c["g64"]).abs().max())
    print(f"style only {shape}: max|g_gpu - g_64| {err:.3e} (bound 4 x {emu:.3e}); max|g| {gmax:.3e}; S = 2^{int(np.log2(c['S']))}")
    assert c["S"] > 1.0 and np.log2(c["S"]) == round(np.log2(c["S"]))          # (1.0: what the perceptual coefficients alone give here)
    assert P.operand_scale([0.0] * 16) == 1.0
    assert gmax > 0 and float(c["g_gpu"].abs().max()) > 0.25 * gmax
    assert err <= 4 * emu, (err, 4 * emu)


def test_identical_images_give_zero_style_and_a_finite_gradient(chain):
    pl = chain(SHAPES[2], 1.0, WEIGHTS[0])["pl_gpu"]
    pl.perceptual_weight, pl.style_weight = 1.0, WEIGHTS[1]
    x, _ = _pair(SHAPES[0])
    percep, style, _, diffs, g = _gpu_run(pl, x, x.clone())
    assert float(style) == 0.0 and float(percep) == 0.0 and all(float(d.abs().max()) == 0.0 for d in diffs.values())
    assert bool(torch.isfinite(g).all())


def test_chain_is_bit_identical_from_run_to_run(chain):
    c = chain(SHAPES[0], 1.0, WEIGHTS[1])
    pl = c["pl_gpu"]
    pl.perceptual_weight, pl.style_weight = 1.0, WEIGHTS[1]
    percep, style, _, diffs, g = _gpu_run(pl, c["x"], c["gt"])
    assert torch.equal(percep.detach(), c["percep"].detach()) and torch.equal(style, c["style"]) and torch.equal(g, c["g_gpu"])
    assert all(torch.equal(diffs[k], c["diffs"][k]) for k in TAPS)


def test_style_weight_zero_takes_the_perceptual_chain_alone(chain):
    """``PerceptualStyleLoss`` at style weight 0 is ``PerceptualLoss``: the same bits, and no style term."""
    from grl_image_restoration_amd import perceptual as P

    c = chain(SHAPES[2], 1.0, WEIGHTS[0])
    pl = c["pl_gpu"]
    pl.perceptual_weight, pl.style_weight = 1.0, 0.0
    xg = c["x"].cuda().requires_grad_(True)
    percep, style = pl(xg, c["gt"].cuda())
    percep.backward()
    plain = P.PerceptualLoss(P.GAN_LAYER_WEIGHTS, P.seeded_state_dict(SEED)).cuda()
    x2 = c["x"].cuda().requires_grad_(True)
    want, _ = plain(x2, c["gt"].cuda())
    want.backward()
    assert style is None and torch.equal(percep.detach(), want.detach()) and torch.equal(xg.grad, x2.grad)
    assert torch.equal(percep.detach(), c["percep"].detach())                   # and the style launches leave the perceptual scalar alone


# ---- GanStep ------------------------------------------------------------------------------------------------------------------------
NAMES_S = ["loss_g_pix", "loss_g_percep", "loss_g_style", "loss_g_gan", "loss_d_real", "loss_d_fake", "out_d_real", "out_d_fake"]
LR = 2e-4


def _build(device, dtype):
    """The tiny generator and the num_feat-8 discriminator of tests/golden/gan/disc.npz (the set-up of tests/test_gpu_perceptual.py)."""
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


def test_gan_step_with_both_terms():
    """One iteration on the GPU with the perceptual and the style term.  ``loss_g_style`` (and ``loss_g_percep``) are held to the
    emulation-derived bound with the generator's own error kept out of it: the float64 composite and its fp16-operand emulation are
    evaluated on the very restored image the GPU run handed to the loss.  Both optimizers step."""
    from grl_image_restoration_amd import FusedAdamW
    from grl_image_restoration_amd import perceptual as P
    from grl_image_restoration_amd.gan import GanStep

    gen = torch.Generator().manual_seed(5)
    lq, gt, gt_usm = torch.rand(2, 3, 16, 16, generator=gen), torch.rand(2, 3, 32, 32, generator=gen), torch.rand(2, 3, 32, 32, generator=gen)
    sd = P.seeded_state_dict(SEED)
    pl_gpu = P.PerceptualStyleLoss(P.GAN_LAYER_WEIGHTS, sd, style_weight=WEIGHTS[0]).cuda()
    pl_cpu = P.PerceptualStyleLoss(P.GAN_LAYER_WEIGHTS, sd, style_weight=WEIGHTS[0])
    g, d = _build("cuda", torch.float32)
    seen = {}

    def percep(y, t):
        seen["y"], seen["t"] = y.detach().cpu().double(), t.detach().cpu().double()
        return pl_gpu(y, t)

    before = [p.detach().clone() for p in list(g.parameters()) + list(d.parameters())]
    step = GanStep(g, d, FusedAdamW(g.parameters(), lr=LR, weight_decay=0), FusedAdamW(d.parameters(), lr=LR, weight_decay=0),
                   lambda y, t: (y - t).abs().mean(), usm_pixel=True, usm_gan=False, perceptual=percep, perceptual_weight=1.0, usm_percep=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = step(lq.cuda(), gt.cuda(), gt_usm.cuda())
    assert list(out) == NAMES_S and all(bool(torch.isfinite(v)) for v in out.values())
    assert torch.equal(seen["t"], gt_usm.double())                              # usm_percep: the sharpened target
    p64, s64 = (float(v) for v in pl_cpu.composite(seen["y"], seen["t"]))
    m64 = torch.stack(pl_cpu.last_style_means)
    pemu, _ = (float(v) for v in pl_cpu.composite(seen["y"], seen["t"], operand_dtype=torch.float16))
    memu = torch.stack(pl_cpu.last_style_means)
    lw = torch.tensor([P.GAN_LAYER_WEIGHTS[n] for n in TAPS], dtype=torch.float64)
    err, bound = abs(float(out["loss_g_style"]) - s64), 4 * WEIGHTS[0] * float((lw * (memu - m64).abs()).sum())
    print(f"loss_g_style: gpu {float(out['loss_g_style']):.7f}; float64 composite on the GPU run's restored image {s64:.7f}: |d| {err:.2e} (bound {bound:.2e})")
    assert float(out["loss_g_style"]) > 0 and err <= bound, (err, bound)
    err, bound = abs(float(out["loss_g_percep"]) - p64), 4 * abs(pemu - p64)
    print(f"loss_g_percep: gpu {float(out['loss_g_percep']):.7f}; float64 {p64:.7f}: |d| {err:.2e} (bound {bound:.2e})")
    assert err <= bound, (err, bound)
    after = list(g.parameters()) + list(d.parameters())
    ng = len(list(g.parameters()))
    assert any(not torch.equal(a, b) for a, b in zip(after[:ng], before[:ng])) and any(not torch.equal(a, b) for a, b in zip(after[ng:], before[ng:]))
