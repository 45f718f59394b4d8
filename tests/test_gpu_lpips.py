"""LPIPS on the GPU (csrc/lpips.hip, lpips.py): the tap and prep kernels against torch on the same fp32 values, the whole VGG16 chain
against the float64 CPU composite, the metric group restorer_perceptual on CUDA tensors and one folder run.

Bounds.  Tap kernel: each out[b] within 4 * (C + 8) * 2^-24 * U_b of a float64 evaluation of the same fp32 features, U_b =
mean_pixels sum_c |w_c| (u0_c^2 + u1_c^2) -- the first-order bound of an fp32 evaluation whose sums have at most C + 8 terms; the
pooled output bit for bit.  Prep: 2 ulp of the fp32 torch expression.  Chain: the tapped features' max-abs error against the
float64 composite <= 4 x the max-abs error of the composite's own fp16-operand emulation (the rule of tests/test_gpu_perceptual.py);
per image |gpu - f64| / f64 <= 4 * E with E the LARGEST relative emulation error |emu - f64| / f64 over the four images of the three
shapes (pooled: one scalar's emulation error can be small by accident, as the 35 x 50 image's is).

The four images, seeded weights 7, computed on the CPU (float64 composite; fp16-operand emulation; relative difference):
    (2, 3, 32, 32) image 0   4.9510386020e-04   4.9504443390e-04   1.20e-04
    (2, 3, 32, 32) image 1   5.2438454553e-04   5.2430773336e-04   1.46e-04      <- E = 1.46e-04, bound 4 E = 5.86e-04
    (1, 3, 35, 50)           5.1592087208e-04   5.1591811137e-04   5.35e-06
    (1, 3, 16, 16)           6.2538225070e-04   6.2533431517e-04   7.66e-05
  The emulation's feature errors on these shapes are 2.0e-3 .. 7.9e-3 at max|f| 3.4 .. 13, i.e. up to 7e-4 relative: E is of
  that order (a distance averages many such errors), not accidentally tiny.

Measured on an MI355X, 2026-10-19 (the tests print every figure next to its bound):
  tap kernel |out[b] - f64|: 1.6e-12 .. 9.8e-11 over C = 64 .. 512, 5 x 7 and 4 x 4 (bounds 3.5e-07 .. 5.1e-07); prep 0 ulp
  tapped features max|f_gpu - f_64|: 0.79 .. 1.09 x the emulation's own error (bound 4 x)
  values, relative to float64: 1.64e-04, 1.47e-04 | 2.98e-05 | 1.54e-04 (bound 5.86e-04)
  metric group, CUDA against CPU on the same rounded (1, 3, 100, 196) pair at scale 2: val_lpips |d| 3.2e-08 (bar 2.9e-07), val_niqe
  1.3e-07 (1e-06), PSNR 1.7e-07 dB (1e-04), SSIM 3.2e-11 (1e-05)
"""

import pytest
import torch
import torch.nn.functional as F

from grl_image_restoration_amd import evaluate as EV, lpips as LP, metrics as M
from tests.test_gpu_niqe import PATH_SCORE_BAR
from tests.test_lpips import NIQE_PARAMS, _pair
from tests.test_metrics import DB, SSIM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
SEED = 7
SHAPES = [(2, 3, 32, 32), (1, 3, 35, 50), (1, 3, 16, 16)]
RECORDED_E = 1.46e-4


def _tok(t):
    """[B, C, H, W] -> the channels-last token matrix [B*H*W, C] (contiguous)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def _img(t, B, H, W):
    return t.view(B, H, W, -1).permute(0, 3, 1, 2)


# ---- the tap kernel alone ------------------------------------------------------------------------------------------------------------
def _tap_inputs(B, C, H, W, seed):
    """[2B, C, H, W] fp32 features with about a quarter of the entries negative, one all-negative pixel in the restored half (its
    norm after the ReLU is zero), and weights of both signs."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(2 * B, C, H, W, generator=g) + 0.67
    f[0, :, 1, 2] = -f[0, :, 1, 2].abs() - 0.1
    w = torch.randn(C, generator=g) / C
    return f, w


def _tap_reference(f, w, B):
    """Float64 torch on the same values: (d [B], U [B])."""
    r = F.relu(f.double())
    u = r / (r.pow(2).sum(dim=1, keepdim=True).sqrt() + 1e-10)
    w = w.double().view(1, -1, 1, 1)
    d = ((u[:B] - u[B:]).pow(2) * w).sum(dim=1).mean(dim=(1, 2))
    U = ((u[:B].pow(2) + u[B:].pow(2)) * w.abs()).sum(dim=1).mean(dim=(1, 2))
    return d, U


@pytest.mark.parametrize("H,W", [(5, 7), (4, 4)])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_tap_kernel_against_float64_torch(C, H, W):
    from grl_image_restoration_amd import ops

    B = 2
    f, w = _tap_inputs(B, C, H, W, seed=C + H)
    assert 0.15 < float((f < 0).float().mean()) < 0.35 and float(w.min()) < 0 < float(w.max())
    tok, wd = _tok(f).to(DEV), w.to(DEV)

    def run():
        out = torch.full((B,), 5.0, dtype=torch.float64, device=DEV)
        pooled = ops.lpips_tap(tok, wd, B, H, W, out, accumulate=False)
        once = out.clone()
        ops.lpips_tap(tok, wd, B, H, W, out, accumulate=True, pool=False)       # a second layer's share
        return once, out, pooled

    once, twice, pooled = run()
    want, U = _tap_reference(f, w, B)
    for b in range(B):
        err, bound = abs(float(once[b]) - float(want[b])), 4 * (C + 8) * EPS * float(U[b])
        print(f"C {C} {H}x{W} image {b}: gpu {float(once[b]):.9e} f64 {float(want[b]):.9e} |d| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (err, bound)
    assert torch.equal(twice, once + once)
    hp, wp = H // 2, W // 2
    assert pooled.dtype == torch.float16 and tuple(pooled.shape) == (2 * B * hp * wp, C)
    assert torch.equal(_img(pooled, 2 * B, hp, wp).cpu(), F.max_pool2d(F.relu(f), 2, 2).half())
    once2, twice2, pooled2 = run()
    assert torch.equal(once, once2) and torch.equal(twice, twice2) and torch.equal(pooled, pooled2)
    # equal halves: exactly 0, whatever the weights
    same = torch.cat([tok[: B * H * W], tok[: B * H * W]])
    out = torch.full((B,), 5.0, dtype=torch.float64, device=DEV)
    ops.lpips_tap(same, wd, B, H, W, out, accumulate=False, pool=False)
    assert torch.equal(out, torch.zeros_like(out))


def test_tap_kernel_keeps_images_apart_and_nan():
    """A NaN feature of image 1's target reaches out[1] and its pooled window, and nothing of image 0."""
    from grl_image_restoration_amd import ops

    B, C, H, W = 2, 128, 5, 7
    f, w = _tap_inputs(B, C, H, W, seed=3)
    clean = torch.zeros(B, dtype=torch.float64, device=DEV)
    ops.lpips_tap(_tok(f).to(DEV), w.to(DEV), B, H, W, clean, accumulate=False)
    f[B + 1, 9, 2, 3] = float("nan")
    out = torch.zeros(B, dtype=torch.float64, device=DEV)
    pooled = _img(ops.lpips_tap(_tok(f).to(DEV), w.to(DEV), B, H, W, out, accumulate=False), 2 * B, 2, 3).cpu()
    want = F.max_pool2d(F.relu(f), 2, 2).half()
    assert torch.equal(out[0], clean[0]) and bool(torch.isnan(out[1]))
    assert int(torch.isnan(want).sum()) == 1 and bool(torch.isnan(pooled[B + 1, 9, 1, 1]))
    assert torch.equal(torch.isnan(pooled), torch.isnan(want)) and torch.equal(pooled.nan_to_num(7.0), want.nan_to_num(7.0))


def test_tap_kernel_refuses_what_it_does_not_cover():
    from grl_image_restoration_amd import ops

    out = torch.zeros(1, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.lpips_tap(torch.zeros(2 * 16, 96, device=DEV), torch.zeros(96, device=DEV), 1, 4, 4, out)


# ---- prep --------------------------------------------------------------------------------------------------------------------------------
def test_prep_against_torch_on_a_strided_view():
    from grl_image_restoration_amd import ops

    big = torch.rand(2, 4, 21, 19, generator=torch.Generator().manual_seed(4)).to(DEV)
    x = big[:, 1:, 2:-1, 3:-2]
    assert not x.is_contiguous()
    B, _, H, W = x.shape
    shift = torch.Tensor([-0.030, -0.088, -0.188]).view(1, 3, 1, 1).to(DEV)
    scale = torch.Tensor([0.458, 0.448, 0.450]).view(1, 3, 1, 1).to(DEV)
    want = ((2 * x - 1) - shift) / scale
    tok = ops.lpips_prep(x)
    assert tuple(tok.shape) == (B * H * W, 4) and float(tok[:, 3].abs().max()) == 0
    got = _img(tok[:, :3], B, H, W)
    ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want)[1] - 24)         # |want| = m * 2^e, m in [0.5, 1): ulp = 2^(e - 24)
    worst = float(((got - want).abs() / ulp).max())
    print(f"prep: worst error {worst:.2f} ulp (bound 2)")
    assert worst <= 2.0


# ---- the whole chain -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    sd, lin = LP.seeded_weights(SEED)
    return LP.LPIPS(sd, lin).to(DEV), LP.LPIPS(sd, lin)


@pytest.fixture(scope="module")
def runs(models):
    """Per shape one GPU run and its two CPU yardsticks, computed once and shared; E pooled over the four images."""
    gpu, cpu = models
    out = {}
    for shape in SHAPES:
        x, gt = _pair(shape)
        val, trace = gpu.forward_traced(x.to(DEV), gt.to(DEV))
        t64, temu = [], []
        f64 = cpu.composite(x, gt, trace=t64)
        emu = cpu.composite(x, gt, operand_dtype=torch.float16, trace=temu)
        out[shape] = dict(x=x, gt=gt, val=val.cpu(), trace=[t.cpu().double() for t in trace], t64=t64, temu=temu, f64=f64, emu=emu)
    E = max(float(((r["emu"] - r["f64"]).abs() / r["f64"]).max()) for r in out.values())
    return out, E


def test_emulation_error_is_the_recorded_one(runs):
    """E as written down in this file's docstring, and of the order of the features' own relative emulation error."""
    out, E = runs
    feat = max(float((e - t).abs().max()) / float(t.abs().max()) for r in out.values() for e, t in zip(r["temu"], r["t64"]))
    print(f"E = {E:.3e} (recorded {RECORDED_E:.2e}); largest relative feature emulation error {feat:.3e}")
    assert abs(E - RECORDED_E) <= 0.02 * RECORDED_E and all(float(r["f64"].min()) > 1e-4 for r in out.values())
    assert 0.1 * feat <= E <= 10 * feat


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_features_against_the_float64_composite(runs, shape):
    r = runs[0][shape]
    assert len(r["trace"]) == 5
    for name, got, want, emu in zip(LP.TAPS, r["trace"], r["t64"], r["temu"]):
        assert tuple(got.shape) == tuple(want.shape) and float(got.min()) == 0
        err, bound = float((got - want).abs().max()), 4 * float((emu - want).abs().max())
        print(f"{shape} {name}: max|f_gpu - f_64| {err:.3e} (bound 4 x {bound / 4:.3e} = {bound:.3e}; max|f| {float(want.abs().max()):.3f})")
        assert err <= bound, (name, err, bound)


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_value_against_the_float64_composite(runs, shape):
    out, E = runs
    r = out[shape]
    assert r["val"].dtype == torch.float64 and tuple(r["val"].shape) == (shape[0],)
    for b in range(shape[0]):
        rel = abs(float(r["val"][b]) - float(r["f64"][b])) / float(r["f64"][b])
        print(f"{shape} image {b}: gpu {float(r['val'][b]):.10e} f64 {float(r['f64'][b]):.10e} emu {float(r['emu'][b]):.10e} "
              f"relative {rel:.3e} (bound 4 x {E:.3e} = {4 * E:.3e})")
        assert rel <= 4 * E, (rel, 4 * E)


def test_chain_identity_separation_and_repeatability(models, runs):
    gpu, _ = models
    r = runs[0][SHAPES[0]]
    x, gt = r["x"].to(DEV), r["gt"].to(DEV)
    assert torch.equal(gpu(x, x), torch.zeros(2, dtype=torch.float64, device=DEV))
    assert torch.equal(gpu(x, gt).cpu(), r["val"])                             # the same bits on every run
    mixed = gpu(torch.stack([gt[0], x[1]]), gt)
    assert float(mixed[0]) == 0.0 and torch.equal(mixed[1].cpu(), r["val"][1]) and torch.equal(gpu(x[1:], gt[1:]).cpu(), r["val"][1:])


# ---- the metric group ---------------------------------------------------------------------------------------------------------------
def test_metric_group_on_cuda_tensors_agrees_with_the_cpu_call(models, runs):
    gpu, cpu = models
    E = runs[1]
    x, gt = _pair((1, 3, 100, 196), seed=6)                # shaved by 2: 96 x 192, two NIQE blocks
    x, gt = EV.tensor_round(x), EV.tensor_round(gt)         # the same rounded images on both sides
    got = M.image_metrics(x.to(DEV), gt.to(DEV), "restorer_perceptual", scale=2, lpips_model=gpu, niqe_params=NIQE_PARAMS)
    want = M.image_metrics(x, gt, "restorer_perceptual", scale=2, lpips_model=cpu, niqe_params=NIQE_PARAMS)
    assert list(got) == list(M.PERCEPTUAL_GROUPS["restorer_perceptual"]) == list(want)
    for k in got:
        a, b = float(got[k]), float(want[k])
        assert got[k].is_cuda and got[k].dtype == torch.float64 and tuple(got[k].shape) == (1,)
        bar = 4 * E * b if k == "val_lpips" else PATH_SCORE_BAR if k == "val_niqe" else SSIM if "ssim" in k else DB
        print(f"{k}: gpu {a:.8f} cpu {b:.8f} |d| {abs(a - b):.3e} (bar {bar:.3e})")
        assert abs(a - b) <= bar, (k, a, b)
    assert torch.equal(M.lpips(x.to(DEV), gt.to(DEV), gpu, scale=2), got["val_lpips"])


def test_evaluate_folder_reports_the_six_means(models, tmp_path):
    """One ``evaluate_folder`` run on two 64 x 128 LQ images with a seeded GRL-Tiny x2: the six means of the per-image values that
    ``image_metrics`` gives on the module's own output."""
    from PIL import Image

    from grl_image_restoration_amd import GRL, make_config
    from oracle import grl_oracle as O

    gpu, _ = models
    model = GRL(**make_config("tiny", "sr_ckpt_df4", upscale=2)).eval()
    model.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 2), strict=True)
    model = model.to(DEV)
    lq_dir, gt_dir = tmp_path / "lq", tmp_path / "gt"
    lq_dir.mkdir(); gt_dir.mkdir()
    to8 = lambda x: (x[0].permute(1, 2, 0).clamp(0, 1) * 255).round().to(torch.uint8).numpy()
    want = []
    for i in range(2):
        lq, gt = O.synthetic_pair("sr", (64, 128), 2, seed=20 + i)
        Image.fromarray(to8(lq)).save(lq_dir / f"im{i}.png")
        Image.fromarray(to8(gt)).save(gt_dir / f"im{i}.png")
        lq8, gt8 = EV._read_image(str(lq_dir / f"im{i}.png")), EV._read_image(str(gt_dir / f"im{i}.png"))
        with torch.no_grad():
            sr = model(lq8.to(DEV))
        want.append({k: float(v) for k, v in M.image_metrics(sr, gt8.to(DEV), "restorer_perceptual", 2, NIQE_PARAMS, gpu).items()})
    got = EV.evaluate_folder(model, str(lq_dir), str(gt_dir), 2, device=DEV, verbose=False, metric_group="restorer_perceptual",
                             niqe_params=NIQE_PARAMS, lpips_model=gpu)
    assert list(got) == list(M.PERCEPTUAL_GROUPS["restorer_perceptual"])
    for k in got:
        mean = sum(w[k] for w in want) / 2
        assert abs(got[k] - mean) <= 1e-12 * max(1.0, abs(mean)), (k, got[k], mean)
    assert got["val_lpips"] > 0 and got["val_niqe"] > 0
    with pytest.raises(ValueError, match="LPIPS model"):
        EV.evaluate_folder(model, str(lq_dir), str(gt_dir), 2, device=DEV, verbose=False, metric_group="restorer_perceptual",
                           niqe_params=NIQE_PARAMS)
