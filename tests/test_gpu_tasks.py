"""grl_demosaic_matlab (csrc/demosaic.hip) through tasks.py on the MI355X: against the reference fixture through both input forms
(packed CFA4 planes and the RGB lattice, strided views included), against the CPU path on a full-HD batch, on bad arguments; GRL-Small
at the dm geometry on the demosaicked fixture image; and the evaluate CLI's dm and dn tasks end to end."""
import re

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, _lib, evaluate as EV, make_config, metrics as M, tasks as T
from oracle import grl_oracle as O
from tests.test_metrics import DB, SSIM
from tests.test_tasks import REF32, dm_cases, golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rgb_from_cfa4(cfa4):
    """An RGB image whose RGGB lattice holds the mosaic (the other samples are noise: the demosaic must not read them)."""
    N, _, h, w = cfa4.shape
    rgb = torch.rand(N, 3, 2 * h, 2 * w, generator=torch.Generator().manual_seed(9))
    rgb[:, 0, 0::2, 0::2], rgb[:, 1, 0::2, 1::2], rgb[:, 1, 1::2, 0::2], rgb[:, 2, 1::2, 1::2] = cfa4.unbind(1)
    return rgb


@pytest.mark.parametrize("name", dm_cases())
def test_hip_dm_matlab_matches_reference(name):
    meta, z = golden("dm_matlab")
    x = z[f"{name}__cfa4"]
    exact, ref32 = z[f"{name}__ref64"].float(), z[f"{name}__ref32"]
    rgb = _rgb_from_cfa4(x)
    N, _, h, w = x.shape
    big = torch.rand(N, 6, h + 3, w + 5).to(DEV)
    big[:, 1:5, 2 : 2 + h, 3 : 3 + w] = x.to(DEV)
    wide = torch.rand(N, 3, 2 * h + 2, 2 * w + 6).to(DEV)
    wide[..., 2:, 4 : 4 + 2 * w] = rgb.to(DEV)
    outs = {
        "cfa4": T.dm_matlab(x.to(DEV)),
        "cfa4_view": T.dm_matlab(big[:, 1:5, 2 : 2 + h, 3 : 3 + w]),                 # a crop of a larger tensor
        "cfa4_channels_last": T.dm_matlab(x.to(DEV).to(memory_format=torch.channels_last)),
        "rgb": T.demosaic_gt(rgb.to(DEV)),
        "rgb_view": T.demosaic_gt(wide[..., 2:, 4 : 4 + 2 * w]),
    }
    for k, got in outs.items():
        assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and got.shape == exact.shape, k
        got = got.cpu()
        if name in meta["eight_bit"]:
            assert torch.equal(got, exact), (k, (got - exact).abs().max())
        else:
            assert (got - exact).abs().max() <= 1e-6, k
        assert (got - ref32).abs().max() <= REF32, k


def test_hip_matches_cpu_path_full_hd():
    g = torch.Generator().manual_seed(12)
    rgb = torch.randint(0, 256, (2, 3, 1080, 1920), generator=g).float() / 255
    want = T.demosaic_gt(rgb)
    got = T.demosaic_gt(rgb.to(DEV))
    assert torch.equal(got.cpu(), want)
    again = T.dm_matlab(T.mosaic_bayer(rgb.to(DEV)).contiguous())
    assert torch.equal(again, got)
    # partial last tiles in both directions of a grid with several tiles each way: 131 x 500 cells (tiles of 16 x 64 cells)
    rgb = torch.randint(0, 256, (1, 3, 262, 1000), generator=g).float() / 255
    assert torch.equal(T.demosaic_gt(rgb.to(DEV)).cpu(), T.demosaic_gt(rgb))


def test_bad_arguments_raise():
    x = torch.rand(1, 4, 6, 6, device=DEV)
    good = [x[:, i] for i in range(4)]
    with pytest.raises(RuntimeError, match="bad argument"):
        T.hip_demosaic([p[:, :1] for p in good])                   # h < 2
    with pytest.raises(RuntimeError, match="bad argument"):
        T.hip_demosaic([p[:, :, :1] for p in good])                # w < 2
    with pytest.raises(RuntimeError, match="bad argument"):
        T.hip_demosaic([p[:0] for p in good])                      # N = 0
    with pytest.raises(ValueError):
        T.hip_demosaic(good[:3] + [x[:, 3, :, :5]])                # planes of different shapes
    with pytest.raises(TypeError):
        T.dm_matlab(x.half())
    with pytest.raises(ValueError):
        T.dm_matlab(x[..., :1, :])
    with pytest.raises(ValueError):
        T.demosaic_gt(torch.rand(1, 3, 8, 9, device=DEV))
    L = _lib.lib()
    args = _lib.GrlDemosaicArgs(N=1, h=6, w=6, out=torch.empty(1, 3, 12, 12, device=DEV).data_ptr())
    assert L.grl_demosaic_matlab(_lib.stream_ptr(), args) == -1    # null planes


def _pipeline_model(**kw):
    meta, z = golden("dm_pipeline")
    model = GRL(**meta["cfg"], **kw).eval()
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, meta["weight_seed"])
    model.load_state_dict(sd, strict=True)
    return model, sd, meta, z


# GRL-Small at the dm geometry against the reference's fp32 output (which is within 1.2e-6 of the same network on the exactly
# demosaicked input, and moves by 4e-6 under a 2^-20 input perturbation).  Split operands (`high`) measured 4.6e-6 max / 9.9e-7 rms:
# the attention kernels handle 8x8 windows / 32x32 stripes / anchors / 4 at head dim 32.  The default (`auto`) calibrates the blocks
# of narrow models with 8x8 windows (plan.py, resolve_precision): measured 5.4e-4 max / 1.2e-4 rms (1.07e-3 on fp16 operands alone).
PIPELINE_BARS = {"high": (1e-5, 2e-6), "auto": (1e-3, 2e-4)}


@pytest.mark.parametrize("precision", sorted(PIPELINE_BARS))
def test_dm_pipeline_matches_reference(precision):
    """The GT goes through demosaic_gt on the GPU, the model through the HIP path."""
    model, _, _, z = _pipeline_model(precision=precision)
    gt = z["gt"].float() / 255
    lq = T.demosaic_gt(gt.to(DEV))
    assert (lq.cpu() - z["lq"]).abs().max() <= REF32
    with torch.no_grad():
        out = model.to(DEV)(lq).float().cpu()
    d = (out - z["output"]).abs()
    bar_max, bar_rms = PIPELINE_BARS[precision]
    assert out.shape == z["output"].shape and d.max() <= bar_max and d.pow(2).mean().sqrt() <= bar_rms, (d.max(), d.pow(2).mean().sqrt())


def _parse_lines(out):
    """Per-image lines of evaluate's verbose output: {file name: {metric: value}}."""
    rows = {}
    for line in out.splitlines():
        m = re.match(r"^(\S+)\s+((?:val_\w+\s+-?[\d.]+\s*)+)$", line.strip())
        if m and not line.startswith("mean"):
            vals = re.findall(r"(val_\w+)\s+(-?[\d.]+)", m.group(2))
            rows[m.group(1)] = {k: float(v) for k, v in vals}
    return rows


def _task_folder(tmp_path, z, name):
    from PIL import Image

    d = tmp_path / name
    d.mkdir()
    Image.fromarray(z["gt"][0].permute(1, 2, 0).numpy()).save(d / "pipe.png")
    odd = np.random.RandomState(3).randint(0, 256, (45, 61, 3)).astype(np.uint8)    # sides not multiples of 8: cropped to 40 x 56
    Image.fromarray(odd).save(d / "odd_1.png")
    return d


def _check_cli(got, out, want):
    rows = _parse_lines(out)
    assert sorted(rows) == sorted(want), (rows, list(want))
    for name, w in want.items():
        for k, v in w.items():
            assert abs(rows[name][k] - v) <= (1e-4 if "ssim" in k else 1e-3), (name, k, rows[name][k], v)   # printed rounded
    assert list(got) == list(M.GROUPS["restorer"])
    for k in got:
        mean = sum(w[k] for w in want.values()) / len(want)
        assert abs(got[k] - mean) <= (SSIM if "ssim" in k else DB), (k, got[k], mean)


def test_evaluate_cli_dm(tmp_path, capsys):
    model, sd, meta, z = _pipeline_model()
    ck = tmp_path / "dm.ckpt"
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}}, ck)
    d = _task_folder(tmp_path, z, "kodak24")
    model = model.to(DEV)
    want = {}
    for name in ("odd_1.png", "pipe.png"):
        gt = T.modcrop(EV._read_image(str(d / name)), 8).to(DEV)
        with torch.no_grad():
            sr = model(T.demosaic_gt(gt))
        want[name] = {k: float(v) for k, v in M.image_metrics(sr, gt, "restorer").items()}
    got = EV.main(["--task", "dm", "--model", "small", "--geometry", "dm", "--ckpt", str(ck), "--gt", str(d), "--metric", "restorer"])
    _check_cli(got, capsys.readouterr().out, want)
    gt = z["gt"].float() / 255
    ref = M.image_metrics(z["output"], gt, "restorer")
    assert abs(want["pipe.png"]["val_psnr"] - float(ref["val_psnr"])) <= 0.01, (want["pipe.png"], ref)


def test_evaluate_cli_dn(tmp_path, capsys):
    cfg = make_config("small", "dn_df4")
    model = GRL(**cfg).eval()
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1)
    model.load_state_dict(sd, strict=True)
    ck = tmp_path / "dn.ckpt"
    torch.save({"params": sd}, ck)
    _, z = golden("dm_pipeline")
    d = _task_folder(tmp_path, z, "cbsd68")
    model = model.to(DEV)
    want, inputs = {}, {n: (lq, gt) for n, lq, gt in EV.task_inputs(str(d), "dn", sigma=25, device=DEV)}
    for name in ("odd_1.png", "pipe.png"):
        gt = T.modcrop(EV._read_image(str(d / name)), 8)
        lq = gt + T.dn_noise(gt.shape[1:], 25, T.dn_noise_key("CBSD68/" + name)).unsqueeze(0)
        assert torch.equal(inputs[name][0], lq) and torch.equal(inputs[name][1], gt), name
        with torch.no_grad():
            sr = model(lq.to(DEV))
        want[name] = {k: float(v) for k, v in M.image_metrics(sr, gt.to(DEV), "restorer").items()}
    got = EV.main(["--task", "dn", "--sigma", "25", "--model", "small", "--geometry", "dn_df4", "--ckpt", str(ck), "--gt", str(d),
                   "--metric", "restorer"])
    _check_cli(got, capsys.readouterr().out, want)
