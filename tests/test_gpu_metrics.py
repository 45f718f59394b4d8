"""grl_image_metrics (csrc/metrics.hip) through metrics.image_metrics on the MI355X: against the reference fixture, against the CPU
restatement, on strided views, run to run, on bad arguments, and end to end through the evaluate CLI."""
import os

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, _lib, evaluate as EV, make_config, metrics as M
from oracle import grl_oracle as O
from tests.test_metrics import DB, SSIM, _cases, _golden, _groups, _inputs, check_against_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(a, b):
    for k in a:
        x, y = a[k].double().cpu(), b[k].double().cpu()
        fin = torch.isfinite(y)
        assert torch.equal(torch.isfinite(x), fin) and torch.equal(x[~fin], y[~fin]), (k, x, y)
        d = float((x[fin] - y[fin]).abs().max()) if fin.any() else 0.0
        assert d <= (SSIM if "ssim" in k else DB), (k, x, y)


@pytest.mark.parametrize("name", _cases())
def test_hip_matches_reference(name):
    z = _golden()
    r, t, scale = _inputs(z, name)
    for group in _groups(r.shape[1]):
        got = M.image_metrics(r.to(DEV), t.to(DEV), group, scale)
        assert all(v.is_cuda and v.dtype == torch.float64 for v in got.values())
        check_against_golden(z, name, group, got)
        _close(got, M.image_metrics(r, t, group, scale))


def test_hip_matches_cpu_path_on_larger_images():
    g = torch.Generator().manual_seed(4)
    for shp, scale in [((2, 3, 203, 333), 4), ((3, 1, 97, 130), 1), ((1, 3, 64, 64), 2)]:
        t = torch.rand(*shp, generator=g)
        r = t + 0.1 * torch.randn(*shp, generator=g)
        for group in _groups(shp[1]):
            _close(M.image_metrics(r.to(DEV), t.to(DEV), group, scale), M.image_metrics(r, t, group, scale))


def test_strided_views_match_contiguous_copies():
    g = torch.Generator().manual_seed(5)
    big_r = (torch.rand(2, 3, 150, 210, generator=g) * 1.2 - 0.1).to(DEV)
    big_t = torch.rand(2, 3, 150, 210, generator=g).to(DEV)
    views = [
        (big_r[..., 3:140, 5:200], big_t[..., 7:144, 2:197]),                                   # crops (evaluate's sr[..., :h, :w])
        (big_r.to(memory_format=torch.channels_last), big_t),                                    # channels-last model output
        (big_r.transpose(-1, -2), big_t.transpose(-1, -2)),                                      # column-major planes
        (torch.cat([big_r, big_r], 1)[:, ::2], big_t[..., ::1, :]),                              # channel stride of two planes
    ]
    for r, t in views:
        for scale in (1, 4):
            a = M.image_metrics(r, t, "restorer_jpeg", scale)
            b = M.image_metrics(r.contiguous(), t.contiguous(), "restorer_jpeg", scale)
            for k in a:
                assert torch.equal(a[k], b[k]), k


def test_two_calls_are_bitwise_equal():
    g = torch.Generator().manual_seed(6)
    r, t = torch.rand(2, 3, 300, 517, generator=g).to(DEV), torch.rand(2, 3, 300, 517, generator=g).to(DEV)
    a = M.image_metrics(r, t, "restorer_jpeg", 2)
    b = M.image_metrics(r, t, "restorer_jpeg", 2)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_bad_arguments_raise():
    x = torch.rand(1, 3, 20, 24, device=DEV)
    bad = [
        (x, x[..., :23], 0, M.BITS["val_psnr"]),                    # shapes differ
        (x[:, :2], x[:, :2], 0, M.BITS["val_psnr"]),                # C = 2
        (x[:, :1], x[:, :1], 0, M.BITS["val_psnr_y"]),              # a Y metric of a grey image
        (x, x, 10, M.BITS["val_psnr"]),                             # 2 border >= H
        (x, x, 0, 0),                                               # no metric
        (x, x, 0, 64),                                              # unknown metric bit
    ]
    for r, t, border, bits in bad:
        with pytest.raises(RuntimeError, match="bad argument"):
            M.hip_image_metrics(r, t, border, bits)
    with pytest.raises(ValueError):
        M.image_metrics(x, x[..., :23], "restorer")
    with pytest.raises(ValueError):
        M.image_metrics(x, x.cpu(), "restorer")
    assert _lib.lib().grl_image_metrics_workspace_bytes(1, 20, 24, 10) == 0


def test_evaluate_cli_metric_group(tmp_path, capsys):
    """evaluate.main(... --metric restorer) on a PNG folder with a seeded GRL-Tiny checkpoint: every reported mean is what the CPU
    path gives on the module's own output, and its val_psnr_y is what the CLI without --metric (evaluate_folder) reports."""
    from PIL import Image

    model = GRL(**make_config("tiny", "sr_ckpt_df4", upscale=2)).eval()        # what the CLI builds for these flags
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 2)
    ck = tmp_path / "ck.pth"
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}}, ck)
    EV.load_checkpoint(model, str(ck))
    model = model.to(DEV)
    lq_dir, gt_dir = tmp_path / "lq", tmp_path / "gt"
    lq_dir.mkdir(); gt_dir.mkdir()
    to8 = lambda x: (x[0].permute(1, 2, 0).clamp(0, 1) * 255).round().to(torch.uint8).numpy()
    want = []
    for i in range(2):
        lq, gt = O.synthetic_pair("sr", (64, 64), 2, seed=20 + i)
        Image.fromarray(to8(lq)).save(lq_dir / f"im{i}.png")
        Image.fromarray(to8(gt)).save(gt_dir / f"im{i}.png")
        lq8 = EV._read_image(str(lq_dir / f"im{i}.png"))
        gt8 = EV._read_image(str(gt_dir / f"im{i}.png"))
        with torch.no_grad():
            sr = model(lq8.to(DEV)).float().cpu()
        want.append({k: float(v) for k, v in M.image_metrics(sr, gt8, "restorer", 2).items()})
    args = ["--model", "tiny", "--geometry", "sr_ckpt_df4", "--scale", "2", "--ckpt", str(ck), "--lq", str(lq_dir),
            "--gt", str(gt_dir)]
    got = EV.main(args + ["--metric", "restorer"])
    out = capsys.readouterr().out
    assert list(got) == list(M.GROUPS["restorer"]) and all(k in out for k in got) and "mean over 2 images" in out
    for k in got:
        mean = sum(w[k] for w in want) / len(want)
        assert abs(got[k] - mean) <= (SSIM if "ssim" in k else DB), (k, got[k], mean)
    psnr_y = EV.main(args)
    assert isinstance(psnr_y, float) and abs(got["val_psnr_y"] - psnr_y) <= 1e-5, (got["val_psnr_y"], psnr_y)
