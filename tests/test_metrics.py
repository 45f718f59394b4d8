"""metrics.image_metrics on CPU tensors (the plain-torch restatement) against what the reference's metric modules report
(tests/golden/metrics/metrics.npz, written by tools/make_golden_metrics.py), its C-ABI struct, and the evaluate CLI's new options."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import _lib, evaluate as EV, metrics as M
from oracle import refshim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics", "metrics.npz")
# bars: PSNR / PSNR-B in dB against the reference's fp32 values; SSIM against the float64 run of the reference's functions (its
# fp32 SSIM carries the rounding of the convolution backend: up to ~3e-5 on the smooth cases, see metrics.py)
DB, SSIM = 1e-4, 1e-5


def _golden():
    return np.load(GOLDEN, allow_pickle=False)


def _cases():
    return sorted({k.split("__")[0] for k in _golden().files})


def _groups(C):
    return [g for g, keys in M.GROUPS.items() if C == 3 or not any(k.endswith("_y") for k in keys)]


def check_against_golden(z, name, group, got):
    for k, v in got.items():
        v = v.detach().double().cpu().numpy()
        for ref in ("", "__fp64") if "ssim" not in k else ("__fp64",):
            want = z[f"{name}__{k}{ref}"].astype(np.float64)
            fin = np.isfinite(want)
            assert (np.isfinite(v) == fin).all() and (v[~fin] == want[~fin]).all(), (name, group, k, v, want)
            bar = SSIM if "ssim" in k else DB
            assert np.abs(v[fin] - want[fin]).max(initial=0.0) <= bar, (name, group, k, v, want)
    for k in (k for k in got if "ssim" in k):     # and the reference's own fp32 SSIM is not far either
        assert np.abs(got[k].double().cpu().numpy() - z[f"{name}__{k}"]).max() < 5e-5


def _inputs(z, name):
    return torch.from_numpy(z[f"{name}__restored"]), torch.from_numpy(z[f"{name}__target"]), int(z[f"{name}__scale"])


@pytest.mark.parametrize("name", _cases())
def test_torch_path_matches_reference(name):
    z = _golden()
    r, t, scale = _inputs(z, name)
    for group in _groups(r.shape[1]):
        got = M.image_metrics(r, t, group, scale)
        assert list(got) == list(M.GROUPS[group]) and all(v.shape == (r.shape[0],) for v in got.values())
        check_against_golden(z, name, group, got)


def test_golden_covers_the_issue_cases():
    z = _golden()
    assert os.path.getsize(GOLDEN) < 4 << 20
    assert np.isinf(z["rgb_identical_23x17__val_psnr"]).all() and np.isfinite(z["rgb_identical_23x17__val_psnrb"]).all()
    assert (z["rgb_12x12__val_psnrb"] == -np.inf).all() and (z["gray_12x12__val_psnrb"] == -np.inf).all()
    shapes = {n: z[f"{n}__restored"].shape for n in _cases()}
    assert any(s[-1] % 8 and min(s[-2:]) >= 16 for s in shapes.values())
    assert max(np.prod(s[-2:]) for s in shapes.values()) >= 300 * 500


def test_val_psnr_y_is_evaluate_psnr_y():
    """evaluate.psnr_y (fp32) and the new val_psnr_y (float64 sums of the same rounded Y planes) agree to the fp32 resolution of
    psnr_y's result (2 ulp: ~4e-6 dB at 30 dB)."""
    g = torch.Generator().manual_seed(1)
    for shp in [(2, 3, 40, 48), (1, 3, 96, 120), (1, 3, 256, 256)]:
        for scale in (1, 2, 4):
            t = (torch.rand(*shp, generator=g) * 255).round() / 255           # 8-bit targets, as images read from files are
            r = t + 0.05 * torch.randn(*shp, generator=g)
            a = M.image_metrics(r, t, "restorer", scale)["val_psnr_y"]
            b = EV.psnr_y(r, t, scale).double()
            assert ((a - b).abs() <= 2 * torch.finfo(torch.float32).eps * b.abs()).all(), (shp, scale, a, b)


def test_arguments_are_checked():
    x = torch.rand(1, 3, 20, 20)
    with pytest.raises(ValueError):
        M.image_metrics(x, x, "restorer_nope")
    with pytest.raises(ValueError):
        M.image_metrics(x, x[..., :19], "restorer")
    with pytest.raises(ValueError):
        M.image_metrics(x[:, :1], x[:, :1], "restorer")                    # Y metrics of a grey image
    with pytest.raises(ValueError):
        M.image_metrics(x[:, :2], x[:, :2], "restorer_gray")
    with pytest.raises(ValueError):
        M.image_metrics(x, x, "restorer", scale=10)                        # shave leaves nothing
    assert set(M.image_metrics(x[:, :1], x[:, :1], "restorer_jpeg_gray")) == {"val_psnr", "val_ssim", "val_psnrb"}


def test_metric_args_layout_matches_the_c_header():
    """The layout of GrlMetricArgs is compared with the header in tests/test_abi.py, like every struct's, and so is
    GRL_METRIC_COUNT; the metric bits stay here."""
    assert _lib.METRIC_COUNT == len(M.BITS)
    assert [M.BITS[k] for k in M.GROUPS["restorer_jpeg"]] == [_lib.METRIC_PSNR, _lib.METRIC_PSNR_Y, _lib.METRIC_SSIM,
                                                              _lib.METRIC_SSIM_Y, _lib.METRIC_PSNRB, _lib.METRIC_PSNRB_Y]


def _script():
    spec = importlib.util.spec_from_file_location("make_golden_metrics", os.path.join(ROOT, "tools", "make_golden_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_golden_inputs_come_from_the_script():
    z = _golden()
    cases = _script().make_cases()
    assert sorted(cases) == _cases()
    for name, (r, t, scale) in cases.items():
        assert np.array_equal(z[f"{name}__restored"], r.numpy()) and np.array_equal(z[f"{name}__target"], t.numpy())
        assert int(z[f"{name}__scale"]) == scale


@pytest.mark.skipif(not os.path.isfile(os.path.join(refshim.REFERENCE_ROOT, "utils", "metrics", "psnrb.py")),
                    reason="needs the reference tree (fixture regeneration)")
def test_golden_reproduced_bit_for_bit_by_the_script():
    z = _golden()
    arrays = _script().build(refshim.REFERENCE_ROOT)
    assert sorted(arrays) == sorted(z.files)
    for k, v in arrays.items():
        assert v.dtype == z[k].dtype and np.array_equal(v, z[k], equal_nan=True), k


def test_read_image_grey(tmp_path):
    from PIL import Image

    a = (np.arange(12 * 10, dtype=np.uint8) * 2).reshape(12, 10)
    Image.fromarray(a, mode="L").save(tmp_path / "g.png")
    x = EV._read_image(str(tmp_path / "g.png"), "L")
    assert x.shape == (1, 1, 12, 10) and torch.equal(x[0, 0], torch.from_numpy(a).float() / 255)
    assert EV._read_image(str(tmp_path / "g.png")).shape == (1, 3, 12, 10)      # the default stays RGB
