"""tasks.py on the CPU (mosaic, the float64 restatement of dm_matlab, the denoising noise, modcrop) against what the reference's own
functions and data sets produce (tests/golden/tasks/*.npz, written by tools/make_golden_tasks.py), the dm preset, the demosaic C-ABI
struct and the evaluate CLI's task options."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import _lib, evaluate as EV, make_config, tasks as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tasks")
# the reference's fp32 dm_matlab against the exact value: its fp32 convolution rounds each partial sum
REF32 = 1e-6


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}


def dm_cases():
    return golden("dm_matlab")[0]["cases"]


def test_mosaic_bayer_is_the_reference_cfa4():
    _, z = golden("dm_matlab")
    got = T.mosaic_bayer(z["mosaic_rgb"])
    assert got.shape == z["mosaic_cfa4"].shape and torch.equal(got, z["mosaic_cfa4"])


@pytest.mark.parametrize("name", dm_cases())
def test_cpu_dm_matlab_matches_reference(name):
    meta, z = golden("dm_matlab")
    x = z[f"{name}__cfa4"]
    got = T.dm_matlab(x)
    assert got.dtype == torch.float32 and got.shape == (x.shape[0], 3, 2 * x.shape[2], 2 * x.shape[3])
    exact = z[f"{name}__ref64"].float()
    if name in meta["eight_bit"]:
        assert torch.equal(got, exact)                    # fp64 sums of 8-bit samples are exact: one rounding to fp32
    else:
        assert (got - exact).abs().max() <= 1e-6
    assert (got - z[f"{name}__ref32"]).abs().max() <= REF32
    if name in meta["eight_bit"]:
        assert torch.equal(T.dm_matlab(x.double()), z[f"{name}__ref64"])


def test_dm_matlab_keeps_native_samples_and_dtype():
    _, z = golden("dm_matlab")
    x = z["u8_b2_8x12__cfa4"]
    y = T.dm_matlab(x)
    assert torch.equal(y[:, 0, 0::2, 0::2], x[:, 0]) and torch.equal(y[:, 1, 0::2, 1::2], x[:, 1])
    assert torch.equal(y[:, 1, 1::2, 0::2], x[:, 2]) and torch.equal(y[:, 2, 1::2, 1::2], x[:, 3])
    assert T.dm_matlab(x.double()).dtype == torch.float64
    const = torch.full((1, 4, 3, 4), 0.25)               # the filters sum to one: a flat mosaic stays flat
    assert torch.equal(T.dm_matlab(const), torch.full((1, 3, 6, 8), 0.25))


def test_demosaic_gt_is_dm_matlab_of_the_mosaic():
    g = torch.Generator().manual_seed(3)
    rgb = torch.randint(0, 256, (2, 3, 10, 14), generator=g).float() / 255
    assert torch.equal(T.demosaic_gt(rgb), T.dm_matlab(T.mosaic_bayer(rgb)))
    assert torch.equal(T.demosaic_gt(rgb.transpose(-1, -2)), T.dm_matlab(T.mosaic_bayer(rgb.transpose(-1, -2).contiguous())))


def test_odd_and_small_sizes_raise():
    with pytest.raises(ValueError):
        T.mosaic_bayer(torch.rand(1, 3, 7, 8))
    with pytest.raises(ValueError):
        T.mosaic_bayer(torch.rand(1, 3, 8, 9))
    with pytest.raises(ValueError):
        T.demosaic_gt(torch.rand(1, 3, 9, 8))
    with pytest.raises(ValueError):
        T.mosaic_bayer(torch.rand(1, 4, 8, 8))
    for h, w in ((1, 4), (4, 1), (1, 1)):
        with pytest.raises(ValueError):
            T.dm_matlab(torch.rand(1, 4, h, w))
        with pytest.raises(ValueError):
            T.demosaic_gt(torch.rand(1, 3, 2 * h, 2 * w))
    with pytest.raises(ValueError):
        T.dm_matlab(torch.rand(1, 3, 4, 4))


def test_dn_noise_is_the_reference_noise():
    meta, z = golden("dn_noise")
    for c in meta["cases"]:
        assert T.dn_noise_key(c["name"]) == c["key"]
        want = z[f"{c['tag']}__noise"]
        got = T.dn_noise(want.shape, meta["sigma"], c["key"])
        assert got.dtype == torch.float32 and torch.equal(got, want), c
    assert not torch.equal(T.dn_noise((1, 8, 8), 25, "a"), T.dn_noise((1, 8, 8), 25, "b"))


def test_dn_test_set_name():
    assert T.dn_test_set_name("kodak24") == "Kodak24" and T.dn_test_set_name("CBSD68") == "CBSD68"
    assert T.dn_test_set_name("mcmaster") == "McMaster" and T.dn_test_set_name("myset") == "myset"


def test_dn_noise_key():
    assert T.dn_noise_key("kodak24/kodim04.png") == "kodak24/kodim04.png"
    assert T.dn_noise_key("set12/08_parrot.png") == "set12/08"
    assert T.dn_noise_key("urban100/img_001_x.png") == "urban100/img"
    assert T.dn_noise_key("_a") == ""


def test_modcrop():
    x = torch.arange(2 * 3 * 21 * 30).reshape(2, 3, 21, 30)
    y = T.modcrop(x, 8)
    assert y.shape == (2, 3, 16, 24) and torch.equal(y, x[..., :16, :24])
    assert T.modcrop(x[0], 8).shape == (3, 16, 24)
    assert T.modcrop(x, 3).shape == (2, 3, 21, 30) and torch.equal(T.modcrop(x, 3), x)
    assert T.modcrop(x, 1).shape == x.shape


def test_dm_preset_matches_reference_config():
    meta, _ = golden("dm_pipeline")
    cfg = make_config("small", "dm")
    assert cfg == meta["cfg"], {k: (cfg.get(k), meta["cfg"].get(k)) for k in set(cfg) | set(meta["cfg"]) if cfg.get(k) != meta["cfg"].get(k)}
    assert cfg["upscale"] == 1 and cfg["upsampler"] == "" and cfg["in_channels"] == 3


def test_demosaic_struct_matches_header():
    A = _lib.GrlDemosaicArgs
    assert ctypes.sizeof(A) == 4 * 8 + 3 * 8 + 4 * 4 + 8
    assert A.out.offset == 72 and A.N.offset == 56
    assert "grl_demosaic_matlab" in _lib.EXPORTS


def test_evaluate_cli_task_arguments(tmp_path):
    gt = tmp_path / "gt"
    gt.mkdir()
    with pytest.raises(SystemExit):
        EV.main(["--task", "sr", "--gt", str(gt)])                # --lq still required for sr
    with pytest.raises(SystemExit):
        EV.main(["--gt", str(gt)])
    with pytest.raises(SystemExit):
        EV.main(["--task", "dn", "--gt", str(gt)])                # no sigma
    with pytest.raises(SystemExit):
        EV.main(["--task", "dm", "--gt", str(gt), "--scale", "2"])
    with pytest.raises(SystemExit):
        EV.main(["--task", "dm", "--gt", str(gt), "--lq", str(gt)])
    with pytest.raises(SystemExit):
        EV.main(["--task", "jpeg", "--gt", str(gt)])


def test_task_inputs_on_cpu(tmp_path):
    """task_inputs reads the GT as 8 bit, crops it to multiples of 8 and adds the keyed noise; dm (with a CPU device) demosaics."""
    from PIL import Image

    g = np.random.RandomState(0)
    d = tmp_path / "myset"
    d.mkdir()
    Image.fromarray(g.randint(0, 256, (21, 35, 3)).astype(np.uint8)).save(d / "b_1.png")
    Image.fromarray(g.randint(0, 256, (16, 24, 3)).astype(np.uint8)).save(d / "a.png")
    items = list(EV.task_inputs(str(d), "dn", sigma=15, device="cpu"))
    assert [n for n, _, _ in items] == ["a.png", "b_1.png"]
    for name, lq, gt in items:
        want = EV._read_image(str(d / name))
        H, W = want.shape[-2] // 8 * 8, want.shape[-1] // 8 * 8
        assert gt.shape == (1, 3, H, W) and torch.equal(gt, want[..., :H, :W])
        key = "myset/" + name.split("_")[0]
        assert torch.equal(lq, gt + T.dn_noise((3, H, W), 15, key).unsqueeze(0))
    other = list(EV.task_inputs(str(d), "dn", sigma=15, noise_prefix="CBSD68", device="cpu"))
    ref = tmp_path / "kodak24"                        # a folder named like a reference test set, in another case
    ref.mkdir()
    Image.fromarray(g.randint(0, 256, (16, 24, 3)).astype(np.uint8)).save(ref / "kodim04.png")
    (_, lq, gt), = EV.task_inputs(str(ref), "dn", sigma=25, device="cpu")
    assert torch.equal(lq, gt + T.dn_noise((3, 16, 24), 25, "Kodak24/kodim04.png").unsqueeze(0))
    assert torch.equal(other[0][1], other[0][2] + T.dn_noise((3, 16, 24), 15, "CBSD68/a.png").unsqueeze(0))
    for name, lq, gt in EV.task_inputs(str(d), "dm", device="cpu"):
        assert torch.equal(lq, T.dm_matlab(T.mosaic_bayer(gt)))
    with pytest.raises(ValueError):
        list(EV.task_inputs(str(d), "dm", channels=1, device="cpu"))
    with pytest.raises(ValueError):
        list(EV.task_inputs(str(d), "dn", device="cpu"))
