"""CPU tests of the USM-sharpened targets: ``tasks.usm_taps`` / ``tasks.usm_sharp`` (the torch restatement), the C ABI's argument
block, ``evaluate --usm-gt``, ``train --usm / --val-usm`` and ``PatchSampler(usm=True)``.

Yardstick: tests/golden/tasks/usm.npz (tools/make_golden_usm.py), a float64 scipy restatement that shares no code with the package,
on the fp32 values of the inputs.  OpenCV is not available, so nothing here claims equality with ``cv2.GaussianBlur``'s summation
order.  The file records blur and result on a 2^-31 grid (|error| <= 2^-32 = 2.4e-10).

Tolerances (u = 2^-24, gamma_n = n u / (1 - n u), |x| <= 1, the taps are positive and sum to 1):
  * a pass is a 51-term fmaf chain: |fl - exact| <= gamma_51 max|x|; two passes: 2 gamma_51 = 6.1e-6 for blur and for soft (m <= 1);
  * ``margin`` = 255 * 2 gamma_51 + 1e-5 = 1.6e-3: a pixel whose |res| * 255 is further than that from the threshold has the same
    mask bit in fp32 and in float64.  The DECIDED threshold of every case is at least 0.01 away from every value, so there the mask
    is exact for any implementation within the blur bound;
  * with equal masks |out - out64| <= 2 gamma_51 (0.5 + 0.5) + 4 u = 6.4e-6: the soft error times |sharp - x| <= weight |res| <= 0.5,
    the blur error times soft * weight <= 0.5, and four roundings of the blend;
  * the CPU path computes in float64 and rounds once: 1e-6 is asked of it (2^-25 of the rounding plus the fixture's grid);
  * 8-bit levels may differ from the recorded ones only where 255 * out64 lies within 1.8e-3 (> 255 * 6.4e-6) of a half-integer,
    and then by one level;
  * at the default threshold 10 the masks may differ at the recorded undecided pixels (U of them), each of which moves soft by at
    most tap_max^2 and the result by at most tap_max^2 * 0.5: the bound is 6.4e-6 + U tap_max^2 0.5.  The float64 result at
    threshold 10 is restated below in numpy from the recorded blur.
"""
import json
import os

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import PatchSampler, PatchStore, _lib, evaluate as EV, presets, tasks as T, train
from grl_image_restoration_amd.image8 import pack8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24
GAMMA51 = 51 * U24 / (1 - 51 * U24)
BLUR_TOL = 2 * GAMMA51 + 2.0 ** -32
OUT_TOL = 6.4e-6
CPU_TOL = 1e-6
HALF_BAND = 1.8e-3


class Fixture:
    def __init__(self):
        z = np.load(os.path.join(ROOT, "tests", "golden", "tasks", "usm.npz"), allow_pickle=False)
        self.meta = json.loads(str(z["meta"]))
        self.taps = z["taps"]
        self.cases = {}
        for name, c in self.meta["cases"].items():
            shape = tuple(c["shape"])
            n = int(np.prod(shape))
            bits = lambda key: np.unpackbits(z[f"{name}__{key}"])[:n].reshape(shape).astype(bool)
            self.cases[name] = dict(
                x8=z[f"{name}__x"], x=torch.from_numpy(z[f"{name}__x"]).float().div(255), threshold=c["threshold"], U=c["U"],
                blur=z[f"{name}__blur_q31"].astype(np.float64) / 2.0 ** 31, out=z[f"{name}__out_q31"].astype(np.float64) / 2.0 ** 31,
                mask=bits("mask"), out8=z[f"{name}__out8"], undecided=bits("undecided"))


@pytest.fixture(scope="module")
def fx():
    return Fixture()


CASES = ("A", "B", "C", "D", "E1", "E2")


def check_levels(k, case):
    """``k``: uint8 levels of an implementation.  They equal the recorded ones except near a half-integer level, by one."""
    k, want = np.asarray(k).astype(np.int64), case["out8"].astype(np.int64)
    level = np.clip(case["out"], 0, 1) * 255.0
    near = np.abs(level - np.floor(level) - 0.5) <= HALF_BAND
    diff = k != want
    assert not (diff & ~near).any(), int((diff & ~near).sum())
    assert np.abs(k - want).max() <= 1
    return int(diff.sum())


def reference_at(case, taps, threshold, weight=0.5):
    """The float64 result at another threshold, from the recorded blur: numpy only, reflect-101 by ``np.pad(mode="reflect")``."""
    t = taps.astype(np.float64)
    h = len(t) // 2
    x = case["x"].double().numpy()
    res = x - case["blur"]
    mask = (np.abs(res) * 255.0 > threshold).astype(np.float64)
    p = np.pad(mask, ((0, 0), (0, 0), (0, 0), (h, h)), mode="reflect")
    rows = sum(t[i] * p[..., i : i + x.shape[-1]] for i in range(len(t)))
    p = np.pad(rows, ((0, 0), (0, 0), (h, h), (0, 0)), mode="reflect")
    soft = sum(t[i] * p[..., i : i + x.shape[-2], :] for i in range(len(t)))
    return mask.astype(bool), soft * np.clip(x + weight * res, 0, 1) + (1 - soft) * x


def test_usm_taps(fx):
    t = T.usm_taps()
    assert t.dtype == torch.float32 and t.shape == (51,) and torch.equal(t, t.flip(0))
    assert abs(float(t.double().sum()) - 1) <= 1e-7
    i = np.arange(51, dtype=np.float64) - 25
    k = np.exp(-(i * i) / (2 * 8.0 ** 2))
    assert np.array_equal(t.numpy(), (k / k.sum()).astype(np.float32)) and np.array_equal(t.numpy(), fx.taps)
    assert torch.equal(T.usm_taps(51), t) and T.usm_taps(2).tolist() == [0.25, 0.5, 0.25] and T.usm_taps(1).tolist() == [1.0]
    with pytest.raises(ValueError):
        T.usm_taps(64)


@pytest.mark.parametrize("name", CASES)
def test_cpu_usm_sharp_on_the_fixture(fx, name):
    c = fx.cases[name]
    out, blur, mask = T.usm_sharp(c["x"], threshold=c["threshold"], parts=True)
    assert out.dtype == torch.float32 and out.shape == c["x"].shape
    assert np.array_equal(mask.numpy() != 0, c["mask"])
    assert np.abs(blur.numpy() - c["blur"]).max() <= 2.0 ** -32 + 1e-15
    err = np.abs(out.double().numpy() - c["out"]).max()
    print(f"{name}: max|cpu - float64| = {err:.3e}")
    assert err <= CPU_TOL
    assert torch.equal(T.usm_sharp(c["x"], threshold=c["threshold"]), out)
    q = T.usm_sharp(c["x"], threshold=c["threshold"], quantise=True)
    assert torch.equal(q, pack8(out).permute(0, 3, 1, 2).float().div(255))
    print(f"{name}: {check_levels((q * 255).round().numpy(), c)} levels differ near a half-integer")


@pytest.mark.parametrize("name", ("A", "B"))
def test_cpu_usm_sharp_at_the_default_threshold(fx, name):
    c = fx.cases[name]
    want_mask, want = reference_at(c, fx.taps, 10.0)
    out, _, mask = T.usm_sharp(c["x"], parts=True)
    assert not ((mask.numpy() != 0) != want_mask)[~c["undecided"]].any()
    assert np.abs(out.double().numpy() - want).max() <= OUT_TOL + c["U"] * float(fx.taps.max()) ** 2 * 0.5


def test_usm_sharp_refuses_what_it_cannot_take():
    with pytest.raises(ValueError):
        T.usm_sharp(torch.zeros(1, 2, 8, 8))
    with pytest.raises(ValueError):
        T.usm_sharp(torch.zeros(3, 8, 8))
    with pytest.raises(TypeError):
        T.usm_sharp(torch.zeros(1, 3, 8, 8, dtype=torch.float64))


def test_usm_args_layout_matches_header_and_abi():
    """The layout of GrlUsmArgs is compared with the header in tests/test_abi.py, like every struct's;
    what is particular to this entry point stays here."""
    assert _lib.ABI_VERSION >= 31
    assert "grl_usm_sharp" in _lib.EXPORTS and "grl_usm_workspace_bytes" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "grl_hip.h")).read()
    assert "utils/utils_bsr/utils_usm.py:34-60" in header and "restoration_sr.py:105-109" in header


# ---- evaluate ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(tmp_path_factory, fx):
    """An LQ / GT folder pair at scale 1: the GT is case B's image (as HWC), the LQ a smoothed copy of it."""
    from PIL import Image

    d = tmp_path_factory.mktemp("usm_pair")
    gt8 = np.ascontiguousarray(fx.cases["B"]["x8"][0].transpose(1, 2, 0))
    lq8 = ((gt8.astype(np.int32) + np.roll(gt8, 1, 0) + np.roll(gt8, 1, 1) + 1) // 3).astype(np.uint8)
    (d / "lq").mkdir()
    (d / "gt").mkdir()
    Image.fromarray(lq8).save(d / "lq" / "im.png")
    Image.fromarray(gt8).save(d / "gt" / "im.png")
    return str(d / "lq"), str(d / "gt"), lq8, gt8


def test_evaluate_folder_scores_against_the_sharpened_gt(fx, pair, tmp_path):
    lq_dir, gt_dir, lq8, gt8 = pair
    c = fx.cases["B"]
    # The sharpened GT that --save-gt writes is held against the float64 restatement at the default threshold under the half-integer
    # condition; the score is then PSNR-Y by hand against exactly that image.
    from PIL import Image

    ident = lambda x: x
    got = EV.evaluate_folder(ident, lq_dir, gt_dir, 1, device="cpu", verbose=False, usm_gt=True, save_dir=str(tmp_path), save_gt=True)
    saved = np.asarray(Image.open(tmp_path / "X1" / "gt" / "im_GT.png"))
    _, want64 = reference_at(c, fx.taps, 10.0)
    check_levels(saved.transpose(2, 0, 1)[None], dict(out=want64, out8=np.rint(np.clip(want64, 0, 1) * 255.0).astype(np.uint8)))
    assert not np.array_equal(saved, gt8)
    lq = torch.from_numpy(lq8).permute(2, 0, 1)[None].float().div(255)
    want = float(EV.psnr_y(lq, torch.from_numpy(saved.copy()).permute(2, 0, 1)[None].float().div(255), 1))
    plain = float(EV.psnr_y(lq, c["x"], 1))
    off = EV.evaluate_folder(ident, lq_dir, gt_dir, 1, device="cpu", verbose=False, usm_gt=False)
    assert got == want and off == plain and got != off
    assert EV.evaluate_folder(ident, lq_dir, gt_dir, 1, device="cpu", verbose=False) == off
    assert EV.evaluate_folder(ident, lq_dir, gt_dir, 1, device="cpu", verbose=False, usm_gt=True) == got
    for task in ("dn", "bsr", "sr_bicubic", "jpeg"):
        with pytest.raises(ValueError):
            EV.evaluate_folder(ident, lq_dir, gt_dir, 1, device="cpu", verbose=False, task=task, sigma=25, quality=10, usm_gt=True)


def test_evaluate_folder_crops_the_gt_to_the_scale_before_sharpening(fx, tmp_path):
    """A 21 x 31 GT at scale 2 is sharpened as its 20 x 30 crop: the border reflects about the cropped edge."""
    from PIL import Image

    gt8 = np.ascontiguousarray(fx.cases["B"]["x8"][0].transpose(1, 2, 0))[:21, :31]
    (tmp_path / "lq").mkdir()
    (tmp_path / "gt").mkdir()
    Image.fromarray(gt8[:20:2, :30:2]).save(tmp_path / "lq" / "a.png")
    Image.fromarray(gt8).save(tmp_path / "gt" / "a.png")
    up = lambda x: x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    got = EV.evaluate_folder(up, str(tmp_path / "lq"), str(tmp_path / "gt"), 2, device="cpu", verbose=False, usm_gt=True)
    gt = torch.from_numpy(gt8).permute(2, 0, 1)[None].float().div(255)
    lq = torch.from_numpy(gt8[:20:2, :30:2]).permute(2, 0, 1)[None].float().div(255)
    want = float(EV.psnr_y(up(lq), T.usm_sharp(gt[..., :20, :30].contiguous(), quantise=True), 2))
    assert got == want


def test_command_lines_take_usm_for_sr_only(pair, capsys):
    lq_dir, gt_dir, _, _ = pair

    def ev(*extra):
        ap = EV._parser()
        a = ap.parse_args(["--gt", gt_dir, *extra])
        EV._check(ap, a)
        return a

    def tr(*extra):
        ap = train._parser()
        a = ap.parse_args(["--gt", gt_dir, "--steps", "1", "--device", "cpu", *extra])
        train._check(ap, a)
        return a

    for call, extra in ((ev, ["--task", "dn", "--sigma", "25", "--usm-gt"]),
                        (tr, ["--task", "dn", "--sigma", "25", "--usm"]),
                        (tr, ["--task", "dn", "--sigma", "25", "--val-usm"]),
                        (tr, ["--task", "sr_bicubic", "--scale", "2", "--usm"])):
        with pytest.raises(SystemExit) as e:
            call(*extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit) as e:                       # bsr takes no --gt at all
        ap = EV._parser()
        EV._check(ap, ap.parse_args(["--task", "bsr", "--lq", lq_dir, "--usm-gt"]))
    assert e.value.code == 2
    capsys.readouterr()
    assert ev("--task", "sr", "--lq", lq_dir, "--usm-gt").usm_gt and not ev("--task", "sr", "--lq", lq_dir).usm_gt
    a = tr("--task", "sr", "--lq", lq_dir, "--scale", "1", "--usm", "--val-usm")
    assert a.usm and a.val_usm
    a = tr("--task", "sr", "--lq", lq_dir, "--scale", "1")
    assert not a.usm and not a.val_usm


# ---- training data ----------------------------------------------------------------------------------------------------------------
def test_sampler_sharpens_the_gt_store_only(fx):
    g = np.random.RandomState(3)
    gts = [np.ascontiguousarray(fx.cases["B"]["x8"][0].transpose(1, 2, 0)), g.randint(0, 256, (24, 40, 3)).astype(np.uint8)]
    lqs = [np.ascontiguousarray(im[::2, ::2]) for im in gts]
    gts = [im[: lq.shape[0] * 2, : lq.shape[1] * 2] for im, lq in zip(gts, lqs)]
    make = lambda **kw: PatchSampler("sr", PatchStore(gts), PatchStore(lqs), patch=8, batch=4, scale=2, seed=5, **kw)
    plain, usm = make(), make(usm=True)
    for n, im in enumerate(gts):
        x = torch.from_numpy(np.ascontiguousarray(im)).permute(2, 0, 1)[None].float().div(255)
        want = pack8(T.usm_sharp(x))[0]
        assert torch.equal(usm.gt_store.image(n), want) and torch.equal(plain.gt_store.image(n), torch.from_numpy(np.ascontiguousarray(im)))
        assert not torch.equal(want, plain.gt_store.image(n))
        assert torch.equal(usm.lq_store.image(n), plain.lq_store.image(n))
    assert usm.gt_store.dims == plain.gt_store.dims
    assert usm.rng_state()["draws"] == plain.rng_state()["draws"]
    wp, wu = plain.draw(), usm.draw()
    assert wp == wu
    (lq_p, gt_p), (lq_u, gt_u) = plain.next(*wp), usm.next(*wu)
    assert torch.equal(lq_p, lq_u) and torch.equal(plain.work, usm.work) and not torch.equal(gt_p, gt_u)
    assert torch.equal(gt_u, usm.gt_store.sample(usm.work, 8, 2))
    with pytest.raises(ValueError):
        PatchSampler("dn", PatchStore(gts), patch=8, batch=2, sigma=25, usm=True)
    with pytest.raises(ValueError):
        PatchSampler("sr_bicubic", PatchStore(gts), patch=8, batch=2, scale=2, usm=True)


def test_bsr_psnr_geometry():
    g = presets.GEOMETRIES["bsr_psnr"]
    assert g == dict(window_size=16, stripe_size=[64, 64], stripe_groups=[None, None], anchor_window_down_factor=4)
    cfg = presets.make_config("base", "bsr_psnr", upscale=4, upsampler="nearest+conv")
    assert cfg["upsampler"] == "nearest+conv" and cfg["window_size"] == 16 and cfg["stripe_size"] == [64, 64]


def test_train_command_line_with_usm_targets(tmp_path, capsys):
    """One eager CPU step of a one-block Tiny model with and without ``--usm --val-usm``: the same crops, another target (so another
    loss), and the validation equals ``evaluate_folder(usm_gt=True)`` on the written checkpoint."""
    from PIL import Image

    from grl_image_restoration_amd import GRL, make_config

    g = np.random.RandomState(0)
    (tmp_path / "gt").mkdir()
    (tmp_path / "lq").mkdir()
    for i in range(2):
        im = g.randint(0, 256, (40, 48, 3)).astype(np.uint8)
        Image.fromarray(im).save(tmp_path / "gt" / f"im{i}.png")
        Image.fromarray(np.ascontiguousarray(im[::2, ::2])).save(tmp_path / "lq" / f"im{i}.png")
    gt, lq = str(tmp_path / "gt"), str(tmp_path / "lq")
    args = ["--task", "sr", "--scale", "2", "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--patch", "16", "--batch", "2",
            "--eager", "--device", "cpu", "--gt", gt, "--lq", lq, "--steps", "1", "--val-gt", gt, "--val-lq", lq, "--val-every", "1",
            "--seed", "3"]
    torch.manual_seed(0)
    plain = train.main(args)
    torch.manual_seed(0)
    usm = train.main(args + ["--usm", "--val-usm", "--out", str(tmp_path / "run")])
    capsys.readouterr()
    assert plain["work"] == usm["work"] and plain["losses"] != usm["losses"] and plain["val"][0][1] != usm["val"][0][1]
    model = GRL(**make_config("tiny", "yaml", upscale=2, img_size=16, depths=[1], num_heads_window=[2], num_heads_stripe=[2])).eval()
    EV.load_checkpoint(model, usm["checkpoint"])
    with torch.no_grad():
        assert EV.evaluate_folder(model, lq, gt, 2, device="cpu", verbose=False, usm_gt=True) == usm["val"][0][1]
