"""The non-blind deblurring front end on the CPU (tasks.py, data.py, the two CLIs) against what the reference's own functions produce
(tests/golden/tasks/db.npz, written by tools/make_golden_db.py): the Gaussian kernel, the flipped fp32 taps, the kernel files, the
validation noise, the CPU blur against the engine's fp32 and float64 LQ, the C-ABI struct, the task lists and the db sampler.

The error bound.  An output is ``fl32(sum_i w_i x_i) + noise`` over n = K^2 taps.  A chain of n fp32 fmaf carries one rounding per
term: its forward error is at most gamma_n sum|w_i x_i| with gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability,
3.1).  The blur kernels are non-negative and sum to 1, so sum|w_i x_i| <= max|x|, and n u <= 729 * 2^-24 = 4.4e-5 makes
gamma_n <= (n + 0.04) u.  The final add of the noise rounds once more: at most u |out|, and |out| <= 1.03 for images in [0, 1] with
noise at sigma 2.  Together: |err| <= (K^2 + 2) 2^-24 max(1, max|x|).  The CPU path sums in float64 and rounds once, so it sits
within an fp32 ulp of the float64 LQ; the bound is the one the fp32 device kernel is held to as well.  The reference's own fp32 LQ
carries the same error, so against it twice the bound is allowed."""
import os
import random

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import PatchSampler, PatchStore, _lib, data as D, evaluate as EV, tasks as T, train
from tests.test_tasks import golden

LEVIN = {"real4": "levin_4", "real5": "levin_5"}


def bound(K, x):
    return (K * K + 2) * 2.0 ** -24 * max(1.0, float(x.abs().max()))


def db_cases(pad=None):
    return [c["name"] for c in golden("db")[0]["cases"] if pad is None or c["pad"] == pad]


_CASES = {}


def db_case(name):
    """(case meta, gt fp32 in [0, 1], taps fp32, noise, reference fp32 LQ, float64 LQ), loaded once and shared with the GPU tests."""
    if name not in _CASES:
        meta, z = golden("db")
        c = next(c for c in meta["cases"] if c["name"] == name)
        _CASES[name] = (c, z[f"{name}__gt"].float() / 255, z[f"taps_{c['kernel']}"], z[f"{name}__noise"], z[f"{name}__lq32"],
                        z[f"{name}__lq64"])
    return _CASES[name]


def check_lq(got, name, what=""):
    """``got`` (fp32, on any device) against the float64 LQ within the bound and the reference's fp32 LQ within twice it; returns
    the error against the float64 LQ."""
    c, gt, taps, _, lq32, lq64 = db_case(name)
    b = bound(taps.shape[0], gt)
    got = got.cpu()
    assert got.dtype == torch.float32 and got.shape == lq64.shape, (name, what, got.shape)
    e64, e32 = float((got.double() - lq64).abs().max()), float((got - lq32).abs().max())
    print(f"{name} {what}: |err| vs float64 {e64:.3e}, vs reference fp32 {e32:.3e}, bound {b:.3e}")
    assert e64 <= b and e32 <= 2 * b, (name, what, e64, e32, b)
    return e64


def test_gaussian_kernel_and_taps_are_the_reference():
    meta, z = golden("db")
    k = T.gaussian_blur_kernel()
    assert k.dtype == torch.float64 and k.shape == (25, 25)
    assert float((k - z["gaussian"]).abs().max()) <= 1e-15
    assert torch.equal(T.load_blur_kernel("gaussian"), k)
    assert meta["levin_sizes"] == [19, 17, 15, 27, 13, 21, 23, 23]
    for name, kernel in (("gaussian", k), ("real4", z["levin_4"]), ("real5", z["levin_5"])):
        taps, want = T.blur_taps(kernel), z[f"taps_{name}"]
        assert taps.dtype == torch.float32 and taps.shape == want.shape
        assert bool(((taps - want).abs() <= torch.from_numpy(np.spacing(want.abs().numpy()))).all()), name
        assert torch.equal(T.blur_taps(kernel.numpy()), taps)
    for name in ("real4", "real5"):                                           # the flip is observable on these
        want = z[f"taps_{name}"]
        assert not torch.equal(want, want.flip(0, 1)) and not torch.equal(want, want.flip(0)) and not torch.equal(want, want.flip(1))
        assert torch.equal(T.blur_taps(z[LEVIN[name]]), T.blur_taps(z[LEVIN[name]].flip(0, 1)).flip(0, 1))


def test_load_blur_kernel_reads_both_layouts(tmp_path):
    _, z = golden("db")
    levin = np.empty((1, 8), dtype=object)
    for i in range(8):
        levin[0, i] = z[f"levin_{i + 1}"].numpy()
    both = tmp_path / "Levin09.npy"
    np.save(both, levin, allow_pickle=True)
    for i in range(8):
        assert torch.equal(T.load_blur_kernel(f"real{i + 1}", str(both)), z[f"levin_{i + 1}"])
    plain = tmp_path / "k5.npy"
    np.save(plain, z["levin_5"].numpy())
    assert torch.equal(T.load_blur_kernel("real5", str(plain)), z["levin_5"])
    np.save(tmp_path / "k5f.npy", z["levin_5"].numpy().astype(np.float32))   # another float type of the plain layout
    assert T.load_blur_kernel("real5", str(tmp_path / "k5f.npy")).dtype == torch.float64
    with pytest.raises(ValueError):
        T.load_blur_kernel("real9", str(both))
    with pytest.raises(ValueError):
        T.load_blur_kernel("motion", str(both))
    with pytest.raises(ValueError):
        T.load_blur_kernel("real1")                                           # no file named
    with pytest.raises(OSError):
        T.load_blur_kernel("real1", str(tmp_path / "missing.npy"))
    np.save(tmp_path / "even.npy", np.ones((4, 4)) / 16)
    with pytest.raises(ValueError):
        T.load_blur_kernel("real1", str(tmp_path / "even.npy"))
    other = np.empty((2, 2), dtype=object)
    other[:] = 0
    np.save(tmp_path / "other.npy", other, allow_pickle=True)
    with pytest.raises(ValueError):
        T.load_blur_kernel("real1", str(tmp_path / "other.npy"))
    with pytest.raises(ValueError):
        T.blur_taps(np.ones((33, 33)))


def test_db_noise_is_the_reference_bit_for_bit():
    meta, z = golden("db")
    assert meta["sigma"] == 2
    for name in db_cases("same"):
        want = z[f"{name}__noise"]
        for n in range(want.shape[0]):                                        # seed 0 for every image: all of a batch are equal
            got = T.db_noise(want.shape[1:], meta["sigma"])
            assert got.dtype == torch.float32 and torch.equal(got, want[n]), name
    assert not torch.equal(T.db_noise((3, 8, 9), 2), T.db_noise((3, 8, 9), 3))


@pytest.mark.parametrize("name", db_cases())
def test_cpu_blur_matches_the_reference(name):
    c, gt, taps, noise, lq32, lq64 = db_case(name)
    K = taps.shape[0]
    if c["pad"] == "same":
        check_lq(T.db_lq(gt, taps, noise), name, "cpu db_lq")
        got = T.blur(gt, taps, "same", add=noise[0])                          # a (C, H, W) noise broadcasts over the batch
        assert torch.equal(got, T.db_lq(gt, taps, noise))
        with pytest.raises(ValueError):
            T.blur(gt, taps, "same", want_center=True)
    else:
        got, center = T.blur(gt, taps, "valid", add=noise, want_center=True)
        check_lq(got, name, "cpu valid")
        Ho, Wo = gt.shape[2] - K + 1, gt.shape[3] - K + 1
        assert center.is_contiguous() and torch.equal(center, gt[..., K // 2 : K // 2 + Ho, K // 2 : K // 2 + Wo])
        assert torch.equal((center * 255).round().to(torch.uint8), golden("db")[1][f"{name}__target"])
        same = T.blur(gt, taps, "same")                                       # the reference's order: blur with padding, then crop
        crop = same[..., K // 2 : K // 2 + Ho, K // 2 : K // 2 + Wo]           # two float64 sums, each rounded once: an fp32 ulp apart at most
        assert float((T.blur(gt, taps, "valid") - crop).abs().max()) <= 2.0 ** -23


def test_blur_argument_errors():
    x, taps = torch.rand(1, 3, 12, 12), torch.full((5, 5), 0.04)
    assert T.blur(x, taps, "valid").shape == (1, 3, 8, 8) and T.blur(x, taps).shape == x.shape
    with pytest.raises(ValueError):
        T.blur(x, torch.full((4, 4), 1 / 16.0))                               # even
    with pytest.raises(ValueError):
        T.blur(x, torch.full((33, 33), 1e-3))
    with pytest.raises(ValueError):
        T.blur(x, torch.full((13, 13), 1e-2), "valid")                        # H < K
    with pytest.raises(ValueError):
        T.blur(x, taps, "reflect")
    with pytest.raises(TypeError):
        T.blur(x.half(), taps)
    with pytest.raises(ValueError):
        T.blur(x[0], taps)
    one = torch.zeros(1, 1)
    one[0, 0] = 1.0
    assert torch.equal(T.blur(x, one), x)                                     # K = 1


def test_blur_args_layout_matches_header_and_abi():
    """The layout of GrlBlurArgs is compared with the header in tests/test_abi.py, like every struct's;
    what is particular to this entry point stays here."""
    assert _lib.ABI_VERSION >= 28
    assert "grl_blur_depthwise" in _lib.EXPORTS


def test_task_lists_and_cli_errors(tmp_path, capsys):
    assert "db" in EV.TASKS and "db" in D.TASKS
    gt = tmp_path / "gt"
    gt.mkdir()
    ev = ["--task", "db", "--gt", str(gt), "--device", "cpu"]
    for extra in (["--scale", "2"], ["--lq", str(gt)], ["--channels", "1"], ["--blur-kernel", "real3"],
                  ["--blur-kernel", "real9", "--blur-kernel-file", str(gt / "none.npy")],
                  ["--blur-kernel", "real3", "--blur-kernel-file", str(gt / "none.npy")]):
        with pytest.raises(SystemExit) as e:
            EV.main(ev + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit):
        EV.main(["--task", "dm", "--gt", str(gt), "--blur-kernel", "real3"])    # the option belongs to db
    with pytest.raises(ValueError, match="no images"):                          # accepted by the parser; the empty folder stops it
        EV.main(ev + ["--model", "tiny", "--geometry", "yaml"])
    with pytest.raises(ValueError):
        list(EV.task_inputs(str(gt), "db", channels=1, device="cpu"))
    tr = ["--task", "db", "--gt", str(gt), "--steps", "1", "--device", "cpu"]
    for extra in (["--scale", "2"], ["--lq", str(gt)], ["--channels", "1"], ["--sigma-range", "1", "3"], ["--blur-kernel", "real3"],
                  ["--blur-kernel", "gauss"], ["--val-lq", str(gt)]):
        with pytest.raises(SystemExit) as e:
            train.main(tr + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit):
        train.main(["--task", "dm", "--gt", str(gt), "--steps", "1", "--device", "cpu", "--blur-kernel-file", "k.npy"])
    ap = train._parser()
    a = ap.parse_args(tr)
    train._check(ap, a)
    assert a.sigma == 2.0 and a.scale == 1 and a.blur_kernel == "gaussian"      # db.yaml:8
    capsys.readouterr()


def test_task_inputs_db_on_the_cpu(tmp_path):
    """evaluate's db items from a folder: the crop to multiples of 8, the shared noise, the reference's LQ."""
    from PIL import Image

    c, gt, taps, noise, lq32, lq64 = db_case("g_40x56_b2")
    raw = golden("db")[1]["g_40x56_b2__gt"]
    odd = np.zeros((45, 61, 3), dtype=np.uint8)                                # cropped to 40 x 56
    odd[:40, :56] = raw[1].permute(1, 2, 0).numpy()
    Image.fromarray(raw[0].permute(1, 2, 0).numpy()).save(tmp_path / "a.png")
    Image.fromarray(odd).save(tmp_path / "b.png")
    items = list(EV.task_inputs(str(tmp_path), "db", device="cpu"))
    assert [n for n, _, _ in items] == ["a.png", "b.png"]
    for n, (_, lq, g) in enumerate(items):
        assert torch.equal(g, gt[n : n + 1]) and lq.shape == g.shape
        assert float((lq.double() - lq64[n : n + 1]).abs().max()) <= bound(25, gt)
    other = list(EV.task_inputs(str(tmp_path), "db", device="cpu", sigma=10, taps=golden("db")[1]["taps_real5"]))
    assert float((other[0][1] - items[0][1]).abs().max()) > 1e-2


SIZES = [(60, 70), (20, 50)]                       # with P = 16 and K = 13 (P' = 28) the second one is padded at the bottom


def _store_images():
    g = np.random.RandomState(21)
    return [g.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]


def test_db_sampler_on_a_cpu_store():
    _, z = golden("db")
    taps = z["taps_real5"]
    K, P, B, seed = taps.shape[0], 16, 5, 9
    Pp = P + K - 1
    imgs = _store_images()
    s = PatchSampler("db", PatchStore(imgs), patch=P, batch=B, taps=taps, sigma=2, seed=seed)
    assert s.draw_patch == Pp and s.sigma == 2.0
    # the draws use P': the reference's _random_index on the image padded to P'
    got, sigmas = s.draw()
    rng = random.Random(seed)
    want = []
    for _ in range(B):
        n = rng.randrange(len(imgs))
        x, y = rng.randrange(0, max(SIZES[n][0], Pp) - Pp + 1), rng.randrange(0, max(SIZES[n][1], Pp) - Pp + 1)
        want.append((n, x, y, sum(bit for bit in (1, 2, 4) if rng.random() < 0.5)))
    assert got == want and sigmas is None
    # an explicit list: the padded image, the last valid origin, flips
    work = [(1, 0, 0, 0), (1, 0, 22, 3), (0, 32, 42, 0), (0, 5, 7, 4), (0, 0, 0, 6)]
    s = PatchSampler("db", PatchStore(imgs), patch=P, batch=B, taps=taps, sigma=2, seed=seed)
    state = s.rng_state()
    lq, gt = s.next(work)
    big = PatchStore(imgs).sample(torch.tensor(work, dtype=torch.int32), Pp, 1)
    assert lq.shape == gt.shape == (B, 3, P, P) and lq.dtype == torch.float32
    assert float(big[0, :, 20:].abs().max()) == 0 and float(big[0, :, :20].abs().max()) > 0       # rows 20 .. 27 are padding
    assert torch.equal(gt, big[..., K // 2 : K // 2 + P, K // 2 : K // 2 + P])
    assert float(gt[0, :, 20 - K // 2 :].abs().max()) == 0                    # ... and reach the cropped target
    noise = torch.randn(B, 3, P, P, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    assert torch.equal(lq, T.blur(big, taps, "valid") + noise * (2 / 255))
    assert abs(float((lq - T.blur(big, taps, "valid")).std()) / (2 / 255) - 1) < 0.1
    # the generator is part of the state
    again = s.next(work)
    assert not torch.equal(again[0], lq) and torch.equal(again[1], gt)
    s.set_rng_state(state)
    back = s.next(work)
    assert torch.equal(back[0], lq)
    # noise handed in
    lq2, _ = s.next(work, noise=noise)
    assert torch.equal(lq2, lq)
    # argument checks
    with pytest.raises(ValueError):
        PatchSampler("db", PatchStore(imgs), patch=P, batch=B)                 # no taps
    with pytest.raises(ValueError):
        PatchSampler("db", PatchStore(imgs), patch=P, batch=B, taps=taps, sigma_range=(1, 3))
    with pytest.raises(ValueError):
        PatchSampler("db", PatchStore(imgs), patch=P, batch=B, taps=taps, scale=2)
    with pytest.raises(ValueError):
        PatchSampler("db", PatchStore(imgs), PatchStore(imgs), patch=P, batch=B, taps=taps)
    with pytest.raises(ValueError):
        PatchSampler("db", PatchStore([i[:, :, 0] for i in imgs]), patch=P, batch=B, taps=taps)
    with pytest.raises(ValueError):
        PatchSampler("dm", PatchStore(imgs), patch=P, batch=B, taps=taps)
    assert PatchSampler("db", PatchStore(imgs), patch=P, batch=B, taps=taps).sigma == 2.0


def test_train_cli_db_on_the_cpu(tmp_path, capsys):
    """One eager step and one validation of --task db on CPU tensors: the sampler, the loss and ``evaluate_folder(task="db")`` with
    the command's taps and sigma."""
    from PIL import Image

    g = np.random.RandomState(4)
    d = tmp_path / "gt"
    d.mkdir()
    for i in range(2):
        Image.fromarray(g.randint(0, 256, (32, 32, 3)).astype(np.uint8)).save(d / f"im{i}.png")
    np.save(tmp_path / "k5.npy", golden("db")[1]["levin_5"].numpy())
    torch.manual_seed(0)
    r = train.main(["--task", "db", "--blur-kernel", "real5", "--blur-kernel-file", str(tmp_path / "k5.npy"), "--model", "tiny",
                    "--geometry", "yaml", "--depths", "1", "--patch", "16", "--batch", "2", "--eager", "--device", "cpu", "--gt", str(d),
                    "--steps", "1", "--val-gt", str(d), "--val-every", "1", "--out", str(tmp_path / "run")])
    assert r["steps"] == [0] and np.isfinite(r["losses"][0]) and os.path.isfile(r["checkpoint"])
    assert all(x <= 32 - 28 and y <= 32 - 28 for _, x, y, _ in r["work"][0])                # the draws use P' = 16 + 12
    assert len(r["val"]) == 1 and r["val"][0][0] == 1 and np.isfinite(r["val"][0][1])
    obj = torch.load(r["checkpoint"], map_location="cpu", weights_only=False)
    assert obj["args"]["task"] == "db" and obj["args"]["sigma"] == 2.0 and obj["sampler_rng"]["noise"] is not None
    capsys.readouterr()
