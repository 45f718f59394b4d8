"""CPU tests of the blind-SR degradation (bsr_degrade.py): the float64 restatements of ``cv_resize`` and ``blur_items`` (the yardstick
of the two kernels), the host blur kernels, the draws, the noise forms, the rule table with ``degrade`` and the C ABI's two argument
blocks.

Yardsticks: torch's float64 ``F.interpolate`` (bilinear / bicubic, ``align_corners=False``, which is OpenCV's sampling rule with the
same A = -0.75), ``avg_pool2d`` and ``repeat_interleave`` for INTER_AREA at integer factors, and tests/golden/tasks/degrade.npz
(tools/make_golden_degrade.py: scipy's ``ndimage.convolve(mode="mirror")`` in float64 and ``multivariate_normal.pdf``).  OpenCV is not
available; nothing here claims equality with its bytes.  The float64 paths are asked for 1e-12.

The bounds of the fp32 kernels, used by tests/test_gpu_degrade.py, with u = 2^-24 and inputs in [0, 1]:
  * ``resize_bound``: an output is chain_y(wy * fl32(chain_x(wx * x))) with n_x and n_y taps.  Rounding every weight to fp32 moves a
    pass by at most u sum|w| max|in|; an n-term fmaf chain by at most gamma_n sum|w| max|in| <= (n + 0.01) u sum|w| max|in|.  With
    S = sum|w| per axis (1 for linear and area, at most 1.375 for cubic at t = 0.5) the horizontal pass is off by at most
    (n_x + 1.01) u S, which the vertical pass carries with gain S, and the vertical pass adds (n_y + 1.01) u S * S (its inputs are at
    most S).  Together (n_x + n_y + 2.02) u S^2 <= (n_x + n_y + 8) u for S = 1 and, as S^2 <= 1.9, <= 2 (n_x + n_y + 8) u for cubic:
    the bound the issue sets.  The float64 yardstick itself is exact to 1e-15.
  * ``blur_bound``: tests/test_blur.py's ``bound``: (K^2 + 2) u for a K^2-term fmaf chain with positive taps of sum 1 (+- K^2 u / 2
    after their rounding to fp32, inside the + 2).
"""
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from grl_image_restoration_amd import PatchSampler, PatchStore, _lib, bsr_degrade as B, data as D, evaluate as EV, task_rules as R, train
from tests.test_blur import bound as blur_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U24 = 2.0 ** -24


def resize_bound(interp, h, w, ho, wo):
    ny, nx = B.resize_taps(interp, h, w, ho, wo)
    return (nx + ny + 8) * U24 * (2 if interp == B.INTER_CUBIC else 1)


class Fixture:
    def __init__(self):
        z = np.load(os.path.join(ROOT, "tests", "golden", "tasks", "degrade.npz"), allow_pickle=False)
        self.meta = json.loads(str(z["meta"]))
        self.blur = {}
        for name, c in self.meta["blur"].items():
            k = z[f"{name}__k"]
            self.blur[name] = dict(x=torch.from_numpy(z[f"{name}__x"]), k=k, taps=torch.from_numpy(np.flip(k).copy()),
                                   stride=c["stride"], K=c["K"], out=z[f"{name}__out"])
        self.kernels = [(m, z[f"kernel_{n}"]) for n, m in enumerate(self.meta["kernels"])]


_FX = []


def fixture():
    """Loaded once, shared with the GPU tests."""
    if not _FX:
        _FX.append(Fixture())
    return _FX[0]


@pytest.fixture(scope="module")
def fx():
    return fixture()


# ---- cv_resize --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(9, 13), (74, 106), (37, 53), (20, 80), (50, 7)])
def test_cpu_resize_linear_and_cubic_equal_interpolate(size):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(3, 37, 53, generator=g, dtype=torch.float64)
    lin, cub = B.cv_resize([x, x], [size, size], [B.INTER_LINEAR, B.INTER_CUBIC])
    for got, mode in ((lin, "bilinear"), (cub, "bicubic")):
        want = F.interpolate(x[None], size=size, mode=mode, align_corners=False)[0]
        err = float((got - want).abs().max())
        print(f"{mode} 37x53 -> {size}: {err:.2e}")
        assert got.dtype == torch.float64 and got.shape == want.shape and err <= 1e-12


def test_cpu_resize_area_at_integer_factors():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(3, 36, 48, generator=g, dtype=torch.float64)
    down3, down_mixed, up2, up_mixed = B.cv_resize([x] * 4, [(12, 16), (18, 12), (72, 96), (36, 144)], [B.INTER_AREA] * 4)
    assert float((down3 - F.avg_pool2d(x[None], 3)[0]).abs().max()) <= 1e-12
    assert float((down_mixed - F.avg_pool2d(x[None], (2, 4))[0]).abs().max()) <= 1e-12
    assert float((up2 - x.repeat_interleave(2, 1).repeat_interleave(2, 2)).abs().max()) <= 1e-12
    assert float((up_mixed - x.repeat_interleave(3, 2)).abs().max()) <= 1e-12
    # a fractional factor keeps the mean (every source pixel is covered once) and the weights of an output sum to 1
    frac = B.cv_resize([x], [(13, 17)], [B.INTER_AREA])[0]
    assert abs(float(frac.mean() - x.mean())) <= 1e-12
    for n, no in ((36, 13), (48, 17), (400, 51)):
        W = B._axis_matrix(n, no, "area_table")
        assert float((W.sum(1) - 1).abs().max()) <= 1e-12 and float((W.sum(0) * n / no - 1).abs().max()) <= 1e-12


def test_cpu_resize_edges_and_refusals():
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(3, 1, 9, generator=g), torch.rand(3, 8, 1, generator=g)
    for ip in (1, 2, 3):
        oa, ob = B.cv_resize([a, b], [(1, 4), (3, 1)], [ip, ip])
        assert oa.shape == (3, 1, 4) and ob.shape == (3, 3, 1) and oa.dtype == torch.float32
        assert float(oa.min()) >= float(a.min()) - 0.2 and float(oa.max()) <= float(a.max()) + 0.2
    same = B.cv_resize([a], [(1, 9)], [2])[0]
    assert torch.equal(same, a)
    with pytest.raises(ValueError):
        B.cv_resize([a], [(1, 4)], [0])
    with pytest.raises(ValueError):
        B.cv_resize([a], [(0, 4)], [1])
    with pytest.raises(ValueError):
        B.cv_resize([a, torch.rand(1, 4, 4)], [(1, 4), (2, 2)], [1, 1])
    with pytest.raises(ValueError):
        B.cv_resize([], [], [])


# ---- blur_items -------------------------------------------------------------------------------------------------------------------
def test_cpu_blur_items_on_the_fixture(fx):
    names = list(fx.blur)
    for C in (1, 3):
        group = [n for n in names if fx.blur[n]["x"].shape[0] == C]
        outs = B.blur_items([fx.blur[n]["x"].double() for n in group], [fx.blur[n]["taps"].double() for n in group],
                            [fx.blur[n]["stride"] for n in group])
        for n, o in zip(group, outs):
            err = np.abs(o.numpy() - fx.blur[n]["out"]).max()
            print(f"{n}: {err:.2e}")
            assert o.shape == fx.blur[n]["out"].shape and err <= 1e-12
    c = fx.blur["k7"]
    wrong = B.blur_items([c["x"].double()], [torch.from_numpy(c["k"].copy()).double()], [1])[0]      # the unflipped kernel
    assert np.abs(wrong.numpy() - c["out"]).max() > 1e-3
    o32 = B.blur_items([c["x"]], [c["taps"]], [1])[0]
    assert o32.dtype == torch.float32 and np.abs(o32.double().numpy() - c["out"]).max() <= 2 * U24
    for bad in (dict(taps=[torch.rand(4, 4)]), dict(taps=[torch.rand(33, 33)]), dict(strides=[0]), dict(taps=[torch.rand(3, 5)])):
        with pytest.raises(ValueError):
            B.blur_items([c["x"]], bad.get("taps", [c["taps"]]), bad.get("strides", [1]))


# ---- the host kernels -------------------------------------------------------------------------------------------------------------
def test_host_kernels(fx):
    for m, want in fx.kernels:
        got = B.anisotropic_gaussian(m["ksize"], m["theta"], m["l1"], m["l2"])
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * want.max() + 1e-15
    from grl_image_restoration_amd import tasks as T

    assert np.array_equal(B.fspecial_gaussian(25, 1.6), T.gaussian_blur_kernel(25, 1.6).numpy())
    k = np.random.RandomState(0).rand(9, 9)
    for sf, shift in ((2, 0.5), (4, 1.5)):
        got = B.shift_kernel(k, sf)
        want = np.zeros_like(k)
        for i in range(9):
            for j in range(9):
                y, x = min(i + shift, 8.0), min(j + shift, 8.0)
                y0, x0 = int(np.floor(y)), int(np.floor(x))
                y1, x1, ty, tx = min(y0 + 1, 8), min(x0 + 1, 8), y - np.floor(y), x - np.floor(x)
                want[i, j] = (k[y0, x0] * (1 - tx) + k[y0, x1] * tx) * (1 - ty) + (k[y1, x0] * (1 - tx) + k[y1, x1] * tx) * ty
        assert np.abs(got - want).max() <= 1e-14
    assert np.array_equal(B.shift_kernel(k, 1), k)
    assert np.array_equal(B._taps32(k).numpy(), T.blur_taps(k).numpy())


# ---- the draws --------------------------------------------------------------------------------------------------------------------
def _plain(plan):
    return [{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in op.items()} for op in plan]


def test_draw_plan_is_a_pure_function_of_the_rng_state():
    a, b = random.Random(7), random.Random(7)
    for scale in (4, 2, 4):
        assert _plain(B.draw_plan(a, scale, 64)) == _plain(B.draw_plan(b, scale, 64))
    assert a.getstate() == b.getstate()
    # ``stages`` leaves the stream alone: the same draws, fewer ops
    full, part = B.draw_plan(a, 4, 64), B.draw_plan(b, 4, 64, stages=(0, 1, 5, 6))
    assert a.getstate() == b.getstate()
    keep = [op for op in _plain(full) if op["stage"] in (-1, 0, 1, 5, 6, 9)]
    assert _plain(part) == keep and len(part) < len(full)
    for bad in (dict(scale=3), dict(crop=66), dict(crop=12), dict(stages=(9,))):
        with pytest.raises(ValueError):
            B.draw_plan(a, bad.get("scale", 4), bad.get("crop", 64), bad.get("stages"))


def test_draw_plan_shapes_orders_and_coverage():
    rng = random.Random(0)
    seen = set()
    for n in range(200):
        scale = (4, 2)[n % 2]
        plan = B.draw_plan(rng, scale, 64)
        pos = {op["stage"]: op["pos"] for op in plan}
        assert pos[1] < pos[6], "stage 6 follows stage 1"
        assert [op["pos"] for op in plan] == sorted(op["pos"] for op in plan)
        assert plan[-1]["op"] == "jpeg_final" and plan[-1]["size"] == 64 // scale and 20 <= plan[-1]["quality"] <= 95
        assert 2 not in pos, "the camera-noise stage is not built"
        size = 64
        for op in plan:
            if op["op"] == "blur":
                K = op["kernel"].shape[0]
                assert K % 2 == 1 and 7 <= K <= 25 and abs(op["kernel"].sum() - 1) <= 1e-12 and -(-size // op["stride"]) == op["size"]
            elif op["op"] not in ("resize", "imresize_half"):
                assert op["size"] == size
            assert op["size"] >= 1
            size = op["size"]
        assert size == 64 // scale
        seen |= {(op["stage"], op["op"], op.get("form"), op.get("interp")) for op in plan}
    want = {(-1, "resize"), (-1, "imresize_half"), (0, "blur"), (1, "resize"), (1, "blur"), (3, "gauss"), (4, "jpeg"), (5, "blur"),
            (6, "resize"), (7, "speckle"), (8, "poisson"), (9, "jpeg_final")}
    assert want <= {s[:2] for s in seen}
    for stage in (3, 7):
        assert {s[2] for s in seen if s[0] == stage and s[2]} == {"pixel", "gray", "corr"}
    for stage in (1, 6):
        assert {s[3] for s in seen if s[0] == stage and s[3]} == {1, 2, 3}


# ---- the noise forms --------------------------------------------------------------------------------------------------------------
def test_noise_forms():
    x = torch.full((3, 64, 64), 0.5)
    g = torch.Generator().manual_seed(0)
    level = 20
    d = B.add_noise(x, dict(op="gauss", level=level, form="pixel"), g) - x
    assert abs(float(d.std()) / (level / 255) - 1) <= 0.10 and abs(float(d.mean())) <= 0.1 * level / 255
    d = B.add_noise(x, dict(op="gauss", level=level, form="gray"), g) - x
    assert torch.equal(d[0], d[1]) and torch.equal(d[0], d[2]) and abs(float(d[0].std()) / (level / 255) - 1) <= 0.10
    corr = B._corr_noise(random.Random(5))
    cov = np.array(corr["cov"])
    assert np.allclose(cov, cov.T) and np.all(np.linalg.eigvalsh(cov) >= -1e-12) and cov.max() <= (25 / 255) ** 2
    d = (B.add_noise(x, dict(op="gauss", level=level, form="corr", **corr), g) - x).reshape(3, -1).double().numpy()
    sample = d @ d.T / d.shape[1]
    print("requested diagonal", np.diag(cov), "sample", np.diag(sample))
    assert np.all(np.abs(np.diag(sample) / np.diag(cov) - 1) <= 0.25)
    # speckle: the same three forms times the image
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    ramp = torch.linspace(0.1, 0.9, 3 * 64 * 64).view(3, 64, 64)
    for form in ("pixel", "gray", "corr"):
        op = dict(level=level, form=form, **(corr if form == "corr" else {}))
        add = B.add_noise(ramp, dict(op="gauss", **op), g1) - ramp
        mul = B.add_noise(ramp, dict(op="speckle", **op), g2) - ramp
        assert float((mul - ramp * add).abs().max()) <= 1e-6
    p = B.add_noise(x, dict(op="poisson", vals=10 ** 2.5), g)
    assert abs(float(p.mean()) / 0.5 - 1) <= 0.02 and float(p.std()) > 0
    k = p * 10 ** 2.5
    assert float((k - k.round()).abs().max()) <= 1e-3


# ---- the pipeline on the CPU ------------------------------------------------------------------------------------------------------
def test_apply_plans_on_the_cpu():
    from grl_image_restoration_amd import tasks as T

    rng = random.Random(11)
    plans = [B.draw_plan(rng, 4, 64) for _ in range(4)]
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(0))
    run = lambda seed: B.apply_plans(x, plans, torch.Generator().manual_seed(seed), parts=True)
    out, pre, q = run(1)
    assert out.shape == (4, 3, 16, 16) and out.dtype == torch.float32 and 0 <= float(out.min()) and float(out.max()) <= 1
    assert torch.equal((out * 255).round() / 255, out) and q.tolist() == [p[-1]["quality"] for p in plans]
    assert torch.equal(out, T.jpeg_roundtrip(pre, q)) and 0 <= float(pre.min()) and float(pre.max()) <= 1
    again = run(1)
    assert torch.equal(again[0], out) and torch.equal(again[1], pre)
    assert not torch.equal(run(2)[1], pre)
    assert torch.equal(B.apply_plans(x, plans, torch.Generator().manual_seed(1)), out)
    # a sample's result does not depend on its neighbours when no noise is drawn
    quiet = [B.draw_plan(rng, 2, 64, stages=(0, 1, 4, 5, 6)) for _ in range(3)]
    all3 = B.apply_plans(x[:3], quiet)
    assert all3.shape == (3, 3, 32, 32)
    for b in range(3):
        assert torch.equal(B.apply_plans(x[b : b + 1], quiet[b : b + 1])[0], all3[b])
    with pytest.raises(ValueError):
        B.apply_plans(x[:2], plans)
    with pytest.raises(ValueError):
        B.apply_plans(x[:2], [B.draw_plan(rng, 4, 64, stages=(0,)), B.draw_plan(rng, 4, 64)])      # two final sizes


# ---- rules, sampler, command line -------------------------------------------------------------------------------------------------
def test_rules_and_task_tuples_are_unchanged():
    assert tuple(R.RULES) == EV.TASKS == ("sr", "dn", "dm", "sr_bicubic", "bsr", "db", "jpeg")
    assert D.TASKS == ("sr", "sr_bicubic", "dn", "dm", "db", "jpeg")
    assert [t for t, r in R.RULES.items() if r.degrade] == ["sr"] and not R.RULES["bsr"].trainable
    assert R.TaskRule("x").degrade is False


def test_resolve_with_degrade_both_ways():
    ok = R.resolve("sr", "sampler", scale=4, degrade=True, patch=64)
    assert ok.degrade_crop == 400 and ok.scale == 4
    assert R.resolve("sr", "train", scale=2, degrade=True, degrade_crop=128, patch=64).degrade_crop == 128
    assert R.resolve("sr", "train", degrade=True).scale == 4
    assert R.resolve("sr", "sampler", scale=4, lq=True).degrade_crop is None
    refused = [dict(task="sr", lq=True), dict(task="sr", scale=3), dict(task="sr", scale=1), dict(task="sr", degrade_crop=66),
               dict(task="sr", degrade_crop=12), dict(task="sr", patch=101), dict(task="sr", degrade_crop=64, patch=17),
               dict(task="sr", channels=1), dict(task="sr_bicubic"), dict(task="dn", sigma=25), dict(task="jpeg", quality=10)]
    for kw in refused:
        kw = dict(dict(scale=4), **kw)
        with pytest.raises(ValueError):
            R.resolve(kw.pop("task"), "sampler", degrade=True, **kw)
    with pytest.raises(ValueError):
        R.resolve("sr", "evaluate", lq=True, degrade=True)
    with pytest.raises(ValueError):
        R.resolve("sr", "sampler", lq=True, degrade_crop=128)              # the crop without degrade
    with pytest.raises(ValueError):
        R.resolve("sr", "sampler", scale=4)                                # without degrade an LQ store is still required
    with pytest.raises(ValueError):
        R.resolve("sr", "train", scale=4, degrade=True, val=True)          # validation still reads an LQ / GT folder pair


def _store(sizes=((70, 80), (64, 96), (90, 64)), seed=0):
    g = np.random.RandomState(seed)
    return [g.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]


def test_sampler_with_degrade_on_the_cpu():
    from grl_image_restoration_amd import tasks as T

    images = _store()
    make = lambda **kw: PatchSampler("sr", PatchStore(images), degrade=True, degrade_crop=64, patch=8, scale=4, batch=4, seed=3, **kw)
    s, twin = make(), make()
    work, extras = s.draw()
    work2, extras2 = twin.draw()
    assert work2 == work and [(_plain(p), r, c) for p, r, c in extras2] == [(_plain(p), r, c) for p, r, c in extras]
    assert len(extras) == 4 and all(0 <= r <= 8 and 0 <= c <= 8 and p[-1]["size"] == 16 for p, r, c in extras)
    state = s.rng_state()
    lq, gt = s.next(work, extras)
    assert lq.shape == (4, 3, 8, 8) and gt.shape == (4, 3, 32, 32)
    crops = s.gt_store.sample(torch.tensor(work, dtype=torch.int32), 64, 1)
    gen = torch.Generator().set_state(state["noise"])
    full = B.apply_plans(crops, [e[0] for e in extras], gen)
    for b, (_, r, c) in enumerate(extras):
        assert torch.equal(gt[b], crops[b, :, 4 * r : 4 * r + 32, 4 * c : 4 * c + 32])
        assert torch.equal(lq[b], full[b, :, r : r + 8, c : c + 8])
    # the state carries the draws and the generator: the twin continues where ``s`` stood
    twin.set_rng_state(state)
    lq2, gt2 = twin.next(work, extras)
    assert torch.equal(lq2, lq) and torch.equal(gt2, gt)
    a, b = s.next(), twin.next()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[1], gt)
    # with usm the sharpened crop is the input of the degradation and the target
    u = make(usm=True)
    assert u.gt_store.dims == s.gt_store.dims and torch.equal(u.gt_store.data, s.gt_store.data)
    work, extras = u.draw()
    state = u.rng_state()
    lq, gt = u.next(work, extras)
    sharp = T.usm_sharp(u.gt_store.sample(torch.tensor(work, dtype=torch.int32), 64, 1))
    full = B.apply_plans(sharp, [e[0] for e in extras], torch.Generator().set_state(state["noise"]))
    for b, (_, r, c) in enumerate(extras):
        assert torch.equal(gt[b], sharp[b, :, 4 * r : 4 * r + 32, 4 * c : 4 * c + 32])
        assert torch.equal(lq[b], full[b, :, r : r + 8, c : c + 8])
    with pytest.raises(ValueError):
        PatchSampler("sr", PatchStore(_store(((70, 80), (60, 96)))), degrade=True, degrade_crop=64, patch=8, scale=4)   # too small
    with pytest.raises(ValueError):
        PatchSampler("sr", PatchStore(images), PatchStore(images), degrade=True, degrade_crop=64, patch=8, scale=4)
    with pytest.raises(ValueError):
        PatchSampler("dn", PatchStore(images), degrade=True, sigma=25, patch=8)
    with pytest.raises(ValueError):
        s.next(work)


def test_train_command_line_takes_degrade_for_sr_only(tmp_path, capsys):
    def tr(*extra):
        ap = train._parser()
        a = ap.parse_args(["--gt", str(tmp_path), "--steps", "1", "--device", "cpu", *extra])
        train._check(ap, a)
        return a

    for extra in (["--task", "sr", "--degrade", "--lq", str(tmp_path)], ["--task", "sr", "--degrade", "--scale", "3"],
                  ["--task", "sr", "--degrade-crop", "128", "--lq", str(tmp_path)], ["--task", "dn", "--sigma", "25", "--degrade"],
                  ["--task", "sr_bicubic", "--degrade"], ["--task", "sr", "--degrade", "--patch", "101"],
                  ["--task", "sr", "--degrade", "--channels", "1"], ["--task", "sr"]):
        with pytest.raises(SystemExit) as e:
            tr(*extra)
        assert e.value.code == 2, extra
    capsys.readouterr()
    a = tr("--task", "sr", "--degrade")
    assert a.degrade and a.degrade_crop == 400 and a.scale == 4
    a = tr("--task", "sr", "--degrade", "--degrade-crop", "128", "--scale", "2", "--usm")
    assert a.degrade_crop == 128 and a.usm
    a = tr("--task", "sr", "--lq", str(tmp_path))
    assert not a.degrade and a.degrade_crop is None


def test_train_and_the_frozen_set_on_the_cpu(tmp_path, capsys):
    """The smoke run of the feature on the CPU: a frozen validation set from ``python -m ...bsr_degrade``, then two eager steps of a
    one-block Tiny model on a folder of three generated images, validated on the frozen set."""
    from PIL import Image

    (tmp_path / "gt").mkdir()
    for n, im in enumerate(_store(((72, 80), (64, 100), (96, 64)), seed=4)):
        Image.fromarray(im).save(tmp_path / "gt" / f"im{n}.png")
    gt = str(tmp_path / "gt")
    frozen = str(tmp_path / "frozen")
    stems = B.main(["--gt", gt, "--out", frozen, "--scale", "4", "--seed", "2", "--crop", "64", "--device", "cpu"])
    assert stems == ["im0", "im1", "im2"]
    for s in stems:
        lq, g = np.asarray(Image.open(os.path.join(frozen, "LQ", s + ".png"))), np.asarray(Image.open(os.path.join(frozen, "GT", s + ".png")))
        assert lq.shape == (16, 16, 3) and g.shape == (64, 64, 3)
    src = np.asarray(Image.open(tmp_path / "gt" / "im0.png"))
    assert np.array_equal(np.asarray(Image.open(os.path.join(frozen, "GT", "im0.png"))), src[4:68, 8:72])
    again = str(tmp_path / "frozen2")
    B.main(["--gt", gt, "--out", again, "--scale", "4", "--seed", "2", "--crop", "64", "--device", "cpu"])
    assert np.array_equal(np.asarray(Image.open(os.path.join(again, "LQ", "im1.png"))), np.asarray(Image.open(os.path.join(frozen, "LQ", "im1.png"))))
    args = ["--task", "sr", "--degrade", "--degrade-crop", "64", "--scale", "4", "--model", "tiny", "--geometry", "yaml", "--depths", "1",
            "--patch", "8", "--batch", "2", "--eager", "--device", "cpu", "--gt", gt, "--steps", "2", "--seed", "3",
            "--val-gt", os.path.join(frozen, "GT"), "--val-lq", os.path.join(frozen, "LQ"), "--val-every", "2", "--out", str(tmp_path / "run")]
    torch.manual_seed(0)
    out = train.main(args)
    capsys.readouterr()
    assert len(out["losses"]) == 2 and all(np.isfinite(out["losses"])) and len(out["val"]) == 1 and np.isfinite(out["val"][0][1])
    ck = torch.load(out["checkpoint"], map_location="cpu", weights_only=False)
    assert ck["sampler_rng"]["noise"] is not None and ck["args"]["degrade"] and ck["args"]["degrade_crop"] == 64
    torch.manual_seed(0)
    usm = train.main(args[:-2] + ["--usm"])
    capsys.readouterr()
    assert usm["work"] == out["work"] and usm["losses"] != out["losses"]


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_args_layout_matches_header_and_abi():
    """The layouts of GrlCvResizeArgs and GrlBlurItemsArgs are compared with the header in tests/test_abi.py, like every struct's;
    what is particular to this entry point stays here."""
    assert _lib.ABI_VERSION >= 32
    assert "grl_cv_resize" in _lib.EXPORTS and "grl_blur_items" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "grl_hip.h")).read()
    assert "utils_sisr.py:350-354" in header and "utils_sisr.py:359-362" in header and "VOUCHES" in header
