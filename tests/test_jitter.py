"""The colour jitter of the blind-SR training branch on the CPU (grl_image_restoration_amd/jitter.py): the float64 restatement of
torchvision's ``ColorJitter.forward`` against Python's ``colorsys`` (the hue op) and against closed forms written out here (the
other three), its invariants, the draws, and the option through ``task_rules``, ``PatchSampler`` and the ``train`` command line.
torchvision is not installed where these tests run: nothing here, and nothing in tests/test_gpu_jitter.py, is a run of it.

``kernel_cases`` builds the item list of the GPU tests, and ``E_FP32`` is the worst deviation of torch's fp32 CPU evaluation of the
statement from its float64 evaluation on exactly those items -- the reference's own arithmetic, not the code under test --
measured once on the CPU and frozen; ``test_the_frozen_fp32_deviation`` measures it again.
"""
import colorsys
import itertools

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import PatchSampler, PatchStore, _lib, bsr_degrade as B, jitter as J, task_rules as R, tasks as T, train

ORDERS = list(itertools.permutations(range(4)))
CORNERS = [(0.8, 0.8, 0.8, -0.05), (1.2, 1.2, 1.2, 0.05), (1.0, 1.0, 1.0, 0.0)]
E_FP32 = 1.165e-6


def adversarial_pixels():
    """(N, 3) values on the k / 255 grid where the hue op branches: greys, near-greys (one channel 1 / 255 off), two equal maxima,
    two equal minima, black, white, primaries and secondaries."""
    px = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    for v in (1, 64, 128, 200, 254):
        px.append((v, v, v))
        for c in range(3):
            for d in (-1, 1):
                q = [v, v, v]
                q[c] += d
                px.append(tuple(q))
        for lo in (0, v // 2):
            px += [(v, v, lo), (v, lo, v), (lo, v, v), (v, lo, lo), (lo, v, lo), (lo, lo, v)]
    return np.asarray(px, dtype=np.float64) / 255.0


def image8(seed, h, w):
    """A (3, h, w) fp32 image on the k / 255 grid: colour ramps plus texture, with the adversarial pixels planted from the start."""
    g = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 255.0 * (x + y) / max(h + w - 2, 1)])
    im = np.clip(0.6 * base + 0.4 * g.randint(0, 256, (3, h, w)), 0, 255).astype(np.uint8).astype(np.float64) / 255.0
    adv = adversarial_pixels()
    n = min(len(adv), h * w)
    flat = im.reshape(3, -1)
    flat[:, :n] = adv[g.permutation(len(adv))[:n]].T
    return torch.from_numpy(flat.reshape(3, h, w).astype(np.float32))


def kernel_cases():
    """The items of the GPU tests: 24 of 3 x 19 x 23, one per order, then 3 x 1 x 1, 3 x 1 x 70, 3 x 64 x 64 and 3 x 33 x 130; every
    second of the 24 and two of the others carry a corner set of factors, the rest draws of ``draw_jitter``."""
    gen = torch.Generator().manual_seed(11)
    cases = []
    for i, order in enumerate(ORDERS):
        f = J.draw_jitter(gen)[1:] if i % 2 == 0 else CORNERS[(i // 2) % 3]
        cases.append(dict(x=image8(100 + i, 19, 23), params=(order, *f)))
    for i, ((h, w), order, f) in enumerate((((1, 1), (3, 0, 1, 2), None), ((1, 70), (2, 3, 0, 1), CORNERS[0]), ((64, 64), (0, 3, 2, 1), None),
                                            ((33, 130), (3, 2, 1, 0), None), ((33, 130), (2, 0, 3, 1), CORNERS[1]))):
        cases.append(dict(x=image8(200 + i, h, w), params=(order, *(f or J.draw_jitter(gen)[1:]))))
    return cases


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [-0.05, 0.05, 0.0173])
def test_hue_against_colorsys(shift):
    g = np.random.RandomState(3)
    px = np.concatenate([adversarial_pixels(), g.randint(0, 256, (200, 3)) / 255.0])
    assert len(px) >= 300
    got = J.hue(torch.from_numpy(px.T.copy()).reshape(3, 1, -1), shift)[:, 0].T.numpy()
    for p, out in zip(px, got):
        h, s, v = colorsys.rgb_to_hsv(*p)
        want = colorsys.hsv_to_rgb((h + shift) % 1.0, s, v)
        assert np.abs(out - np.asarray(want)).max() <= 1e-12, (p, out, want)


def test_brightness_contrast_saturation_against_closed_forms():
    x = image8(5, 17, 21).double()
    a = x.numpy()
    y = 0.2989 * a[0] + 0.587 * a[1] + 0.114 * a[2]
    for f in (0.8, 1.0, 1.2, 0.9371):
        assert np.abs(J.brightness(x, f).numpy() - np.clip(f * a, 0, 1)).max() <= 1e-12
        assert np.abs(J.contrast(x, f).numpy() - np.clip(f * a + (1 - f) * y.mean(), 0, 1)).max() <= 1e-12
        assert np.abs(J.saturation(x, f).numpy() - np.clip(f * a + (1 - f) * y[None], 0, 1)).max() <= 1e-12
    assert abs(float(J.contrast_mean(x)) - y.mean()) <= 1e-12


def test_invariants():
    x = image8(6, 19, 23).double()
    gen = torch.Generator().manual_seed(0)
    grey = torch.rand(1, 9, 11, generator=gen, dtype=torch.float64).expand(3, 9, 11).contiguous()
    for order in ORDERS:
        assert float((J.jitter_image(x, (order, 1.0, 1.0, 1.0, 0.0)) - x).abs().max()) <= 1e-12, order
        for f in CORNERS[:2] + [J.draw_jitter(gen)[1:]]:
            out = J.jitter_image(x, (order, *f))
            assert out.shape == x.shape and 0 <= float(out.min()) and float(out.max()) <= 1
            g = J.jitter_image(grey, (order, *f))
            assert float((g - g[:1]).abs().max()) <= 1e-12, "a grey image stays grey"
    # the list front end: new tensors, the means next to them, and its refusals
    out, means = J.color_jitter([x, grey], [(ORDERS[7], *CORNERS[0]), (ORDERS[3], *CORNERS[1])], with_means=True)
    assert torch.equal(out[0], J.jitter_image(x, (ORDERS[7], *CORNERS[0]))) and means.dtype == torch.float64 and means.shape == (2,)
    with pytest.raises(ValueError, match="permutation"):
        J.color_jitter([x], [((0, 1, 2, 2), 1.0, 1.0, 1.0, 0.0)])
    with pytest.raises(ValueError, match="one parameter set"):
        J.color_jitter([x, x], [(ORDERS[0], 1.0, 1.0, 1.0, 0.0)])
    with pytest.raises(ValueError, match=r"\(3, h, w\)"):
        J.color_jitter([x[:1]], [(ORDERS[0], 1.0, 1.0, 1.0, 0.0)])


def test_the_frozen_fp32_deviation():
    """E_FP32: torch's fp32 CPU evaluation of the statement against its float64 evaluation on the items of the GPU tests.
    The measurement has to reproduce the frozen constant to within a factor of two (summation orders differ between builds)."""
    worst = worst_mean = 0.0
    for c in kernel_cases():
        want, m64 = J.jitter_image(c["x"].double(), c["params"], with_mean=True)
        got, m32 = J.jitter_image(c["x"], c["params"], with_mean=True)
        assert got.dtype == torch.float32
        worst = max(worst, float((got.double() - want).abs().max()))
        worst_mean = max(worst_mean, abs(float(m32) - float(m64)))
    print(f"fp32 against float64 on the kernel cases: images {worst:.3e} (frozen {E_FP32:.3e}), means {worst_mean:.3e}")
    assert E_FP32 / 2 <= worst <= E_FP32 * 2 and worst_mean <= E_FP32


# ---- the draws -------------------------------------------------------------------------------------------------------------------
def test_draws_are_the_five_torch_calls():
    g, ref = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    seen = set()
    for _ in range(200):
        order, b, c, s, h = J.draw_jitter(g)
        want_order = torch.randperm(4, generator=ref)
        want = [float(torch.empty(1).uniform_(lo, hi, generator=ref)) for lo, hi in ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.05, 0.05))]
        assert list(order) == want_order.tolist() and [b, c, s, h] == want
        assert 0.8 <= b <= 1.2 and 0.8 <= c <= 1.2 and 0.8 <= s <= 1.2 and -0.05 <= h <= 0.05
        assert all(float(np.float32(v)) == v for v in (b, c, s, h)), "fp32 values"
        seen.add(tuple(order))
    assert seen == set(ORDERS)
    assert torch.equal(g.get_state(), ref.get_state())


# ---- the sampler -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store():
    g = np.random.RandomState(1)
    return PatchStore([g.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((70, 80), (64, 96), (90, 64))])


def _make(store, **kw):
    return PatchSampler("sr", store, degrade=True, degrade_crop=64, patch=8, scale=4, batch=4, seed=5, **kw)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_sampler_without_the_option_is_the_parents(store):
    for kw in (dict(), dict(usm=True, plain_gt=True)):
        a, b = _make(store, **kw), _make(store, jitter=False, **kw)
        for _ in range(2):
            assert _same(a.next(), b.next())
            sa, sb = a.rng_state(), b.rng_state()
            assert set(sa) == set(sb) == {"draws", "noise"} and sa["draws"] == sb["draws"] and torch.equal(sa["noise"], sb["noise"])
        assert not hasattr(b, "jitter_gen")


def _quiet_plans(seed, n):
    import random

    rng = random.Random(seed)
    return [B.draw_plan(rng, 4, 64, stages=(0, 1, 5, 6)) for _ in range(n)]          # blur and resize stages: no noise is drawn


def test_sampler_with_the_option(store):
    on, off = _make(store, jitter=True), _make(store)
    work, extras = on.draw()
    work_off, extras_off = off.draw()
    assert work == work_off and on.rng.getstate() == off.rng.getstate(), "the Python draw stream is untouched"
    assert all(len(e) == 4 and len(f) == 3 and e[1:3] == f[1:3] for e, f in zip(extras, extras_off))
    ref = torch.Generator().manual_seed(5)
    assert [e[3] for e in extras] == [J.draw_jitter(ref) for _ in range(4)], "one parameter set per sample, in sample order"
    on.next(work, extras), off.next(work_off, extras_off)
    assert on.rng.getstate() == off.rng.getstate()       # (the noise generator's stream depends on the pixels: Poisson noise)

    params = [e[3] for e in extras]
    plans = _quiet_plans(3, 4)
    places = [(b % 9, (2 * b) % 9) for b in range(4)]
    crops = store.sample(torch.tensor(work, dtype=torch.int32), 64, 1)
    want = torch.stack(J.color_jitter(list(crops), params))
    assert not torch.equal(want, crops)
    cut = lambda im, b: im[b, :, 4 * places[b][0] : 4 * places[b][0] + 32, 4 * places[b][1] : 4 * places[b][1] + 32]
    lq, gt = on.next(work, [(p, r, c, q) for p, (r, c), q in zip(plans, places, params)])
    full = B.apply_plans(want, plans, None)
    for b, (r, c) in enumerate(places):
        assert torch.equal(gt[b], cut(want, b)), "the target is the jittered crop"
        assert torch.equal(lq[b], full[b, :, r : r + 8, c : c + 8]), "the degradation's input is the jittered crop"
    # with usm and plain_gt all three outputs derive from the jittered crop
    three = _make(store, jitter=True, usm=True, plain_gt=True)
    lq, gt, plain = three.next(work, [(p, r, c, q) for p, (r, c), q in zip(plans, places, params)])
    sharp = T.usm_sharp(want)
    full = B.apply_plans(sharp, plans, None)
    for b, (r, c) in enumerate(places):
        assert torch.equal(plain[b], cut(want, b)) and torch.equal(gt[b], cut(sharp, b))
        assert torch.equal(lq[b], full[b, :, r : r + 8, c : c + 8])
    with pytest.raises(ValueError, match="with jitter"):
        on.next(work, [(p, r, c) for p, (r, c) in zip(plans, places)])


def test_sampler_state_continues_the_stream(store):
    s = _make(store, jitter=True)
    s.next(), s.next()
    state = s.rng_state()
    assert set(state) == {"draws", "noise", "jitter"}
    nxt = s.next()
    s.set_rng_state(state)
    assert _same(s.next(), nxt)
    fresh = _make(store, jitter=True)
    fresh.set_rng_state(state)
    assert _same(fresh.next(), nxt)
    other = _make(store, jitter=True)
    other.set_rng_state({k: v for k, v in state.items() if k != "jitter"})           # a checkpoint from before the option
    assert not _same(other.next(), nxt)


# ---- the option ------------------------------------------------------------------------------------------------------------------
def test_option_errors(store, tmp_path, capsys):
    assert R.resolve("sr", "train", scale=4, patch=8, degrade=True, degrade_crop=64, jitter=True).degrade_crop == 64
    for where, kw in (("train", dict(lq=True)), ("sampler", dict(lq=True)), ("evaluate", dict(lq=True))):
        with pytest.raises(ValueError, match="colour jitter.*belongs to training with degrade"):
            R.resolve("sr", where, scale=4, jitter=True, **kw)
    g = np.random.RandomState(0)
    with pytest.raises(ValueError, match="belongs to training with degrade"):
        PatchSampler("sr", PatchStore([g.randint(0, 256, (40, 40, 3)).astype(np.uint8)]),
                     PatchStore([g.randint(0, 256, (10, 10, 3)).astype(np.uint8)]), patch=4, scale=4, jitter=True)

    def tr(*extra):
        ap = train._parser()
        a = ap.parse_args(["--gt", str(tmp_path), "--steps", "1", "--device", "cpu", *extra])
        train._check(ap, a)
        return a

    for extra in (["--task", "sr", "--jitter", "--lq", str(tmp_path)], ["--task", "dn", "--sigma", "25", "--jitter"]):
        with pytest.raises(SystemExit) as e:
            tr(*extra)
        assert e.value.code == 2, extra
    assert "--degrade" in capsys.readouterr().err
    assert tr("--task", "sr", "--degrade", "--jitter").jitter and not tr("--task", "sr", "--degrade").jitter


def test_abi():
    assert "grl_color_jitter" in _lib.EXPORTS and "grl_color_jitter_num_workgroups" in _lib.EXPORTS and _lib.ABI_VERSION >= 38
