"""The camera-noise stage of the blind-SR degradation on the CPU: the bank's tables and the float64 restatement of ``isp`` against what
the reference's own modules computed (tests/golden/tasks/isp.npz, tools/make_golden_isp.py), the draws of ``draw_plan`` with a bank,
``apply_plans`` with the ``camera`` op, the targets of ``PatchSampler`` and the options."""
import hashlib
import os
import random

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import PatchSampler, PatchStore, bsr_degrade as B, isp, task_rules as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tasks", "isp.npz")

# The largest distance, over every value of the three recorded cases (raw plane, noisy LQ, HR round trip), between the float64
# restatement and the reference's fp32 outputs: 1.002e-5, measured when the fixture was made.  It is the fp32 rounding of the
# reference itself (the restatement run in fp32 is within 3.5e-6 of it).  The restatement is held to twice this figure; the kernels
# (tests/test_gpu_isp.py) to four times it against the float64 restatement.
REFERENCE_TO_RESTATEMENT = 1.002e-5


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def bank(golden):
    return isp.CameraBank.from_arrays(golden["forward1"], golden["forward2"], golden["curve_x"], golden["curve_y"])


def analytic_bank(jump_curve=None):
    """A bank that needs no scipy: the fixture's matrices, and for every curve the tables of y = t^0.8 and its inverse.  Curve
    ``jump_curve`` gets an inverse table with a jump of 1e-2 put in by hand at entry 600000, as the inverse tables of four of the
    reference's curves have them."""
    g = np.load(GOLDEN)
    t = torch.linspace(0, 1, isp.TABLE_N, dtype=torch.float64)
    smooth = torch.stack([t ** 0.8, t ** 1.25]).float()
    tables = {c: smooth for c in range(len(isp.CURVES))}
    if jump_curve is not None:
        inv = t ** 1.25
        inv[600000:] = (inv[600000:] + 1e-2).clamp(max=1.0)
        tables[jump_curve] = torch.stack([t ** 0.8, inv]).float()
    return isp.CameraBank.from_arrays(g["forward1"], g["forward2"], g["curve_x"], g["curve_y"], tables=tables)


def draws(seed, curve=None):
    """In-range draws of the stage for one sample."""
    r = random.Random(seed)
    d = dict(camera=r.randrange(11), curve=r.randrange(11) if curve is None else curve, fw=r.random(), d_r=1.2 + 1.2 * r.random(),
             d_b=1.2 + 1.2 * r.random(), e=0.2 * r.random() - 0.1)
    log_shot = r.uniform(-4, np.log10(0.006))
    d.update(shot=10 ** log_shot, read=10 ** (2.275 * log_shot + 1.47 + r.uniform(-0.5, 0.5)))
    return d


def image8(seed, h, w):
    """An 8-bit image as a (3, h, w) fp32 tensor on the k / 255 grid: colour ramps plus texture over 64 .. 255, one black and one
    white corner pixel.  No deep shadows besides the black pixel: where the linear value is below 1.1e-3, a step of the t^0.8
    table times the 12.92 of the sRGB curve's linear segment is larger than the kernels' bar, so that a table index one off --
    which the reference's own fp32 arithmetic has against float64 as well -- would show as a miss (tests/test_gpu_isp.py)."""
    g = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 255.0 * (x + y) / max(h + w - 2, 1)])
    im = np.clip(64 + 0.75 * (0.7 * base + 0.3 * g.randint(0, 256, (3, h, w))), 0, 255).astype(np.uint8)
    im[:, :1, :1], im[:, -1:, -1:] = 0, 255
    return torch.from_numpy(im.astype(np.float32) / 255.0)


def test_bank_tables_equal_the_references_sampled_entries(golden, bank):
    idx = torch.from_numpy(golden["table_idx"].astype(np.int64))
    for c in range(len(isp.CURVES)):
        t = bank.table(c)
        assert t.shape == (2, isp.TABLE_N) and t.dtype == torch.float32 and not bool(torch.isnan(t).any())
        assert torch.equal(t[0][idx[c]], torch.from_numpy(golden["table_yi"][c])), isp.CURVES[c]
        assert torch.equal(t[1][idx[c]], torch.from_numpy(golden["table_yi_inv"][c])), isp.CURVES[c]
    flat = bank.tables()
    assert flat.shape == (22 * isp.TABLE_N,) and torch.equal(flat[5 * isp.TABLE_N : 6 * isp.TABLE_N], bank.table(2)[1])


def _case(golden, bank, n, dtype):
    k = lambda s: golden[f"case{n}__{s}"]
    d = {s: float(k(s)) for s in ("fw", "d_r", "d_b", "e", "shot", "read")}
    p = bank.params(dict(d, camera=int(k("camera")), curve=int(k("curve"))))
    as_t = lambda a: torch.from_numpy(a.astype(np.float32) / 255.0).permute(2, 0, 1).to(dtype)
    return p, as_t(k("x")), as_t(k("hr")), torch.from_numpy(k("z"))


def test_float64_restatement_reproduces_the_reference(golden, bank):
    worst = 0.0
    for n in range(3):
        p, x, hr, z = _case(golden, bank, n, torch.float64)
        raw = isp.mosaic(isp.unprocess(x, p))
        (lq,), (hro,) = isp.camera_noise([x], [hr], [p], [z])
        assert lq.dtype == hro.dtype == torch.float64 and lq.shape == x.shape and hro.shape == hr.shape
        for name, got in (("raw", raw), ("out", lq), ("hr_out", hro)):
            want = torch.from_numpy(golden[f"case{n}__{name}"])
            err = float((got - want.double()).abs().max())           # over every value: none is left out
            print(f"case {n} {name} {tuple(want.shape)}: max|restatement - reference| = {err:.3e}")
            worst = max(worst, err)
    print(f"worst {worst:.3e}, bar {2 * REFERENCE_TO_RESTATEMENT:.3e}")
    assert worst <= 2 * REFERENCE_TO_RESTATEMENT


def test_fp32_restatement_is_the_references_arithmetic(golden, bank):
    for n in range(3):
        p, x, hr, z = _case(golden, bank, n, torch.float32)
        (lq,), (hro,) = isp.camera_noise([x], [hr], [p], [z])
        for got, name in ((lq, "out"), (hro, "hr_out")):
            assert float((got - torch.from_numpy(golden[f"case{n}__{name}"])).abs().max()) <= 2 * REFERENCE_TO_RESTATEMENT


def test_params_are_the_references_fp32_products(bank):
    d = draws(3)
    p = bank.params(d)
    rec = p.rec
    assert rec.shape == (isp.REC,) and rec.dtype == torch.float32 and p.curve == d["curve"] and p.bank is bank
    w1i, w2i, w2, w1 = (rec[9 * i : 9 * i + 9].view(3, 3) for i in range(4))
    eye = torch.eye(3)
    assert torch.allclose(w1 @ w1i, eye, atol=1e-5) and torch.allclose(w2 @ w2i, eye, atol=1e-5)
    fw = np.float32(d["fw"])
    mix = fw * bank.forward1[d["camera"]] + (1 - fw) * bank.forward2[d["camera"]]
    assert torch.allclose(w2, mix * torch.tensor([d["d_r"], 1.0, d["d_b"]]), atol=1e-6)
    # XYZ(D50) white -> linear sRGB white
    assert torch.allclose(w1 @ torch.tensor([0.96422, 1.0, 0.82521]), torch.ones(3), atol=2e-4)
    assert float(rec[36]) == pytest.approx(2 ** d["e"], rel=1e-6) and float(rec[36] * rec[37]) == pytest.approx(1.0, rel=1e-6)
    assert float(rec[38]) == pytest.approx(d["shot"], rel=1e-6) and float(rec[39]) == pytest.approx(d["read"], rel=1e-6)


def test_side_rule_and_list_checks(bank):
    p = bank.params(draws(1))
    with pytest.raises(ValueError, match="at least 3"):
        isp.camera_noise([torch.rand(3, 2, 8)], None, [p], [torch.zeros(2, 8)])
    with pytest.raises(ValueError, match="one params"):
        isp.camera_noise([torch.rand(3, 4, 4)], None, [p, p], [torch.zeros(4, 4)])
    with pytest.raises(ValueError, match=r"\(h, w\)"):
        isp.camera_noise([torch.rand(3, 4, 4)], None, [p], [torch.zeros(4, 5)])


# ---- the draws --------------------------------------------------------------------------------------------------------------------
def plan_hash(plan):
    """sha256 over a plan's scalars: floats at 12 significant digits, a blur kernel or matrix as its shape and its sum at 9."""
    parts = []
    for op in plan:
        for k in sorted(op):
            v = op[k]
            if isinstance(v, np.ndarray) or isinstance(v, list):
                v = f"{np.asarray(v).shape}:{np.asarray(v).sum():.9g}"
            elif isinstance(v, float):
                v = f"{v:.12g}"
            parts.append(f"{k}={v}")
    return hashlib.sha256(";".join(parts).encode()).hexdigest()[:16]


# (seed, scale, crop): the hashes of the first three plans and the generator's next random(), taken from the commit before the
# camera stage existed
PARENT_PLANS = {
    (0, 4, 400): (["ecddbcfeef2e375e", "537a0d290f2f83f9", "e7313c66d9c70e4f"], "0.612773179869"),
    (1, 4, 400): (["46d26e5c671caa54", "2413f120ec51df7b", "bf1fe702e129fc12"], "0.578175905299"),
    (2, 2, 400): (["d9c81cdbfceb3a76", "699a5672ecaf1144", "df6ccbaf819ad9c2"], "0.42291764839"),
    (3, 4, 64): (["9e4c00b6feb70ed3", "0e7def7c3a98b3b0", "53f6b78ace57e09b"], "0.505420373648"),
    (4, 2, 32): (["5d7c5dbed06c814c", "ddcca3cc62b1c98f", "dfaa97370faa9896"], "0.322810264595"),
}


def test_without_a_bank_the_plans_are_the_parents():
    for (seed, scale, crop), (hashes, nxt) in PARENT_PLANS.items():
        rng = random.Random(seed)
        plans = [B.draw_plan(rng, scale, crop, camera=None) for _ in range(3)]
        assert [plan_hash(p) for p in plans] == hashes and f"{rng.random():.12g}" == nxt, (seed, scale, crop)
        assert all(op["op"] != "camera" and op["stage"] != 2 for p in plans for op in p)


def _plain(plan):
    return [{k: (v.rec.tolist(), v.curve) if isinstance(v, isp.CameraParams) else v.tolist() if isinstance(v, np.ndarray) else v
             for k, v in op.items()} for op in plan]


def test_draws_with_a_bank(bank):
    a, b = random.Random(7), random.Random(7)
    for _ in range(20):
        assert _plain(B.draw_plan(a, 4, 400, camera=bank)) == _plain(B.draw_plan(b, 4, 400, camera=bank))
    # ``stages`` leaves the stream alone, and keeps the ops of its stages only
    a, b = random.Random(8), random.Random(8)
    for _ in range(40):
        full, part = B.draw_plan(a, 4, 400, camera=bank), B.draw_plan(b, 4, 400, stages=(2,), camera=bank)
        assert a.getstate() == b.getstate()
        # the same draws; the side differs, since without stage 1 / 6 nothing shrinks
        strip = lambda plan: [{k: v for k, v in op.items() if k != "size"} for op in _plain(plan) if op["stage"] == 2]
        assert strip(full) == strip(part)
        assert all(op["stage"] in (-1, 2, 9) for op in part)
    rng, acting = random.Random(9), 0
    for _ in range(400):
        ops = [op for op in B.draw_plan(rng, 4, 400, camera=bank) if op["op"] == "camera"]
        assert len(ops) <= 1
        for op in ops:
            acting += 1
            assert op["stage"] == 2 and 1 <= op["pos"] <= 9 and op["size"] >= 3
            assert op["camera"] in range(11) and op["curve"] in range(11) and 0 <= op["fw"] < 1
            assert 1.2 <= op["d_r"] < 2.4 and 1.2 <= op["d_b"] < 2.4 and -0.1 <= op["e"] < 0.1
            assert 1e-4 <= op["shot"] <= 0.006
            line = 2.275 * np.log10(op["shot"]) + 1.47
            assert line - 1.5 - 1e-9 <= np.log10(op["read"]) <= line + 1.5 + 1e-9
            assert isinstance(op["params"], isp.CameraParams) and op["params"].curve == op["curve"]
    print(f"camera op in {acting} of 400 plans")
    assert 0.15 * 400 <= acting <= 0.35 * 400


def test_a_side_below_3_at_the_stage_raises(bank):
    """crop 16 at scale 4: after the first downsample (by up to 2 * scale) the side can be 2."""
    rng, raised = random.Random(0), 0
    for _ in range(300):
        try:
            B.draw_plan(rng, 4, 16, camera=bank)
        except ValueError as e:
            assert "needs at least 3" in str(e)
            raised += 1
    assert raised > 0


# ---- apply_plans ------------------------------------------------------------------------------------------------------------------
def _plans_with_camera(bank, n, scale, crop, stages, want, first_seed=0):
    """The first seed from ``first_seed`` whose ``n`` plans hold exactly ``want`` camera ops."""
    for seed in range(first_seed, first_seed + 500):
        rng = random.Random(seed)
        plans = [B.draw_plan(rng, scale, crop, stages=stages, camera=bank) for _ in range(n)]
        if sum(op["op"] == "camera" for p in plans for op in p) == want:
            return plans
    raise AssertionError("no such seed")


def test_apply_plans_with_and_without_the_op():
    bank = analytic_bank()
    x = torch.stack([image8(s, 64, 64) for s in range(4)])
    plans = _plans_with_camera(bank, 4, 4, 64, None, 2)
    acts = [any(op["op"] == "camera" for op in p) for p in plans]
    gen = lambda: torch.Generator().manual_seed(3)
    out, hr = B.apply_plans(x, plans, gen(), hr=x.clone())
    assert out.shape == (4, 3, 16, 16) and hr.shape == x.shape and 0 <= float(out.min()) and float(out.max()) <= 1
    assert torch.equal((out * 255).round().div(255), out), "the k / 255 grid"
    for b, act in enumerate(acts):
        assert torch.equal(hr[b], x[b]) != act, "the HR pass rewrites the acting samples and no other"
        if act:
            p = next(op["params"] for op in plans[b] if op["op"] == "camera")
            assert torch.equal(hr[b], isp.process(isp.unprocess(x[b], p), p))
    # without hr the HR pass is not run and the return value is the one of before
    again = B.apply_plans(x, plans, gen())
    assert torch.is_tensor(again) and torch.equal(again, out)
    o2, pre, q, hr2 = B.apply_plans(x, plans, gen(), parts=True, hr=x.clone())
    assert torch.equal(o2, out) and torch.equal(hr2, hr) and pre.shape == out.shape and q.shape == (4,)
    # no camera op in any plan: the plans of draw_plan without a bank give what they gave
    rng = random.Random(5)
    plain = [B.draw_plan(rng, 4, 64) for _ in range(4)]
    o3, hr3 = B.apply_plans(x, plain, gen(), hr=x.clone())
    assert torch.equal(o3, B.apply_plans(x, plain, gen())) and torch.equal(hr3, x)
    with pytest.raises(ValueError, match="clone of the batch"):
        B.apply_plans(x, plans, gen(), hr=x[:2].clone())


def test_the_stage_alone_through_apply_plans():
    """stages=(2,) at scale 2: no other op, so the batch before the final JPEG is the stage's output for the acting samples."""
    bank = analytic_bank()
    x = torch.stack([image8(10 + s, 32, 32) for s in range(3)])
    plans = _plans_with_camera(bank, 3, 2, 32, (2,), 2)
    gen = torch.Generator().manual_seed(1)
    _, pre, _ = B.apply_plans(x, plans, gen, parts=True)
    gen = torch.Generator().manual_seed(1)
    ops = {b: op for b, plan in enumerate(plans) for op in plan if op["op"] == "camera"}
    for b in sorted(ops, key=lambda b: (ops[b]["pos"], b)):        # the normals: by position of the shuffle, then in batch order
        z = torch.randn(32, 32, generator=gen)
        (want,), _ = isp.camera_noise([x[b]], None, [ops[b]["params"]], [z])
        assert torch.equal(pre[b], want) and not torch.equal(pre[b], x[b])
    for b in set(range(3)) - set(ops):
        assert torch.equal(pre[b], x[b])


# ---- targets and options ----------------------------------------------------------------------------------------------------------
def test_sampler_targets_follow_the_reference():
    bank = analytic_bank()
    g = np.random.RandomState(1)
    store = PatchStore([g.randint(0, 256, (70, 80, 3)).astype(np.uint8), g.randint(0, 256, (64, 96, 3)).astype(np.uint8)])
    make = lambda **kw: PatchSampler("sr", store, degrade=True, degrade_crop=64, patch=8, scale=4, batch=6, camera=bank, **kw)
    for seed in range(40):                     # a seed whose batch has acting and non-acting samples
        s = make(seed=seed, usm=True, plain_gt=True)
        work, extras = s.draw()
        acts = [any(op["op"] == "camera" for op in e[0]) for e in extras]
        if 0 < sum(acts) < len(acts):
            break
    lq, gt, plain = s.next(work, extras)
    assert lq.shape == (6, 3, 8, 8) and gt.shape == plain.shape == (6, 3, 32, 32)
    from grl_image_restoration_amd import tasks as T

    wt = torch.tensor(work, dtype=torch.int32)
    crops = store.sample(wt, 64, 1)
    sharp = T.usm_sharp(crops)
    cut = lambda im, b: im[:, 4 * extras[b][1] : 4 * extras[b][1] + 32, 4 * extras[b][2] : 4 * extras[b][2] + 32]
    for b, act in enumerate(acts):
        assert torch.equal(plain[b], cut(crops[b], b)), "plain_gt is untouched"
        if act:
            p = next(op["params"] for op in extras[b][0] if op["op"] == "camera")
            assert torch.equal(gt[b], cut(isp.process(isp.unprocess(sharp[b], p), p), b)), "the sharpened crop after the HR pass"
        else:
            assert torch.equal(gt[b], cut(sharp[b], b))
    # without usm the engines train on the untouched crop: the HR pass's result is not the target
    s2 = make(seed=seed)
    w2, e2 = s2.draw()
    assert any(op["op"] == "camera" for e in e2 for op in e[0])
    _, gt2 = s2.next(w2, e2)
    c2 = store.sample(torch.tensor(w2, dtype=torch.int32), 64, 1)
    for b in range(6):
        assert torch.equal(gt2[b], c2[b, :, 4 * e2[b][1] : 4 * e2[b][1] + 32, 4 * e2[b][2] : 4 * e2[b][2] + 32])


def test_option_errors():
    ok = dict(scale=4, patch=8, degrade=True, degrade_crop=64, camera=True)
    assert R.resolve("sr", "train", **ok).degrade_crop == 64
    with pytest.raises(ValueError, match="belongs to training with degrade"):
        R.resolve("sr", "train", scale=4, lq=True, camera=True)
    with pytest.raises(ValueError, match="belongs to training with degrade"):
        R.resolve("sr", "evaluate", scale=4, lq=True, camera=True)
    with pytest.raises(ValueError, match="at least 32.*reflects by 2"):
        R.resolve("sr", "train", **dict(ok, degrade_crop=16, patch=4))
    g = np.random.RandomState(0)
    store = PatchStore([g.randint(0, 256, (40, 40, 3)).astype(np.uint8)])
    with pytest.raises(ValueError, match="at least 32"):
        PatchSampler("sr", store, degrade=True, degrade_crop=16, patch=4, scale=4, camera=analytic_bank())
    with pytest.raises(ValueError, match="belongs to training with degrade"):
        PatchSampler("sr", store, PatchStore([g.randint(0, 256, (10, 10, 3)).astype(np.uint8)]), patch=4, scale=4, camera=analytic_bank())


def test_loader_names_what_it_misses(tmp_path, golden):
    from scipy.io import savemat

    with pytest.raises(FileNotFoundError, match="tonecurves.mat"):
        isp.CameraBank.load(str(tmp_path))
    curves = np.zeros((134, 2 * golden["curve_x"].shape[1]))
    for c, row in enumerate(isp.CURVES):
        curves[row] = np.stack([golden["curve_x"][c], golden["curve_y"][c]]).reshape(-1, order="F")
    savemat(str(tmp_path / "tonecurves.mat"), {"ToneCurves": curves})
    for n, name in enumerate(isp.CAMERAS):
        m = {"ForwardMatrix1": golden["forward1"][n], "ForwardMatrix2": golden["forward2"][n]}
        if name == "nikon_d810":
            del m["ForwardMatrix2"]
        if name != "olympus_em1":
            savemat(str(tmp_path / (name + ".mat")), m)
    with pytest.raises(KeyError, match="nikon_d810.mat has no key 'ForwardMatrix2'"):
        isp.CameraBank.load(str(tmp_path))
    savemat(str(tmp_path / "nikon_d810.mat"), {"ForwardMatrix1": golden["forward1"][8], "ForwardMatrix2": golden["forward2"][8]})
    with pytest.raises(FileNotFoundError, match="olympus_em1.mat"):
        isp.CameraBank.load(str(tmp_path))
    savemat(str(tmp_path / "olympus_em1.mat"), {"ForwardMatrix1": golden["forward1"][10], "ForwardMatrix2": golden["forward2"][10]})
    loaded = isp.CameraBank.load(str(tmp_path))
    assert torch.equal(loaded.forward1, torch.from_numpy(golden["forward1"]).float())
    assert np.array_equal(loaded.curve_x, golden["curve_x"]) and np.array_equal(loaded.curve_y, golden["curve_y"])
