"""CPU tests of progressive training and MixUp (remix.py; the transform is stated in include/grl_hip.h): the draws against the
reference's MixUp_AUG (tests/golden/tasks/remix.npz, tools/make_golden_remix.py) and against Python's own ``random.Random``, the
stage rule against ``bisect``, the torch restatement of ``batch_remix``, and ``train``'s new options on CPU tensors."""
import bisect
import itertools
import os
import random

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import remix as R
from grl_image_restoration_amd import train

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tasks", "remix.npz")


def test_mixup_draws_and_outputs_equal_the_reference_bit_for_bit():
    z = np.load(GOLDEN)
    seeds = z["seed"]
    assert len(seeds) >= 3
    for k, seed in enumerate(seeds):
        lq, gt = torch.from_numpy(z[f"lq{k}"]), torch.from_numpy(z[f"gt{k}"])
        b, scale = lq.shape[0], gt.shape[2] // lq.shape[2]
        gen = torch.Generator().manual_seed(int(seed))
        plan = R.draw_remix(random.Random(0), gen, b, 8, b, 8, True)          # full batch, full patch: only the MixUp draws
        assert plan.idx is None and (plan.x0, plan.y0) == (0, 0)
        assert plan.perm.dtype == torch.int64 and np.array_equal(plan.perm.numpy(), z[f"perm{k}"])
        assert plan.lam.dtype == torch.float32 and plan.lam.numpy().tobytes() == z[f"lam{k}"].tobytes()
        # the reference mixes non-square images too; the restatement's blend is the same expression, applied directly ...
        lam = plan.lam.view(-1, 1, 1, 1)
        for x, want in ((lq, z[f"lq_out{k}"]), (gt, z[f"gt_out{k}"])):
            assert (lam * x + (1 - lam) * x[plan.perm]).numpy().tobytes() == want.tobytes()
        # ... and through batch_remix where the case is a square pair
        if lq.shape[2] == lq.shape[3]:
            a, b_ = R.batch_remix(lq, gt, plan, scale)
            assert a.numpy().tobytes() == z[f"lq_out{k}"].tobytes() and b_.numpy().tobytes() == z[f"gt_out{k}"].tobytes()


def test_progressive_draws_are_pythons_own():
    for seed, (B, P, b, p) in enumerate([(8, 64, 4, 32), (8, 64, 8, 32), (8, 64, 3, 64), (5, 9, 1, 1)]):
        own, ref = random.Random(seed), random.Random(seed)
        for _ in range(3):
            plan = R.draw_remix(own, None, B, P, b, p, False)
            idx = tuple(ref.sample(range(B), k=b)) if b < B else None
            x0 = ref.randrange(P - p + 1) if p < P else 0
            y0 = ref.randrange(P - p + 1) if p < P else 0
            assert (plan.idx, plan.x0, plan.y0, plan.perm, plan.lam) == (idx, x0, y0, None, None)
        assert own.getstate() == ref.getstate()


def test_no_draw_is_consumed_by_a_part_that_is_off():
    rng, gen = random.Random(5), torch.Generator().manual_seed(5)
    s_rng, s_gen = rng.getstate(), gen.get_state().clone()
    plan = R.draw_remix(rng, gen, 4, 16, 4, 16, False)                        # b == B, p == P, MixUp off
    assert plan == (None, 0, 0, None, None)
    assert rng.getstate() == s_rng and torch.equal(gen.get_state(), s_gen)
    R.draw_remix(rng, gen, 4, 16, 2, 8, False)                                # progressive only: the torch stream stays
    assert rng.getstate() != s_rng and torch.equal(gen.get_state(), s_gen)
    rng.setstate(s_rng)
    R.draw_remix(rng, gen, 4, 16, 4, 16, True)                                # MixUp only: the Python stream stays
    assert rng.getstate() == s_rng and not torch.equal(gen.get_state(), s_gen)
    # b == B with a crop consumes exactly the two randrange draws
    ref = random.Random(5)
    want = (ref.randrange(9), ref.randrange(9))
    plan = R.draw_remix(rng, gen, 4, 16, 4, 8, False)
    assert (plan.x0, plan.y0) == want and rng.getstate() == ref.getstate()
    # the class: a step of a full-size stage before --mixup-after draws nothing and hands the batch back
    m = R.BatchRemix(2, 4, 1, [2, 2], [2, 1], [4, 2], mixup=True, mixup_after=1, seed=9)
    before = m.rng_state()
    lq, gt = torch.rand(2, 3, 4, 4), torch.rand(2, 3, 4, 4)
    a, b = m(0, lq, gt)
    assert a is lq and b is gt and m.rng_state()["draws"] == before["draws"] and torch.equal(m.rng_state()["mixup"], before["mixup"])


def test_stage_of_is_bisect_left():
    for steps in ([3], [2, 2], [1000, 2000], [1, 1, 5]):
        S = list(itertools.accumulate(steps))
        for n in range(S[-1] + 3):
            assert R.stage_of(n, steps) == bisect.bisect_left(S, n)
    assert R.stage_of(2, [2, 2]) == 0 and R.stage_of(3, [2, 2]) == 1 and R.stage_of(4, [2, 2]) == 1      # n == S_g stays in stage g
    m = R.BatchRemix(8, 64, 4, [2, 2], [8, 4], [32, 64])
    assert [m.sizes(n) for n in range(5)] == [(8, 32)] * 3 + [(4, 64)] * 2
    with pytest.raises(ValueError):
        m.sizes(5)


def test_cpu_batch_remix_identity_crop_and_channel_counts():
    g = torch.Generator().manual_seed(0)
    for scale in (1, 2, 3, 4):
        lq, gt = torch.randn(3, 6, 7, 7, generator=g), torch.randn(3, 3, 7 * scale, 7 * scale, generator=g)      # Cl = 6 / Cg = 3
        a, b = R.batch_remix(lq, gt, R.RemixPlan(None, 0, 0, None, None), scale)
        assert a.numpy().tobytes() == lq.numpy().tobytes() and b.numpy().tobytes() == gt.numpy().tobytes()
        a, b = R.batch_remix(lq, gt, R.RemixPlan((2, 0), 1, 3, None, None), scale, patch=4)
        assert torch.equal(a, lq[[2, 0]][:, :, 1:5, 3:7]) and a.is_contiguous()
        assert torch.equal(b, gt[[2, 0]][:, :, scale : 5 * scale, 3 * scale : 7 * scale]) and b.is_contiguous()
        # selection, crop and blend together, into given buffers
        perm, lam = torch.tensor([1, 0]), torch.tensor([0.25, 0.7])
        out = (torch.full((2, 6, 4, 4), 9.0), torch.full((2, 3, 4 * scale, 4 * scale), 9.0))
        a, b = R.batch_remix(lq, gt, R.RemixPlan((2, 0), 1, 3, perm, lam), scale, out=out)
        assert a is out[0] and b is out[1]
        x = lq[[2, 0]][:, :, 1:5, 3:7]
        assert torch.equal(a, lam.view(2, 1, 1, 1) * x + (1 - lam.view(2, 1, 1, 1)) * x[perm])
    # a fixed point of the permutation is still computed: lam * x + (1 - lam) * x, which is not always x
    x = torch.rand(1, 1, 64, 64, generator=g)
    lam = torch.tensor([0.3])
    a, _ = R.batch_remix(x, x.clone(), R.RemixPlan(None, 0, 0, torch.tensor([0]), lam), 1)
    assert torch.equal(a, lam * x + (1 - lam) * x) and not torch.equal(a, x)


def test_an_invalid_plan_raises():
    lq, gt = torch.zeros(3, 3, 8, 8), torch.zeros(3, 3, 16, 16)
    ok = R.RemixPlan((0, 2), 1, 2, torch.tensor([1, 0]), torch.tensor([0.5, 0.5]))
    R.batch_remix(lq, gt, ok, 2, patch=5)
    bad = [
        (ok._replace(idx=(0, 3)), 5),                    # a sample outside the batch
        (ok._replace(idx=(0, -1)), 5),
        (ok._replace(idx=()), 5),
        (ok._replace(x0=4), 5),                          # 4 + 5 > 8
        (ok._replace(y0=-1), 5),
        (ok, 9),                                         # p > P
        (ok, 0),
        (ok._replace(perm=torch.tensor([0, 0])), 5),     # no permutation
        (ok._replace(perm=torch.tensor([0, 2])), 5),
        (ok._replace(lam=torch.tensor([0.5])), 5),
        (ok._replace(lam=None), 5),
    ]
    for plan, p in bad:
        with pytest.raises(ValueError):
            R.batch_remix(lq, gt, plan, 2, patch=p)
    with pytest.raises(ValueError):
        R.batch_remix(lq, gt[:, :, :8, :8], ok, 2, patch=5)                   # not a pair of that scale
    with pytest.raises(ValueError):
        R.batch_remix(lq, gt, ok, 2, out=(torch.zeros(2, 3, 5, 5), torch.zeros(2, 3, 10, 11)))
    for kw in (dict(stage_steps=[1], batch_sizes=[1, 1], patch_sizes=[4]), dict(stage_steps=[1], batch_sizes=[3], patch_sizes=[4]),
               dict(stage_steps=[1], batch_sizes=[1], patch_sizes=[9]), dict(mixup_after=2)):
        with pytest.raises(ValueError):
            R.BatchRemix(2, 8, 1, **kw)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image

    d = tmp_path_factory.mktemp("remix_gt")
    g = np.random.RandomState(0)
    for i in range(3):
        Image.fromarray(g.randint(0, 256, (40, 48, 3)).astype(np.uint8)).save(d / f"im{i}.png")
    return str(d)


ARGS = ["--task", "sr_bicubic", "--scale", "2", "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--patch", "16", "--batch", "2",
        "--eager", "--device", "cpu", "--lr", "1e-3", "--seed", "3"]
STAGES = ["--stage-steps", "2+2", "--batch-sizes", "1+2", "--patch-sizes", "8+16"]


def test_every_refusal_exits_with_status_2(folder, capsys):
    base = ARGS + ["--gt", folder, "--steps", "4"]
    bad = [
        ["--stage-steps", "2+2", "--batch-sizes", "1", "--patch-sizes", "8+16"],          # lists of different lengths
        ["--stage-steps", "4", "--batch-sizes", "1+2", "--patch-sizes", "8"],
        ["--batch-sizes", "1+2"],
        ["--stage-steps", "2+2", "--batch-sizes", "1+3", "--patch-sizes", "8+16"],        # above --batch
        ["--stage-steps", "2+2", "--batch-sizes", "1+2", "--patch-sizes", "8+32"],        # above --patch
        ["--stage-steps", "2+1", "--batch-sizes", "1+2", "--patch-sizes", "8+16"],        # 3 stage steps for 4 steps
        ["--stage-steps", "2+x", "--batch-sizes", "1+2", "--patch-sizes", "8+16"],
        ["--stage-steps", "2+0+2", "--batch-sizes", "1+1+2", "--patch-sizes", "8+8+16"],
        ["--mixup-after", "1"],                                                           # without --mixup
        STAGES + ["--mixup-after", "1"],
        ["--mixup", "--mixup-after", "-1"],
    ]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            train.main(base + extra)
        assert e.value.code == 2, extra
    gan = ["--task", "sr", "--scale", "2", "--lq", folder, "--gt", folder, "--steps", "4", "--device", "cpu", "--patch", "16", "--batch", "2",
           "--gan"]
    for extra in (STAGES, ["--mixup"], STAGES + ["--mixup", "--mixup-after", "1"]):
        with pytest.raises(SystemExit) as e:
            train.main(gan + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()


def test_two_stage_run_with_mixup_and_its_resume(folder, tmp_path, capsys):
    opts = ARGS + STAGES + ["--mixup", "--mixup-after", "1", "--gt", folder]
    torch.manual_seed(0)
    whole = train.main(opts + ["--steps", "4", "--out", str(tmp_path / "whole")])
    assert whole["steps"] == [0, 1, 2, 3] and all(np.isfinite(whole["losses"]))
    assert whole["stages"] == [(0, 1, 8), (3, 2, 16)]                         # step 2 == S_0 still belongs to stage 0
    plain = train.main(ARGS + ["--gt", folder, "--steps", "1"])
    assert "stages" not in plain and plain["work"] == whole["work"][:1]       # the sampler's stream is what it was

    torch.manual_seed(0)
    first = train.main(opts + ["--steps", "2", "--out", str(tmp_path / "split")])
    assert first["losses"] == whole["losses"][:2] and first["stages"] == [(0, 1, 8)]
    obj = torch.load(first["checkpoint"], map_location="cpu", weights_only=False)
    assert set(obj) == {"state_dict", "step", "optimizer", "sampler_rng", "args", "remix_rng"} and obj["step"] == 2
    assert set(obj["remix_rng"]) == {"draws", "mixup"}

    rest = train.main(opts + ["--steps", "4", "--resume", first["checkpoint"], "--out", str(tmp_path / "split")])
    assert rest["steps"] == [2, 3] and rest["work"] == whole["work"][2:]
    assert rest["stages"] == [(2, 1, 8), (3, 2, 16)]                          # the stage follows from the step
    assert rest["losses"] == pytest.approx(whole["losses"][2:], rel=1e-5)
    a = torch.load(whole["checkpoint"], map_location="cpu", weights_only=False)["state_dict"]
    b = torch.load(rest["checkpoint"], map_location="cpu", weights_only=False)["state_dict"]
    assert a.keys() == b.keys() and all(torch.allclose(a[k], b[k], rtol=1e-5, atol=1e-7) for k in a)
    capsys.readouterr()
