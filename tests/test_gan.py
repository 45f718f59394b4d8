"""The GAN stage on the CPU: the composite discriminator and ``GanStep`` in float64 against the reference's own float64 runs
(tests/golden/gan/disc.npz, disc_grads.npz and disc_grads_B.npz, written by tools/make_golden_gan.py from models/aux_archs/discriminator.py and
engines/base_gan.py:86-147).

Bounds.  Discriminator: 1e-10 * max(1, max|fixture array|) -- both sides are float64 runs of the same arithmetic, possibly summed
in another order (the large gradient tensors are int32 fixed point over their own max-abs <= 0.2: off by at most 4.7e-11).
``GanStep``: the six logged scalars of two iterations to 1e-8 relative."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from grl_image_restoration_amd.discriminator import UNetDiscriminatorSN
from grl_image_restoration_amd.gan import GanStep, gan_loss

HERE = os.path.dirname(os.path.abspath(__file__))
SN = [f"conv{i}" for i in range(1, 9)]
NAMES = ["loss_g_pix", "loss_g_gan", "loss_d_real", "loss_d_fake", "out_d_real", "out_d_fake"]


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(HERE, "golden", "gan", "disc.npz"), allow_pickle=False)
    arrays = {k: z[k] for k in z.files if k != "meta"}
    for name in ("disc_grads.npz", "disc_grads_B.npz"):           # the parameter gradients of case A / case B
        g = np.load(os.path.join(HERE, "golden", "gan", name), allow_pickle=False)
        arrays.update({k: g[k] for k in g.files})
    return json.loads(str(z["meta"])), arrays


def fixture_state(arrays) -> dict:
    """The reference's 28-key state dict (float64) from the fixture."""
    sd = {k[len("d__p__"):]: torch.from_numpy(v.astype(np.float64)) for k, v in arrays.items() if k.startswith("d__p__")}
    for c in SN:
        sd[f"{c}.weight_u"] = torch.from_numpy(arrays[f"d__u0__{c}"])
        sd[f"{c}.weight_v"] = torch.from_numpy(arrays[f"d__v0__{c}"])
    return sd


def fresh(arrays, num_feat=8):
    d = UNetDiscriminatorSN(3, num_feat, True).double()
    sd = fixture_state(arrays)
    assert len(sd) == 28
    d.load_state_dict(sd, strict=True)
    return d


def close(got, want, what):
    want = torch.as_tensor(want)
    bound = 1e-10 * max(1.0, float(want.abs().max()))
    err = float((torch.as_tensor(got).double() - want).abs().max())
    print(f"{what}: max|d| {err:.3e} (bound {bound:.1e})")
    assert err <= bound, (what, err, bound)


def fixture_grad(arrays, case, key):
    name = f"d__{case}__g__{key}"
    if name + "__q" in arrays:
        return torch.from_numpy(arrays[name + "__q"].astype(np.float64)) * (float(arrays[name + "__qmax"]) / 2.0 ** 31)
    return torch.from_numpy(arrays[name])


def test_state_dict_carries_the_reference_names(fx):
    _, arrays = fx
    d = UNetDiscriminatorSN(3, 8, True)
    keys = set(d.state_dict())
    assert keys == set(fixture_state(arrays)) and len(keys) == 28
    assert sum(p.numel() for p in d.parameters()) == 68649
    with pytest.raises(ValueError):
        d(torch.zeros(1, 3, 12, 16))


@pytest.mark.parametrize("case", ["A", "B"])
def test_composite_discriminator_matches_the_reference_in_float64(fx, case):
    _, arrays = fx
    x, xf = torch.from_numpy(arrays[f"d__{case}__x"]).double(), torch.from_numpy(arrays[f"d__{case}__xf"]).double()
    d = fresh(arrays).eval()
    with torch.no_grad():
        close(d(x), arrays[f"d__{case}__eval"], "eval logits")
    for c in SN:                                      # eval mode: no power iteration
        assert torch.equal(getattr(d, c).weight_u, torch.from_numpy(arrays[f"d__u0__{c}"]))
    d = fresh(arrays).train()
    for k in (1, 2, 3):
        with torch.no_grad():
            close(d(x), arrays[f"d__{case}__train{k}"], f"train logits {k}")
        for c in SN:
            close(getattr(d, c).weight_u, arrays[f"d__{case}__u{k}__{c}"], f"u{k} {c}")
            close(getattr(d, c).weight_v, arrays[f"d__{case}__v{k}__{c}"], f"v{k} {c}")
    d = fresh(arrays).train()
    xg = x.clone().requires_grad_(True)
    gan_loss(d(xg), True, is_disc=True).backward()
    close(xg.grad, arrays[f"d__{case}__gx"], "input gradient")
    d = fresh(arrays).train()
    loss = gan_loss(d(x), True, True) + gan_loss(d(xf), False, True)
    close(loss.detach(), arrays[f"d__{case}__dloss"], "D loss")
    loss.backward()
    for k, p in d.named_parameters():
        close(p.grad, fixture_grad(arrays, case, k), f"grad {k}")


def test_gan_loss_weight_applies_to_the_generator_only():
    z = torch.tensor([[0.3, -1.2], [2.0, 0.0]], dtype=torch.float64)
    ref1 = torch.nn.BCEWithLogitsLoss()(z, torch.ones_like(z))
    ref0 = torch.nn.BCEWithLogitsLoss()(z, torch.zeros_like(z))
    assert gan_loss(z, True, is_disc=True, weight=0.1) == ref1 and gan_loss(z, False, is_disc=True) == ref0
    assert gan_loss(z, True, is_disc=False, weight=0.1) == ref1 * 0.1


def test_gan_step_matches_the_reference_alternation(fx):
    from grl_image_restoration_amd import GRL
    from oracle import grl_oracle as O

    meta, arrays = fx
    g = GRL(**meta["g_cfg"])
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in g.state_dict().items()}, meta["g_weight_seed"])
    g.load_state_dict(sd, strict=True)
    g = g.double().train()
    d = fresh(arrays).train()
    opt_g, opt_d = torch.optim.Adam(g.parameters(), lr=meta["lr"]), torch.optim.Adam(d.parameters(), lr=meta["lr"])
    seen = []
    step_g = opt_g.step

    def checked_step(*a, **kw):          # at the generator's step no discriminator parameter has a gradient
        seen.append(all(p.grad is None for p in d.parameters()))
        return step_g(*a, **kw)

    opt_g.step = checked_step
    step = GanStep(g, d, opt_g, opt_d, lambda y, t: (y - t).abs().mean(), pixel_weight=meta["pixel_weight"], gan_weight=meta["gan_weight"],
                   gan_loss_weight=meta["gan_loss_weight"], usm_pixel=True, usm_gan=False)
    lq, gt, gt_usm = (torch.from_numpy(arrays[k]).double() for k in ("s__lq", "s__gt", "s__gt_usm"))
    want = arrays["s__scalars"]
    for it in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = step(lq, gt, gt_usm)
        assert list(out) == NAMES
        for j, n in enumerate(NAMES):
            rel = abs(float(out[n]) - want[it, j]) / abs(want[it, j])
            print(f"iteration {it} {n}: {float(out[n]):.12f} against {want[it, j]:.12f} (relative {rel:.2e})")
            assert rel <= 1e-8, (it, n, rel)
        assert all(p.requires_grad for p in d.parameters())
        for c in SN:                     # u advanced three times per iteration
            close(getattr(d, c).weight_u, arrays[f"s__u{3 * (it + 1)}__{c}"], f"u after iteration {it} {c}")
    assert seen == [True, True]


# ---- rule table and command line ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    from PIL import Image

    gt, lq = tmp_path_factory.mktemp("gan_gt"), tmp_path_factory.mktemp("gan_lq")
    g = np.random.RandomState(0)
    for i in range(3):
        Image.fromarray(g.randint(0, 256, (40, 48, 3)).astype(np.uint8)).save(gt / f"im{i}.png")
        Image.fromarray(g.randint(0, 256, (20, 24, 3)).astype(np.uint8)).save(lq / f"im{i}.png")
    return str(gt), str(lq)


GAN_ARGS = ["--task", "sr", "--scale", "2", "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--patch", "8", "--batch", "2",
            "--gan", "--disc-feat", "8", "--usm", "--device", "cpu", "--lr", "1e-3", "--seed", "3"]


def test_gan_rule_and_argument_errors(folders, capsys, monkeypatch):
    from grl_image_restoration_amd import task_rules, train

    assert [t for t in task_rules.RULES if task_rules.RULES[t].gan] == ["sr"]
    with pytest.raises(ValueError, match="no GAN stage"):
        task_rules.resolve("dn", "train", sigma=25, gan=True)
    with pytest.raises(ValueError, match="no GAN stage"):
        task_rules.resolve("sr", "evaluate", lq=True, gan=True)
    gt, lq = folders
    with pytest.raises(SystemExit) as e:                                # a task other than sr
        train.main(["--task", "sr_bicubic", "--scale", "2", "--gt", gt, "--steps", "1", "--device", "cpu", "--gan"])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:                                # --disc-ckpt without --gan
        train.main(["--task", "sr", "--scale", "2", "--gt", gt, "--lq", lq, "--steps", "1", "--device", "cpu", "--disc-ckpt", "x"])
    assert e.value.code == 2
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "1"])
    assert e.value.code == 2
    assert "--eager is single-process; the captured step owns the gradient all-reduce" in capsys.readouterr().err


def test_gan_command_line_checkpoint_and_resume(folders, tmp_path, capsys):
    from grl_image_restoration_amd import GRL, make_config, train
    from grl_image_restoration_amd.evaluate import load_checkpoint, load_discriminator_checkpoint

    gt, lq = folders
    torch.manual_seed(0)
    whole = train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "3", "--out", str(tmp_path / "whole")])
    assert whole["steps"] == [0, 1, 2] and [list(r) for r in whole["gan"]] == [NAMES] * 3
    assert all(np.isfinite(list(r.values())).all() for r in whole["gan"])
    torch.manual_seed(0)
    first = train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "2", "--out", str(tmp_path / "split")])
    assert first["gan"] == whole["gan"][:2]
    ckpt = first["checkpoint"]
    obj = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert set(obj) == {"state_dict", "step", "optimizer", "optimizer_d", "sampler_rng", "args"} and obj["step"] == 2
    keys = set(obj["state_dict"])
    assert all(k.startswith(("model.model_g.", "model.model_d.")) for k in keys)
    assert sum(k.startswith("model.model_d.") for k in keys) == 28 and "model.model_d.conv3.weight_u" in keys
    # evaluate.load_checkpoint reads the generator out of it; the discriminator's keys are ignored
    fresh = GRL(**make_config("tiny", "yaml", upscale=2, img_size=8, depths=[1], num_heads_window=[2], num_heads_stripe=[2]))
    res = load_checkpoint(fresh, ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    want = obj["state_dict"]["model.model_g.conv_first.weight"]
    assert torch.equal(fresh.state_dict()["conv_first.weight"], want)
    d = UNetDiscriminatorSN(3, 8, True)
    load_discriminator_checkpoint(d, ckpt)
    assert torch.equal(d.conv3.weight_u, obj["state_dict"]["model.model_d.conv3.weight_u"])
    assert {int(s["step"]) for s in obj["optimizer_d"]["state"].values()} == {2}
    # --resume: the third step is that of the uninterrupted run -- same batch, same u / v, same optimizer state
    rest = train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "3", "--resume", ckpt, "--out", str(tmp_path / "split")])
    assert rest["steps"] == [2] and rest["work"] == [whole["work"][2]]
    for n in NAMES:
        assert rest["gan"][0][n] == pytest.approx(whole["gan"][2][n], rel=1e-5), n
    a = torch.load(whole["checkpoint"], map_location="cpu", weights_only=False)
    b = torch.load(rest["checkpoint"], map_location="cpu", weights_only=False)
    assert a["state_dict"].keys() == b["state_dict"].keys()
    assert all(torch.allclose(a["state_dict"][k], b["state_dict"][k], rtol=1e-5, atol=1e-7) for k in a["state_dict"])
    for k in ("model.model_d.conv1.weight_u", "model.model_d.conv8.weight_v"):
        assert torch.allclose(a["state_dict"][k], b["state_dict"][k], rtol=1e-5, atol=1e-7)
    # --ckpt / --disc-ckpt: both networks start from the GAN checkpoint's weights (learning rate 0: one step leaves them as loaded)
    again = train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "1", "--lr", "0", "--ckpt", ckpt, "--disc-ckpt", ckpt,
                                   "--out", str(tmp_path / "again")])
    c = torch.load(again["checkpoint"], map_location="cpu", weights_only=False)["state_dict"]
    for k in ("model.model_g.conv_first.weight", "model.model_d.conv0.weight", "model.model_d.conv3.weight_orig", "model.model_d.conv9.bias"):
        assert torch.equal(c[k], obj["state_dict"][k]), k
    assert not torch.equal(c["model.model_d.conv0.weight"], a["state_dict"]["model.model_d.conv0.weight"])
    capsys.readouterr()


def test_float64_image_through_a_float32_generator_on_the_cpu():
    """The composite path casts the image to the parameters' type: float32 parameters take a float64 image (a numpy default array)
    as before, float64 parameters compute in float64."""
    from grl_image_restoration_amd import GRL, make_config

    m = GRL(**make_config("tiny", "yaml", upscale=2, img_size=8, depths=[1], num_heads_window=[2], num_heads_stripe=[2])).eval()
    x = torch.from_numpy(np.random.RandomState(0).rand(1, 3, 8, 8))
    assert x.dtype == torch.float64
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            y64in, y32in = m(x), m(x.float())
            assert y64in.dtype == torch.float32 and torch.equal(y64in, y32in)
            assert m.double()(x.float()).dtype == torch.float64


def test_sampler_hands_out_both_targets(folders):
    from grl_image_restoration_amd import data as D

    gt, lq = folders
    stores = lambda: (D.PatchStore.from_folder(gt, 3, "cpu"), D.PatchStore.from_folder(lq, 3, "cpu"))
    one = D.PatchSampler("sr", *stores(), patch=8, batch=2, scale=2, seed=1, usm=True)
    two = D.PatchSampler("sr", *stores(), patch=8, batch=2, scale=2, seed=1, usm=True, plain_gt=True)
    plain = D.PatchSampler("sr", *stores(), patch=8, batch=2, scale=2, seed=1)
    a, b, c = one.next(), two.next(), plain.next()
    assert len(a) == 2 and len(b) == 3 and len(c) == 2
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(b[2], c[1]) and not torch.equal(b[1], b[2])
    with pytest.raises(ValueError):
        D.PatchSampler("sr", *stores(), patch=8, batch=2, scale=2, seed=1, plain_gt=True)
