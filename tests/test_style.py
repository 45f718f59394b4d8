"""The style loss on the CPU: the float64 composite of ``perceptual.PerceptualStyleLoss`` against the reference's own float64 runs
(tests/golden/gan/style.npz, written by tools/make_golden_style.py from losses/losses.py:59-187 and engines/base_gan.py:86-147),
``GanStep`` with both terms on, and the command line.

Bounds, as tests/test_perceptual.py holds its ``c__`` group.  Composite: 1e-10 * max(1, max|fixture array|) -- both sides are
float64 runs of the same arithmetic, possibly summed in another order.  ``GanStep``: the eight logged scalars of two iterations to
1e-8 relative."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import perceptual as P
from grl_image_restoration_amd.discriminator import UNetDiscriminatorSN
from grl_image_restoration_amd.gan import GanStep

HERE = os.path.dirname(os.path.abspath(__file__))
SN = [f"conv{i}" for i in range(1, 9)]
NAMES_S = ["loss_g_pix", "loss_g_percep", "loss_g_style", "loss_g_gan", "loss_d_real", "loss_d_fake", "out_d_real", "out_d_fake"]


def _npz(name):
    z = np.load(os.path.join(HERE, "golden", "gan", name), allow_pickle=False)
    return json.loads(str(z["meta"])), {k: z[k] for k in z.files if k != "meta"}


@pytest.fixture(scope="module")
def fx():
    return _npz("style.npz")


@pytest.fixture(scope="module")
def disc():
    return _npz("disc.npz")


@pytest.fixture(scope="module")
def weights(fx):
    return P.seeded_state_dict(fx[0]["vgg_seed"])


def close(got, want, what):
    want = torch.as_tensor(want)
    bound = 1e-10 * max(1.0, float(want.abs().max()))
    err = float((torch.as_tensor(got).double() - want).abs().max())
    print(f"{what}: max|d| {err:.3e} (bound {bound:.1e})")
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("case,W", [("A", 400), ("A", 40000), ("B", 400), ("B", 40000)])
def test_composite_matches_the_reference(fx, weights, case, W):
    meta, arrays = fx
    assert float(W) in meta["style_weights"]
    pl = P.PerceptualStyleLoss(meta["layer_weights"], weights, perceptual_weight=1.0, style_weight=float(W))
    x = torch.from_numpy(arrays[f"c__{case}__x"]).double().requires_grad_(True)
    gt = torch.from_numpy(arrays[f"c__{case}__gt"]).double().requires_grad_(True)
    percep, style = pl(x, gt)
    assert percep.dtype == style.dtype == torch.float64
    (percep + style).backward()
    tag = f"c__{case}__w{W}"
    close(percep.detach(), arrays[f"{tag}__percep"], f"{case} {W} percep")
    close(style.detach(), arrays[f"{tag}__style"], f"{case} {W} style")
    close(torch.stack(pl.last_style_means), arrays[f"c__{case}__gram_means"], f"{case} per-layer Gram L1 means")
    close(x.grad, arrays[f"{tag}__dx"], f"{case} {W} d(percep + style)/dx")
    assert gt.grad is None and all(p.grad is None and not p.requires_grad for p in pl.parameters())
    assert list(pl.last_diffs) == list(meta["layer_weights"]) and tuple(pl.last_diffs["conv1_2"].shape) == (x.shape[0], 64, 64)


def test_style_only_case(fx, weights):
    meta, arrays = fx
    so = meta["style_only"]
    pl = P.PerceptualStyleLoss(meta["layer_weights"], weights, perceptual_weight=so["perceptual_weight"], style_weight=so["style_weight"])
    x = torch.from_numpy(arrays[f"c__{so['case']}__x"]).double().requires_grad_(True)
    percep, style = pl(x, torch.from_numpy(arrays[f"c__{so['case']}__gt"]).double())
    assert percep is None
    style.backward()
    close(style.detach(), arrays["o__A__style"], "style-only loss")
    close(x.grad, arrays["o__A__dx"], "style-only dL/dx")


def test_a_term_is_none_exactly_when_its_weight_is_not_positive(weights):
    x, gt = torch.rand(1, 3, 16, 16, generator=torch.Generator().manual_seed(1)), torch.zeros(1, 3, 16, 16)
    for pw, sw in ((1.0, 2.0), (0.0, 2.0), (-1.0, 2.0), (1.0, 0.0), (1.0, -3.0), (0.0, 0.0)):
        percep, style = P.PerceptualStyleLoss(P.GAN_LAYER_WEIGHTS, weights, perceptual_weight=pw, style_weight=sw)(x, gt)
        assert (percep is None) == (pw <= 0) and (style is None) == (sw <= 0), (pw, sw)
        assert percep is None or float(percep) > 0
        assert style is None or float(style) > 0


def test_criteria_and_the_parent_class_keep_their_refusals(weights):
    for crit in ("l2", "fro"):
        with pytest.raises(NotImplementedError):
            P.PerceptualStyleLoss(P.GAN_LAYER_WEIGHTS, weights, style_weight=1.0, criterion=crit)
    with pytest.raises(NotImplementedError, match="PerceptualStyleLoss"):          # the refusal now says where the style loss lives
        P.PerceptualLoss(P.GAN_LAYER_WEIGHTS, weights, style_weight=1.0)
    assert "PerceptualStyleLoss" in P.PerceptualLoss.__doc__
    with pytest.raises(ValueError, match="differ"):
        P.PerceptualStyleLoss(P.GAN_LAYER_WEIGHTS, weights, style_weight=1.0)(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 32))


def test_gram_signs_reproduce_the_composite(fx, weights):
    """The decision-taking forward, fed the decisions of the very run it is compared with (``gram_signs`` from that run's D matrices
    among them), is that run: both losses and the gradient."""
    meta, arrays = fx
    pl = P.PerceptualStyleLoss(meta["layer_weights"], weights, style_weight=400.0)
    x0, gt = torch.from_numpy(arrays["c__B__x"]).double(), torch.from_numpy(arrays["c__B__gt"]).double()
    x = x0.clone().requires_grad_(True)
    tx, tg = [], []
    percep, style = pl.composite(x, gt, trace=tx)
    (percep + style).backward()
    pl.vgg.composite(gt, trace=tg)
    dec = P.decisions_from_trace(pl.vgg, [torch.cat([a, b]) for a, b in zip(tx, tg)], 1, diffs=pl.last_diffs)
    assert list(dec["gram_signs"]) == list(meta["layer_weights"]) and set(dec["gram_signs"]["conv5_4"].unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert "gram_signs" not in P.decisions_from_trace(pl.vgg, [torch.cat([a, b]) for a, b in zip(tx, tg)], 1)
    x2 = x0.clone().requires_grad_(True)
    percep2, style2 = pl.composite(x2, gt, decisions=dec)
    (percep2 + style2).backward()
    close(percep2.detach(), percep.detach(), "percep under its own decisions")
    close(style2.detach(), style.detach(), "style under its own decisions")
    close(x2.grad, x.grad, "d(percep + style)/dx under its own decisions")


def test_the_gram_entries_are_bound_and_refuse_cpu_tensors():
    from grl_image_restoration_amd import _lib, ops

    for name in ("grl_vgg_gram_fwd", "grl_vgg_gram_loss", "grl_vgg_gram_bwd"):
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION >= 40
    with pytest.raises(RuntimeError, match="no CPU fallback"):                  # a missing kernel or device is an error, never eager torch
        ops.vgg_gram(torch.zeros(4, 64), 1, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vgg_gram_bwd(torch.zeros(4, 64), torch.zeros(1, 64, 64), 4, 1.0, torch.zeros(4, 64))


def _gan_setup(disc):
    from grl_image_restoration_amd import GRL
    from oracle import grl_oracle as O

    meta, arrays = disc
    g = GRL(**meta["g_cfg"])
    g.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in g.state_dict().items()}, meta["g_weight_seed"]), strict=True)
    g = g.double().train()
    d = UNetDiscriminatorSN(3, 8, True).double()
    sd = {k[len("d__p__"):]: torch.from_numpy(v.astype(np.float64)) for k, v in arrays.items() if k.startswith("d__p__")}
    for c in SN:
        sd[f"{c}.weight_u"], sd[f"{c}.weight_v"] = torch.from_numpy(arrays[f"d__u0__{c}"]), torch.from_numpy(arrays[f"d__v0__{c}"])
    d.load_state_dict(sd, strict=True)
    d.train()
    opts = torch.optim.Adam(g.parameters(), lr=meta["lr"]), torch.optim.Adam(d.parameters(), lr=meta["lr"])
    batch = tuple(torch.from_numpy(arrays[k]).double() for k in ("s__lq", "s__gt", "s__gt_usm"))
    kw = dict(pixel_weight=meta["pixel_weight"], gan_weight=meta["gan_weight"], gan_loss_weight=meta["gan_loss_weight"], usm_pixel=True, usm_gan=False)
    return g, d, opts, batch, kw


def test_gan_step_with_both_terms_matches_the_reference(fx, disc, weights):
    meta, arrays = fx
    g, d, (opt_g, opt_d), batch, kw = _gan_setup(disc)
    pl = P.PerceptualStyleLoss(meta["layer_weights"], weights, style_weight=meta["step_style_weight"])
    step = GanStep(g, d, opt_g, opt_d, lambda y, t: (y - t).abs().mean(), perceptual=pl, perceptual_weight=meta["step_perceptual_weight"],
                   usm_percep=meta["usm_percep"], **kw)
    want = arrays["q__scalars"]
    for it in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = step(*batch)
        assert list(out) == NAMES_S and float(out["loss_g_style"]) > 0
        for j, n in enumerate(NAMES_S):
            rel = abs(float(out[n]) - want[it, j]) / abs(want[it, j])
            print(f"iteration {it} {n}: {float(out[n]):.12f} against {want[it, j]:.12f} (relative {rel:.2e})")
            assert rel <= 1e-8, (it, n, rel)
    assert all(p.grad is None for p in pl.parameters())


# ---- command line -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    from PIL import Image

    gt, lq = tmp_path_factory.mktemp("style_gt"), tmp_path_factory.mktemp("style_lq")
    g = np.random.RandomState(0)
    for i in range(3):
        Image.fromarray(g.randint(0, 256, (40, 48, 3)).astype(np.uint8)).save(gt / f"im{i}.png")
        Image.fromarray(g.randint(0, 256, (20, 24, 3)).astype(np.uint8)).save(lq / f"im{i}.png")
    return str(gt), str(lq)


GAN_ARGS = ["--task", "sr", "--scale", "2", "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--patch", "8", "--batch", "2",
            "--gan", "--disc-feat", "8", "--usm", "--device", "cpu", "--lr", "1e-3", "--seed", "3"]


def test_style_weight_needs_gan_and_vgg(folders, capsys):
    from grl_image_restoration_amd import train

    gt, lq = folders
    for args in (GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "1", "--style-weight", "400"],                     # --gan without --vgg
                 ["--task", "sr", "--scale", "2", "--gt", gt, "--lq", lq, "--steps", "1", "--device", "cpu", "--style-weight", "400"]):
        with pytest.raises(SystemExit) as e:
            train.main(args)
        assert e.value.code == 2 and "--style-weight needs --gan --vgg" in capsys.readouterr().err


def test_gan_command_line_with_the_style_loss(folders, tmp_path, weights, capsys):
    from grl_image_restoration_amd import train

    gt, lq = folders
    path = tmp_path / "vgg19-dcbb9e9d.pth"
    torch.save({k: v.half() for k, v in weights.items()}, path)
    common = GAN_ARGS + ["--gt", gt, "--lq", lq, "--vgg", str(path), "--usm-percep", "--style-weight", "400"]
    torch.manual_seed(0)
    res = train.main(common + ["--steps", "2", "--out", str(tmp_path / "run")])
    assert res["steps"] == [0, 1] and [list(r) for r in res["gan"]] == [NAMES_S] * 2
    assert all(np.isfinite(list(r.values())).all() and r["loss_g_style"] > 0 and r["loss_g_percep"] > 0 for r in res["gan"])
    for r, loss in zip(res["gan"], res["losses"]):                              # the printed loss is the generator's total
        assert loss == pytest.approx(r["loss_g_pix"] + r["loss_g_percep"] + r["loss_g_style"] + r["loss_g_gan"], rel=1e-6)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("step")]
    assert len(lines) == 2 and all("loss_g_style" in ln for ln in lines)
    obj = torch.load(res["checkpoint"], map_location="cpu", weights_only=False)
    assert obj["args"]["style_weight"] == 400.0 and all(k.startswith(("model.model_g.", "model.model_d.")) for k in obj["state_dict"])
    # --style-weight 0 builds exactly what is built without the option
    torch.manual_seed(0)
    plain = train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--vgg", str(path), "--usm-percep", "--steps", "1", "--style-weight", "0"])
    assert "loss_g_style" not in plain["gan"][0] and plain["gan"][0]["loss_g_percep"] == pytest.approx(res["gan"][0]["loss_g_percep"], rel=1e-6)
    # resume: one more step from the two-step checkpoint, the style term still on
    more = train.main(common + ["--steps", "3", "--resume", res["checkpoint"]])
    assert more["steps"] == [2] and list(more["gan"][0]) == NAMES_S and np.isfinite(list(more["gan"][0].values())).all()
