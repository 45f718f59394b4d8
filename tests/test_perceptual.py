"""The VGG19 perceptual loss on the CPU: the float64 composite of perceptual.py against the reference's own float64 runs
(tests/golden/gan/percep.npz, written by tools/make_golden_vgg.py from models/aux_archs/vgg.py, losses/losses.py:59-172 and
engines/base_gan.py:86-147), ``GanStep`` with the term on, the weight loader and the command line.

Bounds.  Composite: 1e-10 * max(1, max|fixture array|) -- both sides are float64 runs of the same arithmetic, possibly summed in
another order.  ``GanStep``: the seven logged scalars of two iterations to 1e-8 relative."""
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
NAMES = ["loss_g_pix", "loss_g_gan", "loss_d_real", "loss_d_fake", "out_d_real", "out_d_fake"]
NAMES_P = ["loss_g_pix", "loss_g_percep", "loss_g_gan", "loss_d_real", "loss_d_fake", "out_d_real", "out_d_fake"]


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(HERE, "golden", "gan", "percep.npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), {k: z[k] for k in z.files if k != "meta"}


@pytest.fixture(scope="module")
def disc():
    z = np.load(os.path.join(HERE, "golden", "gan", "disc.npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), {k: z[k] for k in z.files if k != "meta"}


@pytest.fixture(scope="module")
def weights(fx):
    return P.seeded_state_dict(fx[0]["vgg_seed"])


def close(got, want, what):
    want = torch.as_tensor(want)
    bound = 1e-10 * max(1.0, float(want.abs().max()))
    err = float((torch.as_tensor(got).double() - want).abs().max())
    print(f"{what}: max|d| {err:.3e} (bound {bound:.1e})")
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("case", ["A", "B", "R"])
def test_composite_matches_the_reference(fx, weights, case):
    meta, arrays = fx
    c = meta["cases"][case]
    pl = P.PerceptualLoss(meta["layer_weights"], weights, use_input_norm=True, range_norm=c["range_norm"], perceptual_weight=c["perceptual_weight"])
    x = torch.from_numpy(arrays[f"c__{case}__x"]).double().requires_grad_(True)
    gt = torch.from_numpy(arrays[f"c__{case}__gt"]).double().requires_grad_(True)
    loss, style = pl(x, gt)
    assert style is None and loss.dtype == torch.float64
    loss.backward()
    close(loss.detach(), arrays[f"c__{case}__loss"], f"{case} loss")
    close(torch.stack(pl.last_layer_means), arrays[f"c__{case}__means"], f"{case} per-layer L1 means")
    close(x.grad, arrays[f"c__{case}__dx"], f"{case} dL/dx")
    assert gt.grad is None and all(p.grad is None and not p.requires_grad for p in pl.parameters())


def test_features_are_taken_before_relu_and_only_borrowed_layers_exist(weights):
    v = P.VGG19Features(["conv2_2", "relu1_1", "pool1"], weights)
    assert v.names[-1] == "conv2_2" and len(v.convs) == 4 and len(list(v.parameters())) == 8
    f = v(torch.rand(1, 3, 16, 18, generator=torch.Generator().manual_seed(0)).double())
    assert list(f) == ["relu1_1", "pool1", "conv2_2"]
    assert tuple(f["pool1"].shape) == (1, 64, 8, 9) and tuple(f["conv2_2"].shape) == (1, 128, 8, 9)
    assert float(f["conv2_2"].min()) < 0 <= float(f["relu1_1"].min())          # before / after ReLU
    assert P.NAMES.index("conv5_4") == 34 and [i for i in P.CONV_INDEX.values()] == [0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34]


def test_own_decisions_reproduce_the_composite_and_the_emulation_runs(fx, weights):
    """The decision-taking forward, fed the decisions of the very run it is compared with, is that run: loss and gradient."""
    meta, arrays = fx
    pl = P.PerceptualLoss(meta["layer_weights"], weights)
    x0, gt = torch.from_numpy(arrays["c__B__x"]).double(), torch.from_numpy(arrays["c__B__gt"]).double()
    x = x0.clone().requires_grad_(True)
    tx, tg = [], []
    loss = pl.composite(x, gt, trace=tx)
    loss.backward()
    pl.vgg.composite(gt, trace=tg)
    dec = P.decisions_from_trace(pl.vgg, [torch.cat([a, b]) for a, b in zip(tx, tg)], 1)
    assert len(dec["masks"]) == 16 and len(dec["pool_idx"]) == 4 and list(dec["signs"]) == list(meta["layer_weights"])
    x2 = x0.clone().requires_grad_(True)
    loss2 = pl.composite(x2, gt, decisions=dec)
    loss2.backward()
    close(loss2.detach(), loss.detach(), "loss under its own decisions")
    close(x2.grad, x.grad, "dL/dx under its own decisions")
    x3 = x0.clone().requires_grad_(True)
    S = P.operand_scale(pl._coefs(*[x0.shape[i] for i in (0, 2, 3)]))
    pl.composite(x3, gt, operand_dtype=torch.float16, decisions=dec, grad_scale=S).backward()
    rel = float((x3.grad - x.grad).abs().max() / x.grad.abs().max())
    print(f"fp16-operand emulation under shared decisions: max|g_emu - g_64| / max|g| = {rel:.2e}")
    assert 0 < rel < 5e-3                                                      # fp16 operands: a few 2^-11, not zero and not a flip
    # at perceptual_weight 1e-6 the tap terms (~1e-9) are below fp16's subnormals: without a scale the emulation loses them
    pl6 = P.PerceptualLoss(meta["layer_weights"], weights, perceptual_weight=1e-6)
    x4 = x0.clone().requires_grad_(True)
    pl6.composite(x4, gt, operand_dtype=torch.float16, decisions=dec, grad_scale=1.0).backward()
    assert float((x4.grad * 1e6 - x.grad).abs().max() / x.grad.abs().max()) > 10 * rel
    x5 = x0.clone().requires_grad_(True)
    pl6.composite(x5, gt, operand_dtype=torch.float16, decisions=dec, grad_scale=P.operand_scale(pl6._coefs(1, 19, 17))).backward()
    assert float((x5.grad * 1e6 - x.grad).abs().max() / x.grad.abs().max()) < 5e-3             # under the chain's scale: fp16 roundings again


def test_operand_scale_is_a_power_of_two_from_the_coefficients():
    for coefs, up in (([1e-8, 3e-6], 1.0), ([0.1 / 64, 1.0 / 2], 1e-3), ([5.0], -2.0)):
        S = P.operand_scale(coefs, up)
        k = max(coefs) * abs(up) * S
        assert np.log2(S) == round(np.log2(S)) and 2.0 ** -4 < k <= 2.0 ** -3, (coefs, up, S, k)
    assert P.operand_scale([1.0], 0.0) == 1.0 and P.operand_scale([1.0], float("inf")) == 1.0


def test_weight_loader(tmp_path, weights):
    path = tmp_path / "vgg19-dcbb9e9d.pth"
    sd = {k: v.half() for k, v in weights.items()}
    sd.update({"classifier.0.weight": torch.zeros(4, 4), "classifier.0.bias": torch.zeros(4)})
    torch.save(sd, path)
    got = P.load_vgg19(str(path))
    v = P.VGG19Features(list(P.GAN_LAYER_WEIGHTS), got)                          # classifier.* ignored
    assert len(v.weights) == 16 and torch.equal(v.weights[15], weights["features.34.weight"]) and v.weights[0].dtype == torch.float32
    assert not any(p.requires_grad for p in v.parameters())
    short = P.VGG19Features(["conv1_2"], {k: t for k, t in got.items() if k.startswith(("features.0.", "features.2."))})
    assert len(short.weights) == 2                                              # borrows only up to the last requested layer
    bad = dict(got)
    del bad["features.21.bias"]
    with pytest.raises(KeyError, match="features.21.bias"):
        P.VGG19Features(list(P.GAN_LAYER_WEIGHTS), bad)
    bad = dict(got)
    bad["features.5.weight"] = torch.zeros(128, 64, 1, 1)
    with pytest.raises(ValueError, match="features.5.weight"):
        P.VGG19Features(list(P.GAN_LAYER_WEIGHTS), bad)


def test_argument_errors(weights):
    pl = P.PerceptualLoss(P.GAN_LAYER_WEIGHTS, weights)
    with pytest.raises(ValueError, match="at least 16 x 16"):
        pl(torch.zeros(1, 3, 15, 16), torch.zeros(1, 3, 15, 16))
    with pytest.raises(ValueError, match="at least 16 x 16"):
        pl.vgg(torch.zeros(1, 3, 32, 8))
    for kw in (dict(style_weight=1.0), dict(criterion="l2"), dict(criterion="fro")):
        with pytest.raises(NotImplementedError):
            P.PerceptualLoss(P.GAN_LAYER_WEIGHTS, weights, **kw)
    with pytest.raises(ValueError, match="not a layer of vgg19"):
        P.VGG19Features(["conv6_1"], weights)
    assert P.PerceptualLoss(P.GAN_LAYER_WEIGHTS, weights, perceptual_weight=0.0)(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16)) == (None, None)


def test_hip_chain_names_the_tap_sets_it_does_not_cover(weights):
    """Host logic only: which tap sets the CUDA chain takes (a tap closes its block or is the last layer borrowed)."""
    assert P.VGG19Features(list(P.GAN_LAYER_WEIGHTS), weights)._hip_plan() == \
        [(False, False), (True, True)] * 2 + ([(False, False)] * 3 + [(True, True)]) * 2 + [(False, False)] * 3 + [(True, False)]
    assert P.VGG19Features(["conv1_2", "conv2_1"], weights)._hip_plan() == [(False, False), (True, True), (True, False)]
    # an untapped convolution that closes a block goes through the tap kernel with coefficient 0: a single conv5_4 tap is covered
    single = P.PerceptualLoss({"conv5_4": 1.0}, weights)
    assert single.vgg._hip_plan() == [(False, False), (False, True)] * 2 + ([(False, False)] * 3 + [(False, True)]) * 2 + [(False, False)] * 3 + [(True, False)]
    coefs = single._coefs(2, 32, 32)
    assert len(coefs) == 16 and coefs[:15] == [0.0] * 15 and coefs[15] == 1.0 / (2 * 512 * 2 * 2)
    for taps, word in ((["conv1_2", "conv2_2", "conv3_2", "conv3_4"], "conv3_2"), (["relu1_2"], "relu1_2")):
        with pytest.raises(NotImplementedError, match=word):
            P.VGG19Features(taps, weights)._hip_plan()


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


def test_gan_step_with_the_perceptual_term_matches_the_reference(fx, disc, weights):
    meta, arrays = fx
    g, d, (opt_g, opt_d), batch, kw = _gan_setup(disc)
    pl = P.PerceptualLoss(meta["layer_weights"], weights)
    step = GanStep(g, d, opt_g, opt_d, lambda y, t: (y - t).abs().mean(), perceptual=pl, perceptual_weight=meta["step_perceptual_weight"],
                   usm_percep=meta["usm_percep"], **kw)
    want = arrays["p__scalars"]
    for it in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = step(*batch)
        assert list(out) == NAMES_P and float(out["loss_g_percep"]) > 0
        for j, n in enumerate(NAMES_P):
            rel = abs(float(out[n]) - want[it, j]) / abs(want[it, j])
            print(f"iteration {it} {n}: {float(out[n]):.12f} against {want[it, j]:.12f} (relative {rel:.2e})")
            assert rel <= 1e-8, (it, n, rel)
    assert all(p.grad is None for p in pl.parameters())


def test_gan_step_without_the_term_is_what_it_was(disc):
    g, d, (opt_g, opt_d), batch, kw = _gan_setup(disc)
    step = GanStep(g, d, opt_g, opt_d, lambda y, t: (y - t).abs().mean(), perceptual=None, usm_percep=True, **kw)
    want = disc[1]["s__scalars"]
    for it in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = step(*batch)
        assert list(out) == NAMES
        for j, n in enumerate(NAMES):
            assert abs(float(out[n]) - want[it, j]) / abs(want[it, j]) <= 1e-8, (it, n)


# ---- command line -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    from PIL import Image

    gt, lq = tmp_path_factory.mktemp("percep_gt"), tmp_path_factory.mktemp("percep_lq")
    g = np.random.RandomState(0)
    for i in range(3):
        Image.fromarray(g.randint(0, 256, (40, 48, 3)).astype(np.uint8)).save(gt / f"im{i}.png")
        Image.fromarray(g.randint(0, 256, (20, 24, 3)).astype(np.uint8)).save(lq / f"im{i}.png")
    return str(gt), str(lq)


GAN_ARGS = ["--task", "sr", "--scale", "2", "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--patch", "8", "--batch", "2",
            "--gan", "--disc-feat", "8", "--usm", "--device", "cpu", "--lr", "1e-3", "--seed", "3"]


def test_vgg_options_belong_to_gan(folders, capsys):
    from grl_image_restoration_amd import train

    gt, lq = folders
    base = ["--task", "sr", "--scale", "2", "--gt", gt, "--lq", lq, "--steps", "1", "--device", "cpu"]
    for extra in (["--vgg", "x.pth"], ["--usm-percep"], ["--perceptual-weight", "0.5"]):
        with pytest.raises(SystemExit) as e:
            train.main(base + extra)
        assert e.value.code == 2 and "belong to --gan" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                                        # --usm-percep without --vgg
        train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "1", "--usm-percep"])
    assert e.value.code == 2 and "need --vgg" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                                        # GT patch side 4 * 2 = 8 < 16
        train.main([a if a != "8" or GAN_ARGS[i - 1] != "--patch" else "4" for i, a in enumerate(GAN_ARGS)]
                   + ["--gt", gt, "--lq", lq, "--steps", "1", "--vgg", "x.pth"])
    assert e.value.code == 2 and "at least 16" in capsys.readouterr().err


def test_gan_command_line_with_vgg(folders, tmp_path, weights):
    from grl_image_restoration_amd import train

    gt, lq = folders
    path = tmp_path / "vgg19-dcbb9e9d.pth"
    torch.save({k: v.half() for k, v in weights.items()}, path)
    torch.manual_seed(0)
    res = train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "2", "--vgg", str(path), "--usm-percep", "--out", str(tmp_path / "run")])
    assert res["steps"] == [0, 1] and [list(r) for r in res["gan"]] == [NAMES_P] * 2
    assert all(np.isfinite(list(r.values())).all() and r["loss_g_percep"] > 0 for r in res["gan"])
    for r, loss in zip(res["gan"], res["losses"]):                              # the printed loss is the generator's total
        assert loss == pytest.approx(r["loss_g_pix"] + r["loss_g_percep"] + r["loss_g_gan"], rel=1e-6)
    torch.manual_seed(0)
    plain = train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "1"])
    assert list(plain["gan"][0]) == NAMES and plain["gan"][0]["loss_g_pix"] == pytest.approx(res["gan"][0]["loss_g_pix"], rel=1e-6)
    obj = torch.load(res["checkpoint"], map_location="cpu", weights_only=False)  # the frozen VGG stays out of the checkpoint
    assert all(k.startswith(("model.model_g.", "model.model_d.")) for k in obj["state_dict"])
