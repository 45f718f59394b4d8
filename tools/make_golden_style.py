"""Writes tests/golden/gan/style.npz: the reference's own PerceptualLoss with the style term on (losses/losses.py:59-187, Gram matrices of
the five tapped VGG19 features, criterion "l1") and the GAN alternation with both terms, in float64 (data only, under 512 KB).

Needs the reference tree (oracle/refshim.py: GRL_REFERENCE_ROOT).  ``tools/make_golden_vgg.py`` is loaded by file path for its
``reference_perceptual_loss`` (the reference's class behind a stand-in torchvision module) and its case list; weights, working
directory and inputs are that tool's: ``seeded_state_dict(7)`` under ``experiments/pretrained_models/vgg19-dcbb9e9d.pth`` of a temporary
directory, cases A (2, 3, 16, 24) and B (1, 3, 19, 17) drawn from the same generator in the same order (so ``c__A__x`` here is
``c__A__x`` of percep.npz).

Style weights.  At ``style_weight = 1`` the style term is 1/403 to 1/457 of the perceptual term on these weights (measured by this tool
on (2, 3, 16, 24), (1, 3, 19, 17) and (2, 3, 32, 32) and recorded in meta["percep_over_style_at_weight_1"]); the fixture uses 400
("balanced") and 40 000 ("style-dominated").

Group ``c__`` -- per case:
  c__<case>__x, c__<case>__gt           inputs (float32 values; x = clamp(gt + 0.1 noise))
  c__<case>__gram_means [5]             L1Loss(gram(f(x)), gram(f(gt))) per tapped layer, in layer order, before the weights
  c__<case>__w<W>__percep, __style      the two returned terms at perceptual_weight 1 and style_weight W (400, 40000)
  c__<case>__w<W>__dx                   d (percep + style) / d x
Group ``o__`` -- style only (perceptual_weight 0, style_weight 400) on case A: the reference returns (None, style)
  o__A__style, o__A__dx
Group ``q__`` -- two iterations of the alternation exactly as make_golden_vgg.py's ``p__`` group runs them (same generator, same
discriminator start state, same inputs, Adam 1e-3 twice, L1, weights 1 / 1 / 0.1, perceptual weight 1 against ``gt``) with
style_weight 400:
  q__scalars [2, 8]: loss_g_pix, loss_g_percep, loss_g_style, loss_g_gan, loss_d_real, loss_d_fake, out_d_real, out_d_fake

    python tools/make_golden_style.py [--out tests/golden/gan]
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "gan")
WEIGHTS = (400.0, 40000.0)
STEP_STYLE_WEIGHT = 400.0
RATIO_SHAPES = [(2, 3, 16, 24), (1, 3, 19, 17), (2, 3, 32, 32)]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _make(PL, V, perceptual_weight, style_weight):
    return PL(layer_weights=dict(V.LAYER_WEIGHTS), vgg_type="vgg19", use_input_norm=True, range_norm=False, perceptual_weight=perceptual_weight,
              style_weight=style_weight, criterion="l1").double()


def _pair(shape, g):
    gt = torch.rand(shape, generator=g)
    return (gt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1), gt


def build_cases(PL, V):
    arrays = {}
    g = torch.Generator().manual_seed(11)                   # make_golden_vgg.build_cases: the same draws in the same order
    for name, shape, range_norm, _ in V.CASES[:2]:
        assert not range_norm
        x, gt = _pair(shape, g)
        arrays[f"c__{name}__x"], arrays[f"c__{name}__gt"] = x.numpy(), gt.numpy()
        for W in WEIGHTS:
            pl = _make(PL, V, 1.0, W)
            xg = x.double().requires_grad_(True)
            percep, style = pl(xg, gt.double())
            (percep + style).backward()
            tag = f"c__{name}__w{int(W)}"
            arrays[f"{tag}__percep"], arrays[f"{tag}__style"] = np.float64(percep.item()), np.float64(style.item())
            arrays[f"{tag}__dx"] = xg.grad.numpy()
            print(f"case {name} style_weight {W:g}: percep {percep.item():.8f} style {style.item():.8f} max|dx| {xg.grad.abs().max().item():.3e}")
        fx, fg = pl.vgg(x.double()), pl.vgg(gt.double())
        assert list(fx) == list(V.LAYER_WEIGHTS)
        arrays[f"c__{name}__gram_means"] = np.array([torch.nn.L1Loss()(pl._gram_mat(fx[k]), pl._gram_mat(fg[k])).item() for k in fx], dtype=np.float64)
        print(f"case {name}: Gram L1 means {arrays[f'c__{name}__gram_means']}")
    x, gt = torch.from_numpy(arrays["c__A__x"]), torch.from_numpy(arrays["c__A__gt"])
    xg = x.double().requires_grad_(True)
    percep, style = _make(PL, V, 0.0, WEIGHTS[0])(xg, gt.double())
    assert percep is None
    style.backward()
    arrays["o__A__style"], arrays["o__A__dx"] = np.float64(style.item()), xg.grad.numpy()
    print(f"style only: {style.item():.8f} max|dx| {xg.grad.abs().max().item():.3e}")
    return arrays


def measure_ratios(PL, V):
    """percep / style at style_weight 1 on the three shapes the weights were chosen from."""
    out = {}
    g = torch.Generator().manual_seed(11)
    pl = _make(PL, V, 1.0, 1.0)
    for shape in RATIO_SHAPES:
        x, gt = _pair(shape, g)
        with torch.no_grad():
            percep, style = pl(x.double(), gt.double())
        out["x".join(str(v) for v in shape)] = percep.item() / style.item()
        print(f"{shape}: percep / style at style_weight 1 = {out['x'.join(str(v) for v in shape)]:.1f}")
    return out


def build_steps(PL, V, out_dir):
    """make_golden_vgg.build_steps with the style term after the perceptual one (base_gan.py:105-116)."""
    gan = _load("make_golden_gan", os.path.join(ROOT, "tools", "make_golden_gan.py"))
    from grl_image_restoration_amd.presets import make_config
    from oracle import grl_oracle as O
    from oracle import refshim

    z = np.load(os.path.join(out_dir, "disc.npz"), allow_pickle=False)
    state = {k[len("d__p__"):]: torch.from_numpy(z[k].astype(np.float64)) for k in z.files if k.startswith("d__p__")}
    for c in gan.SN:
        state[f"{c}.weight_u"], state[f"{c}.weight_v"] = torch.from_numpy(z[f"d__u0__{c}"]), torch.from_numpy(z[f"d__v0__{c}"])
    D = gan.reference_discriminator()
    GRL = refshim.import_reference_grl()
    kw = dict(gan.G_CFG)
    cfg = make_config(kw.pop("model"), kw.pop("geometry"), **kw)
    torch.manual_seed(0)
    gnet = GRL(**cfg)
    full = gnet.state_dict()
    full.update(O.seeded_state_dict({k: tuple(v.shape) for k, v in full.items()}, seed=0))
    gnet.load_state_dict(full, strict=True)
    gnet = gnet.double().train()
    d = gan.fresh(D, state).train()
    lq, gt, gt_usm = (torch.from_numpy(z[k]).double() for k in ("s__lq", "s__gt", "s__gt_usm"))
    pl = _make(PL, V, 1.0, STEP_STYLE_WEIGHT)
    opt_g, opt_d = torch.optim.Adam(gnet.parameters(), lr=1e-3), torch.optim.Adam(d.parameters(), lr=1e-3)
    rows = []
    for it in range(2):
        for p in d.parameters():
            p.requires_grad_(False)
        restored = gnet(lq)
        loss_g_pix = torch.nn.L1Loss()(restored, gt_usm) * 1.0
        loss_g_percep, loss_g_style = pl(restored, gt)
        loss_g_percep, loss_g_style = loss_g_percep * 1.0, loss_g_style * 1.0
        loss_g_gan = gan.bce(d(restored), True) * 0.1 * 1.0
        opt_g.zero_grad()
        (loss_g_pix + loss_g_percep + loss_g_style + loss_g_gan).backward()
        assert all(p.grad is None for p in d.parameters()) and all(p.grad is None for p in pl.parameters())
        opt_g.step()
        for p in d.parameters():
            p.requires_grad_(True)
        for p in gnet.parameters():
            p.requires_grad_(False)
        restored = gnet(lq)
        real = d(gt)
        loss_d_real = gan.bce(real, True)
        fake = d(restored.detach())
        loss_d_fake = gan.bce(fake, False)
        opt_d.zero_grad()
        (loss_d_real + loss_d_fake).backward()
        opt_d.step()
        opt_d.zero_grad()
        for p in gnet.parameters():
            p.requires_grad_(True)
        rows.append([loss_g_pix.item(), loss_g_percep.item(), loss_g_style.item(), loss_g_gan.item(), loss_d_real.item(), loss_d_fake.item(),
                     real.detach().mean().item(), fake.detach().mean().item()])
        print(f"iteration {it}: {rows[-1]}")
    return {"q__scalars": np.array(rows, dtype=np.float64)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args(argv)
    out_dir = os.path.abspath(a.out)
    from grl_image_restoration_amd.perceptual import seeded_state_dict

    V = _load("make_golden_vgg", os.path.join(ROOT, "tools", "make_golden_vgg.py"))
    PL = V.reference_perceptual_loss()
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "experiments", "pretrained_models"))
        torch.save(seeded_state_dict(V.VGG_SEED), os.path.join(tmp, "experiments", "pretrained_models", "vgg19-dcbb9e9d.pth"))
        os.chdir(tmp)
        try:
            arrays = build_cases(PL, V)
            ratios = measure_ratios(PL, V)
            arrays.update(build_steps(PL, V, out_dir))
        finally:
            os.chdir(here)
    meta = dict(vgg_seed=V.VGG_SEED, layer_weights=V.LAYER_WEIGHTS, cases={n: dict(shape=list(s)) for n, s, _, _ in V.CASES[:2]},
                style_weights=list(WEIGHTS), style_only=dict(case="A", perceptual_weight=0.0, style_weight=WEIGHTS[0]),
                percep_over_style_at_weight_1=ratios, step_perceptual_weight=1.0, step_style_weight=STEP_STYLE_WEIGHT, usm_percep=False,
                torch=torch.__version__)
    path = os.path.join(out_dir, "style.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    print(f"wrote {path}: {len(arrays)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
