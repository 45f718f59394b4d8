"""Writes tests/golden/gan/percep.npz: the reference's own VGG19 perceptual loss and the GAN alternation with that term on, in float64
(data only, under 512 KB).

Needs the reference tree (oracle/refshim.py: GRL_REFERENCE_ROOT).  ``models/aux_archs/vgg.py`` and ``losses/losses.py`` are loaded by
file path.  The first imports ``torchvision.models.vgg``, which is not installed: this tool registers a small stand-in module of its
own whose ``vgg19(pretrained=False)`` builds torchvision's ``features`` stack (Conv2d 3x3 pad 1 / ReLU(inplace) / MaxPool2d(2, 2) in
the layout 64 64 M 128 128 M 256 x4 M 512 x4 M 512 x4 M), so the keys are torchvision's ``features.N.weight`` / ``.bias``.  The reference
reads its weights from ``experiments/pretrained_models/vgg19-dcbb9e9d.pth`` relative to the working directory: the tool works in a
temporary directory that holds the seeded weights under that name, so the reference takes its ``pretrained=False`` + ``load_state_dict``
branch (vgg.py:204-209) and nothing is downloaded.

Weights: ``grl_image_restoration_amd.perceptual.seeded_state_dict(meta["vgg_seed"])`` -- He-scaled draws from a seeded generator rounded
to fp16-representable values; reproducible from the seed, so the 80 MB are never stored.

Group ``c__`` -- ``losses.PerceptualLoss(layer_weights=meta["layer_weights"], ...)`` as config/loss/gan_training_loss.yaml builds it,
``.double()``.  Per case (A (2, 3, 16, 24), B (1, 3, 19, 17): both sides odd, R (1, 3, 16, 16): range_norm with inputs in [-1, 1] and
perceptual_weight 0.5):
  c__<case>__x, c__<case>__gt     inputs (float32 values; x = clamp(gt + 0.1 noise))
  c__<case>__loss                 percep_loss
  c__<case>__means [5]            L1Loss per tapped layer, in layer order, before the layer weights
  c__<case>__dx                   d percep_loss / d x

Group ``p__`` -- two iterations of the alternation (engines/base_gan.py:86-147) exactly as make_golden_gan.py's ``s__`` group runs them
(same generator, discriminator start state ``d__`` of disc.npz, inputs ``s__lq`` / ``s__gt`` / ``s__gt_usm``, restored 16 x 16, Adam
1e-3 twice, L1, weights 1 / 1 / 0.1) with the perceptual term on at weight 1 against ``gt`` (use_usm_percep false):
  p__scalars [2, 7]: loss_g_pix, loss_g_percep, loss_g_gan, loss_d_real, loss_d_fake, out_d_real, out_d_fake per iteration

    python tools/make_golden_vgg.py [--out tests/golden/gan]
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "gan")
VGG_SEED = 7
LAYER_WEIGHTS = {"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1, "conv4_4": 1, "conv5_4": 1}      # gan_training_loss.yaml
CASES = [("A", (2, 3, 16, 24), False, 1.0), ("B", (1, 3, 19, 17), False, 1.0), ("R", (1, 3, 16, 16), True, 0.5)]
CFG19 = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class _StandInVGG(nn.Module):
    def __init__(self):
        super().__init__()
        layers, cin = [], 3
        for v in CFG19:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.features = nn.Sequential(*layers)


def reference_perceptual_loss():
    """The reference's ``losses.PerceptualLoss`` class, with the stand-in torchvision module in place."""
    from oracle import refshim

    def vgg19(pretrained=False, **kw):
        assert not pretrained, "the stand-in never downloads: the weights file must exist"
        return _StandInVGG()

    tv, tvm, tvv = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.models.vgg")
    tvv.vgg19 = vgg19
    tv.models, tvm.vgg = tvm, tvv
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.models.vgg": tvv})
    refshim.import_reference_grl()             # puts the reference's ``models`` package on the path
    _load("models.aux_archs.vgg", os.path.join(refshim.REFERENCE_ROOT, "models", "aux_archs", "vgg.py"))
    return _load("ref_losses", os.path.join(refshim.REFERENCE_ROOT, "losses", "losses.py")).PerceptualLoss


def build_cases(PL):
    arrays = {}
    g = torch.Generator().manual_seed(11)
    for name, shape, range_norm, pw in CASES:
        gt = torch.rand(shape, generator=g)
        x = (gt + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
        if range_norm:
            gt, x = gt * 2 - 1, x * 2 - 1
        arrays[f"c__{name}__x"], arrays[f"c__{name}__gt"] = x.numpy(), gt.numpy()
        pl = PL(layer_weights=dict(LAYER_WEIGHTS), vgg_type="vgg19", use_input_norm=True, range_norm=range_norm, perceptual_weight=pw,
                style_weight=0, criterion="l1").double()
        xg = x.double().requires_grad_(True)
        loss, style = pl(xg, gt.double())
        assert style is None
        loss.backward()
        fx, fg = pl.vgg(x.double()), pl.vgg(gt.double())
        assert list(fx) == list(LAYER_WEIGHTS)
        arrays[f"c__{name}__loss"] = np.float64(loss.item())
        arrays[f"c__{name}__means"] = np.array([torch.nn.L1Loss()(fx[k], fg[k]).item() for k in fx], dtype=np.float64)
        arrays[f"c__{name}__dx"] = xg.grad.numpy()
        print(f"case {name}: loss {loss.item():.8f}  means {arrays[f'c__{name}__means']}  max|dx| {xg.grad.abs().max().item():.3e}")
    return arrays


def build_steps(PL, out_dir):
    """make_golden_gan.build_steps with the perceptual term between the pixel and the GAN term (base_gan.py:98-126)."""
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
    pl = PL(layer_weights=dict(LAYER_WEIGHTS), vgg_type="vgg19", use_input_norm=True, range_norm=False, perceptual_weight=1.0,
            style_weight=0, criterion="l1").double()
    opt_g, opt_d = torch.optim.Adam(gnet.parameters(), lr=1e-3), torch.optim.Adam(d.parameters(), lr=1e-3)
    rows = []
    for it in range(2):
        for p in d.parameters():
            p.requires_grad_(False)
        restored = gnet(lq)
        loss_g_pix = torch.nn.L1Loss()(restored, gt_usm) * 1.0
        loss_g_percep, _ = pl(restored, gt)
        loss_g_percep = loss_g_percep * 1.0
        loss_g_gan = gan.bce(d(restored), True) * 0.1 * 1.0
        opt_g.zero_grad()
        (loss_g_pix + loss_g_percep + loss_g_gan).backward()
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
        rows.append([loss_g_pix.item(), loss_g_percep.item(), loss_g_gan.item(), loss_d_real.item(), loss_d_fake.item(),
                     real.detach().mean().item(), fake.detach().mean().item()])
        print(f"iteration {it}: {rows[-1]}")
    return {"p__scalars": np.array(rows, dtype=np.float64)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args(argv)
    out_dir = os.path.abspath(a.out)
    from grl_image_restoration_amd.perceptual import seeded_state_dict

    PL = reference_perceptual_loss()
    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "experiments", "pretrained_models"))
        torch.save(seeded_state_dict(VGG_SEED), os.path.join(tmp, "experiments", "pretrained_models", "vgg19-dcbb9e9d.pth"))
        os.chdir(tmp)
        try:
            arrays = build_cases(PL)
            arrays.update(build_steps(PL, out_dir))
        finally:
            os.chdir(here)
    meta = dict(vgg_seed=VGG_SEED, layer_weights=LAYER_WEIGHTS, cases={n: dict(shape=list(s), range_norm=r, perceptual_weight=w) for n, s, r, w in CASES},
                step_perceptual_weight=1.0, usm_percep=False, torch=torch.__version__)
    path = os.path.join(out_dir, "percep.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    print(f"wrote {path}: {len(arrays)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
