"""Writes tests/golden/gan/disc.npz, disc_grads.npz and disc_grads_B.npz: the reference's own U-Net discriminator and GAN alternation
in float64 (data only; the parameter gradients ``d__A__g__`` / ``d__B__g__`` have a file per case: with either of them disc.npz would
be over 512 KB).

Needs the reference tree (oracle/refshim.py: GRL_REFERENCE_ROOT).  ``models/aux_archs/discriminator.py`` is loaded by file
path -- it imports with torch alone -- and run on the CPU in float64.  ``losses/losses.py`` cannot be imported without torchvision,
so the vanilla GAN loss is ``torch.nn.BCEWithLogitsLoss`` called directly against constant labels (losses.py:212, 267-268, 290-293).

Group ``d__`` -- the discriminator.  ``UNetDiscriminatorSN(3, 8, True)`` (68 649 parameters; at num_feat 64 the state is 17.6 MB).
Every parameter is rounded to an fp16-representable value and stored as fp16; every run below is made on exactly those values, so
an fp16-operand kernel sees no weight rounding.  u / v start from ``d__u0__convN`` / ``d__v0__convN`` (five power iterations from
the random start, as a trained checkpoint has them).  Per case (A: (2, 3, 16, 24),
B: (1, 3, 8, 8)), every run starting again from the stored state:
  d__<case>__x, d__<case>__xf        the two inputs (float32 values in [0, 1]): "real" and "fake"
  d__<case>__eval                    eval-mode logits of x
  d__<case>__train<k>, d__<case>__u<k>__convN, d__<case>__v<k>__convN   k = 1..3: logits of three consecutive train-mode forwards of x
                                     and the buffers after each
  d__<case>__gx                      gradient of BCE(D(x), 1) with respect to x (train mode: the generator-side GAN loss)
  d__<case>__dloss                   BCE(D(x), 1) + BCE(D(xf), 0) in train mode (real first)
  d__<case>__g__<parameter>          its gradient with respect to every weight_orig / weight / bias (disc_grads.npz: case A,
                                     disc_grads_B.npz: case B).  In float64 the parameter gradients of one case are 549 KB, and every
                                     file stays under 512 KB: tensors above 2048 elements are stored as int32 fixed point over their own max-abs (``..__q`` and ``..__qmax``:
                                     value = q * qmax / 2^31, off by at most qmax * 2^-32 <= 4.7e-11 -- asserted: qmax <= 0.2 -- under half
                                     of the 1e-10 the CPU test allows); the others as float64.

Group ``s__`` -- two iterations of the alternation (engines/base_gan.py:86-147) with the reference's own GRL as the generator,
built through oracle/refshim.py as oracle/make_golden.py does: GRL-Tiny cut to depths [1], windows and stripes 8 x 8, upscale 2, drop path 0, LQ 8 x 8 (restored
16 x 16), batch 2, float64, ``torch.optim.Adam`` (lr 1e-3 for both) and L1; pixel weight 1, GAN weight 1, GAN loss weight 0.1; the
pixel target is ``gt_usm``, the discriminator's real input ``gt`` (use_usm_pixel: True, use_usm_gan: False of bsr/grl.yaml).
  meta["g_cfg"] (the constructor arguments; the weights are oracle.grl_oracle.seeded_state_dict(shapes, meta["g_weight_seed"]), reproducible
  without the reference, cast to float64), s__lq, s__gt, s__gt_usm
  s__scalars [2, 6]: loss_g_pix, loss_g_gan, loss_d_real, loss_d_fake, out_d_real, out_d_fake per iteration
  s__u3__convN / s__u6__convN       u after iteration 1 / 2 (three D forwards each)
The discriminator of this group starts from the ``d__`` state.

    python tools/make_golden_gan.py [--out tests/golden/gan]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "gan")
CASES = [("A", (2, 3, 16, 24)), ("B", (1, 3, 8, 8))]
SN = [f"conv{i}" for i in range(1, 9)]
G_CFG = dict(model="tiny", geometry="dm", upscale=2, img_size=8, depths=[1], num_heads_window=[2], num_heads_stripe=[2],
             window_size=8, stripe_size=[8, 8], anchor_window_down_factor=2, drop_path_rate=0.0)


def reference_discriminator():
    from oracle import refshim

    path = os.path.join(refshim.REFERENCE_ROOT, "models", "aux_archs", "discriminator.py")
    spec = importlib.util.spec_from_file_location("ref_discriminator", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.UNetDiscriminatorSN


def bce(logits, real: bool):
    return torch.nn.BCEWithLogitsLoss()(logits, logits.new_ones(logits.size()) * (1.0 if real else 0.0))


def fresh(D, state):
    d = D(3, 8, True).double()
    d.load_state_dict(state, strict=True)
    return d


def build_disc():
    D = reference_discriminator()
    torch.manual_seed(0)
    d = D(3, 8, True).train()
    with torch.no_grad():                      # u / v as a trained checkpoint has them: five power iterations from the random start
        for _ in range(5):                     # (sigma of a fresh random pair is near zero and the logits are in the millions)
            d(torch.zeros(1, 3, 8, 8))
    state = {}
    for k, v in d.state_dict().items():
        v = v.detach().clone()
        if not (k.endswith("weight_u") or k.endswith("weight_v")):
            v = v.to(torch.float16).to(torch.float32)                  # fp16-representable parameters
        state[k] = v.double()
    assert len(state) == 28 and sum(v.numel() for k, v in state.items() if k[-2:] not in ("_u", "_v")) == 68649
    arrays = {}
    for k, v in state.items():
        if k.endswith("weight_u"):
            arrays[f"d__u0__{k.split('.')[0]}"] = v.numpy()
        elif k.endswith("weight_v"):
            arrays[f"d__v0__{k.split('.')[0]}"] = v.numpy()
        else:
            arrays[f"d__p__{k}"] = v.numpy().astype(np.float16)
    g = torch.Generator().manual_seed(1)
    for name, shape in CASES:
        x, xf = torch.rand(shape, generator=g).double(), torch.rand(shape, generator=g).double()
        arrays[f"d__{name}__x"], arrays[f"d__{name}__xf"] = x.float().numpy(), xf.float().numpy()
        d = fresh(D, state).eval()
        with torch.no_grad():
            arrays[f"d__{name}__eval"] = d(x).numpy()
        d = fresh(D, state).train()
        for k in (1, 2, 3):
            with torch.no_grad():
                arrays[f"d__{name}__train{k}"] = d(x).numpy()
            for c in SN:
                arrays[f"d__{name}__u{k}__{c}"] = getattr(d, c).weight_u.numpy().copy()
                arrays[f"d__{name}__v{k}__{c}"] = getattr(d, c).weight_v.numpy().copy()
        d = fresh(D, state).train()
        xg = x.clone().requires_grad_(True)
        bce(d(xg), True).backward()
        arrays[f"d__{name}__gx"] = xg.grad.numpy()
        d = fresh(D, state).train()
        loss = bce(d(x), True) + bce(d(xf), False)
        loss.backward()
        arrays[f"d__{name}__dloss"] = np.float64(loss.item())
        for k, p in d.named_parameters():
            gk = p.grad.numpy()
            if gk.size > 2048:
                qmax = float(np.abs(gk).max())
                assert 0 < qmax <= 0.2, (name, k, qmax)
                arrays[f"d__{name}__g__{k}__q"] = np.rint(gk / qmax * 2.0 ** 31).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)
                arrays[f"d__{name}__g__{k}__qmax"] = np.float64(qmax)
            else:
                arrays[f"d__{name}__g__{k}"] = gk
        print(f"case {name}: max|logit| {np.abs(arrays[f'd__{name}__eval']).max():.4f}  D loss {loss.item():.6f}")
    return arrays, state, D


def build_steps(state, D):
    from grl_image_restoration_amd.presets import make_config
    from oracle import grl_oracle as O
    from oracle import refshim

    GRL = refshim.import_reference_grl()
    kw = dict(G_CFG)
    cfg = make_config(kw.pop("model"), kw.pop("geometry"), **kw)
    torch.manual_seed(0)
    gnet = GRL(**cfg)
    shapes = {k: tuple(v.shape) for k, v in gnet.state_dict().items()}
    sd = O.seeded_state_dict(shapes, seed=0)
    full = gnet.state_dict()
    full.update(sd)
    gnet.load_state_dict(full, strict=True)
    gnet = gnet.double().train()
    d = fresh(D, state).train()
    g = torch.Generator().manual_seed(2)
    lq, gt, gt_usm = (torch.rand(2, 3, 8, 8, generator=g).double(), torch.rand(2, 3, 16, 16, generator=g).double(),
                      torch.rand(2, 3, 16, 16, generator=g).double())
    arrays = {"s__lq": lq.float().numpy(), "s__gt": gt.float().numpy(), "s__gt_usm": gt_usm.float().numpy()}
    opt_g = torch.optim.Adam(gnet.parameters(), lr=1e-3)
    opt_d = torch.optim.Adam(d.parameters(), lr=1e-3)
    rows = []
    for it in range(2):
        # optimizer 0: Lightning's toggle_optimizer turns the other optimizer's parameters off
        for p in d.parameters():
            p.requires_grad_(False)
        restored = gnet(lq)
        loss_g_pix = torch.nn.L1Loss()(restored, gt_usm) * 1.0
        loss_g_gan = bce(d(restored), True) * 0.1 * 1.0
        opt_g.zero_grad()
        (loss_g_pix + loss_g_gan).backward()
        assert all(p.grad is None for p in d.parameters())
        opt_g.step()
        for p in d.parameters():
            p.requires_grad_(True)
        # optimizer 1: self(batch) again -- the updated generator, train mode
        for p in gnet.parameters():
            p.requires_grad_(False)
        restored = gnet(lq)
        real = d(gt)
        loss_d_real = bce(real, True)
        fake = d(restored.detach())
        loss_d_fake = bce(fake, False)
        opt_d.zero_grad()
        (loss_d_real + loss_d_fake).backward()
        opt_d.step()
        opt_d.zero_grad()                      # (so that the assertion above sees what the generator step alone leaves)
        for p in gnet.parameters():
            p.requires_grad_(True)
        rows.append([loss_g_pix.item(), loss_g_gan.item(), loss_d_real.item(), loss_d_fake.item(), real.detach().mean().item(),
                     fake.detach().mean().item()])
        for c in SN:
            arrays[f"s__u{3 * (it + 1)}__{c}"] = getattr(d, c).weight_u.numpy().copy()
        print(f"iteration {it}: {rows[-1]}")
    arrays["s__scalars"] = np.array(rows, dtype=np.float64)
    return arrays, cfg


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args(argv)
    arrays, state, D = build_disc()
    steps, cfg = build_steps(state, D)
    arrays.update(steps)
    meta = dict(num_feat=8, cases={n: list(s) for n, s in CASES}, g_cfg=cfg, g_weight_seed=0, lr=1e-3, pixel_weight=1.0, gan_weight=1.0,
                gan_loss_weight=0.1, torch=torch.__version__)
    os.makedirs(a.out, exist_ok=True)
    # the parameter gradients go to one sibling file per case: with those of one case disc.npz is 645 KB, and each fixture file stays
    # under 512 KB
    grads = {n: {k: arrays.pop(k) for k in list(arrays) if k.startswith(f"d__{n}__g__")} for n, _ in CASES}
    for fname, arrs in (("disc.npz", dict(meta=json.dumps(meta), **arrays)), ("disc_grads.npz", grads["A"]), ("disc_grads_B.npz", grads["B"])):
        path = os.path.join(a.out, fname)
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size < 512 * 1024, size
        print(f"wrote {path}: {len(arrs)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
