"""Writes tests/golden/metrics/metrics.npz: image pairs and what the reference's validation metrics report on them.

The values come from the UNMODIFIED reference modules utils/metrics/{psnr,ssim,psnrb}.py and utils/utils_image.py, imported from
the reference tree (GRL_REFERENCE_ROOT, as for oracle/refshim.py) with two stand-ins in ``sys.modules``: ``cv2`` (imported by
ssim.py, never called) and ``torchmetrics.Metric`` (the base class of the metric modules; only ``add_state`` is used by them).
Each pair goes through what engines/base.py:256-271 does before the metrics -- ``tensor_round`` of both images, ``shave`` by the
scale for SR -- and then through the metric classes' own ``update`` (the Y conversion, the per-image SSIM loop).

Stored per case ``<name>``:
  <name>__restored, <name>__target   fp32 (B, C, H, W) inputs (values outside [0, 1] included: tensor_round clamps)
  <name>__scale                      the SR scale: shave by it when > 1
  <name>__<metric>                   fp32 per-image values of the reference, (B,)
  <name>__<metric>__fp64             the same metric functions run in float64 on the same rounded / converted inputs

    python tools/make_golden_metrics.py [--reference DIR] [--out tests/golden/metrics/metrics.npz]
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.refshim import REFERENCE_ROOT  # noqa: E402  (where the reference tree is; nothing else is used)

OUT = os.path.join(ROOT, "tests", "golden", "metrics", "metrics.npz")

RGB_METRICS = ("val_psnr", "val_psnr_y", "val_ssim", "val_ssim_y", "val_psnrb", "val_psnrb_y")
GRAY_METRICS = ("val_psnr", "val_ssim", "val_psnrb")


def _noise_pair(g, B, C, H, W, spread=0.1):
    t = torch.rand(B, C, H, W, generator=g, dtype=torch.float64).float()
    r = t + spread * torch.randn(B, C, H, W, generator=g, dtype=torch.float64).float()
    return r, t


def _smooth_pair(g, B, C, H, W):
    """An image-like target (a few low-frequency waves) and a restoration of it with 8x8-block artefacts and noise."""
    y = torch.linspace(0, 1, H, dtype=torch.float64).view(H, 1)
    x = torch.linspace(0, 1, W, dtype=torch.float64).view(1, W)
    t = torch.zeros(B, C, H, W, dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            f = torch.rand(4, generator=g, dtype=torch.float64) * 6 + 1
            t[b, c] = 0.5 + 0.25 * torch.sin(f[0] * 3.1 * x + f[1] * 2.3 * y) + 0.2 * torch.cos(f[2] * 4.7 * x * y + f[3])
    blk = torch.randn(B, C, (H + 7) // 8, (W + 7) // 8, generator=g, dtype=torch.float64) * 0.02
    blk = blk.repeat_interleave(8, -2).repeat_interleave(8, -1)[..., :H, :W]
    r = t + blk + 0.02 * torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    q = lambda a: (a.clamp(0, 1) * 255).round().float() / 255      # stored as 8-bit images
    return q(r), q(t)


def make_cases():
    """{name: (restored, target, scale)} -- deterministic (seeded), independent of the reference."""
    cases = {}
    g = torch.Generator().manual_seed(20240)
    cases["rgb_b2_23x17"] = _noise_pair(g, 2, 3, 23, 17) + (1,)
    cases["gray_b2_37x53"] = _noise_pair(g, 2, 1, 37, 53) + (1,)
    cases["rgb_37x53_shave2"] = _noise_pair(g, 1, 3, 37, 53, 0.05) + (2,)
    cases["gray_40x44_shave4"] = _noise_pair(g, 2, 1, 40, 44, 0.05) + (4,)
    cases["rgb_12x12"] = _noise_pair(g, 1, 3, 12, 12) + (1,)
    cases["gray_12x12"] = _noise_pair(g, 1, 1, 12, 12) + (1,)
    t = torch.rand(1, 3, 23, 17, generator=g, dtype=torch.float64).float()
    cases["rgb_identical_23x17"] = (t.clone(), t, 1)
    t = torch.rand(2, 1, 23, 17, generator=g, dtype=torch.float64).float()
    cases["gray_identical_23x17"] = (t.clone(), t, 1)
    r = torch.full((1, 3, 24, 32), 0.5)
    cases["rgb_constant_24x32"] = (r, r + 0.03 * torch.randn(1, 3, 24, 32, generator=g, dtype=torch.float64).float(), 1)
    cases["rgb_smooth_b2_64x72_shave4"] = _smooth_pair(g, 2, 3, 64, 72) + (4,)
    cases["gray_smooth_130x97"] = _smooth_pair(g, 1, 1, 130, 97) + (1,)
    cases["rgb_smooth_300x517"] = _smooth_pair(g, 1, 3, 300, 517) + (1,)
    return cases


def _install_stubs():
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    if "torchmetrics" not in sys.modules:
        tm = types.ModuleType("torchmetrics")

        class Metric:
            def __init__(self, compute_on_step=None, **kwargs):
                pass

            def add_state(self, name, default, dist_reduce_fx=None):
                setattr(self, name, list(default))

        tm.Metric = Metric
        sys.modules["torchmetrics"] = tm


def _import_reference(root):
    if not os.path.isfile(os.path.join(root, "utils", "metrics", "psnrb.py")):
        raise RuntimeError(f"reference tree not found at {root}")
    _install_stubs()
    if root not in sys.path:
        sys.path.insert(0, root)
    from utils import utils_image
    from utils.metrics import psnr, psnrb, ssim

    return utils_image, psnr, ssim, psnrb


def reference_values(root, cases):
    U, P, S, PB = _import_reference(root)
    out = {}
    for name, (restored, target, scale) in cases.items():
        r, t = U.tensor_round(restored.clone(), 1.0), U.tensor_round(target.clone(), 1.0)
        if scale > 1:
            r, t = U.shave(r, scale), U.shave(t, scale)
        C = r.shape[1]
        mk = {"val_psnr": lambda: P.PeakSignalNoiseRatio(data_range=1.0),
              "val_psnr_y": lambda: P.PeakSignalNoiseRatio(data_range=1.0, channel="y"),
              "val_ssim": lambda: S.StructuralSimilarityIndexMeasure(data_range=1.0),
              "val_ssim_y": lambda: S.StructuralSimilarityIndexMeasure(data_range=1.0, channel="y"),
              "val_psnrb": lambda: PB.PeakSignalNoiseRatioBlock(data_range=1.0),
              "val_psnrb_y": lambda: PB.PeakSignalNoiseRatioBlock(data_range=1.0, channel="y")}
        for key in (RGB_METRICS if C == 3 else GRAY_METRICS):
            m = mk[key]()
            m.update(r.clone(), t.clone(), idx=list(range(r.shape[0])))
            out[f"{name}__{key}"] = m.value[0].numpy().astype(np.float32)
            # float64: the same functions on the same rounded (and, for _y, converted: an integer grid) planes
            r64, t64 = r, t
            if key.endswith("_y"):
                r64, t64 = U.rgb2ycbcr(r, 1.0), U.rgb2ycbcr(t, 1.0)
            r64, t64 = r64.double(), t64.double()
            if key.startswith("val_psnrb"):
                v = PB.psnrb(t64, r64)
            elif key.startswith("val_ssim"):
                v = torch.stack([S.ssim(a.unsqueeze(0), b.unsqueeze(0)) for a, b in zip(r64, t64)])
            else:
                v = P.psnr(r64, t64)
            out[f"{name}__{key}__fp64"] = v.numpy().astype(np.float64)
    return out


def build(root):
    cases = make_cases()
    arrays = {}
    for name, (restored, target, scale) in cases.items():
        arrays[f"{name}__restored"] = restored.numpy()
        arrays[f"{name}__target"] = target.numpy()
        arrays[f"{name}__scale"] = np.array(scale, dtype=np.int64)
    arrays.update(reference_values(root, cases))
    return arrays


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=REFERENCE_ROOT)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args(argv)
    arrays = build(a.reference)
    np.savez_compressed(a.out, **arrays)
    print(f"wrote {a.out}: {len(arrays)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
