"""The reference's validation metrics: PSNR, SSIM and PSNR-B, on RGB and on the matlab Y channel (config/metric/*.yaml).

``image_metrics(restored, target, group)`` computes one metric group per image, keyed by the names the reference logs, after the
steps engines/base.py:256-271 takes first: ``tensor_round`` of both images and, for SR (``scale > 1``), a shave of ``scale`` pixels.

  group                 metrics                                                     reference tasks
  restorer              val_psnr, val_psnr_y, val_ssim, val_ssim_y                  SR, colour denoising, deblurring, demosaicking
  restorer_gray         val_psnr, val_ssim                                          grayscale denoising
  restorer_jpeg         restorer + val_psnrb, val_psnrb_y                           colour JPEG artifact removal
  restorer_jpeg_gray    val_psnr, val_ssim, val_psnrb                               grayscale JPEG artifact removal

CUDA tensors go through ``grl_image_metrics`` of libgrl_hip.so (csrc/metrics.hip: one tile pass, one per-image reduction); there
is no torch fallback for them.  CPU tensors take the plain-torch restatement below (the same definitions, evaluated in float64 on
the rounded 8-bit values, like the HIP kernel).  Metric definitions: utils/metrics/psnr.py:44-48, utils/metrics/ssim.py:17-85
(Gaussian window 11, sigma 1.5, zero padding 5, C1 = 0.01^2, C2 = 0.03^2), utils/metrics/psnrb.py:22-115 (``psnrb(target, preds)``:
the blocking effect factor of the prediction alone, with the reference's normalising counts for sides that are not multiples of 8).

The reference evaluates these in fp32.  Its SSIM then depends on how the convolution backend rounds: on smooth images the fp32
value moves by up to ~3e-5 from the exact one, through the E[x^2] - E[x]^2 cancellation.  Both paths here work in float64 (the
kernel's moments and sums, the restatement's convolutions) and are tested against the float64 run of the reference's functions
for SSIM, against its fp32 values for PSNR and PSNR-B.
"""
import ctypes as C
import math
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from .evaluate import rgb_to_y, shave, tensor_round

GROUPS = {
    "restorer": ("val_psnr", "val_psnr_y", "val_ssim", "val_ssim_y"),
    "restorer_gray": ("val_psnr", "val_ssim"),
    "restorer_jpeg": ("val_psnr", "val_psnr_y", "val_ssim", "val_ssim_y", "val_psnrb", "val_psnrb_y"),
    "restorer_jpeg_gray": ("val_psnr", "val_ssim", "val_psnrb"),
}
# GRL_METRIC_* bit of each metric; bit i is column i of grl_image_metrics' output
BITS = {"val_psnr": 1, "val_psnr_y": 2, "val_ssim": 4, "val_ssim_y": 8, "val_psnrb": 16, "val_psnrb_y": 32}
Y_COEF = (65.481, 128.553, 24.966)

_TAPS = None


def ssim_window() -> Tuple[torch.Tensor, torch.Tensor]:
    """(11x11 fp32 window, 1-D float64 taps).  The window is ssim.py's create_window: taps exp(-(x-5)^2 / 4.5) rounded to 6 decimals,
    normalised in float64, outer product cast to fp32.  The taps are that normalised vector scaled by sqrt(sum of the fp32
    window), so that the separable kernel has the fp32 window's total weight (it moves SSIM by ~1e-6 on smooth images)."""
    global _TAPS
    if _TAPS is None:
        g = torch.tensor([round(math.exp(-((x - 5) ** 2) / float(2 * 1.5 ** 2)), 6) for x in range(11)], dtype=torch.float64)
        g = g / g.sum()
        w2 = g.unsqueeze(1).mm(g.unsqueeze(0)).float()
        _TAPS = (w2, g * math.sqrt(w2.double().sum().item()))
    return _TAPS


def _check(restored: torch.Tensor, target: torch.Tensor, group: str, scale: int) -> Tuple[Tuple[str, ...], int]:
    if group not in GROUPS:
        raise ValueError(f"unknown metric group {group!r}: one of {sorted(GROUPS)}")
    if restored.dim() != 4 or restored.shape != target.shape:
        raise ValueError(f"restored {tuple(restored.shape)} and target {tuple(target.shape)}: need two equal (B, C, H, W) shapes")
    keys = GROUPS[group]
    Cc = restored.shape[1]
    if Cc not in (1, 3) or (Cc == 1 and any(k.endswith("_y") for k in keys)):
        raise ValueError(f"group {group!r} on {Cc}-channel images (the _y metrics need RGB; grey images use the *_gray groups)")
    border = scale if scale > 1 else 0
    if 2 * border >= min(restored.shape[-2:]):
        raise ValueError(f"shave by {border} leaves nothing of a {tuple(restored.shape[-2:])} image")
    if restored.device != target.device:
        raise ValueError(f"restored on {restored.device}, target on {target.device}")
    return keys, border


def image_metrics(restored: torch.Tensor, target: torch.Tensor, group: str = "restorer", scale: int = 1) -> Dict[str, torch.Tensor]:
    """Per-image metrics of ``group`` as the reference's validation step reports them: {name: float64 tensor of shape (B,)}.
    ``restored`` and ``target`` are (B, C, H, W) images in [0, 1] (values outside are clamped by the rounding), C = 3 or, for the
    *_gray groups, 1; ``scale > 1`` shaves ``scale`` pixels off every side first (SR).  PSNR is +inf for identical images;
    PSNR-B is finite there and -inf for sides below 16 (the reference's counts are 0)."""
    keys, border = _check(restored, target, group, scale)
    if restored.is_cuda:
        bits = 0
        for k in keys:
            bits |= BITS[k]
        out = hip_image_metrics(restored, target, border, bits)
        return {k: out[:, BITS[k].bit_length() - 1] for k in keys}
    return _torch_metrics(restored, target, keys, border)


def hip_image_metrics(restored: torch.Tensor, target: torch.Tensor, border: int, bits: int) -> torch.Tensor:
    """One ``grl_image_metrics`` call: (B, 6) float64, column i = metric bit (1 << i), NaN where not asked for.  The inputs are read
    in place (any strides); only the library checks the arguments."""
    from . import _lib

    L = _lib.lib()
    r = restored if restored.dtype == torch.float32 else restored.float()
    t = target if target.dtype == torch.float32 else target.float()
    B, _, H, W = r.shape
    ws_bytes = int(L.grl_image_metrics_workspace_bytes(B, H, W, border))
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=r.device)
    out = torch.empty(B, _lib.METRIC_COUNT, dtype=torch.float64, device=r.device)
    taps = ssim_window()[1]
    ycoef = torch.tensor(Y_COEF, dtype=torch.float32) / 255.0     # evaluate.rgb_to_y's fp32 coefficients
    args = _lib.GrlMetricArgs(
        restored=r.data_ptr(), restored_stride=(C.c_int64 * 4)(*r.stride()), shape=(C.c_int32 * 4)(*r.shape),
        target=t.data_ptr(), target_stride=(C.c_int64 * 4)(*t.stride()), target_shape=(C.c_int32 * 4)(*t.shape),
        border=border, metrics=bits, taps=(C.c_double * 11)(*taps.tolist()), y_coef=(C.c_float * 3)(*ycoef.tolist()),
        workspace=ws.data_ptr(), workspace_bytes=ws_bytes, out=out.data_ptr())
    _lib.check(L.grl_image_metrics(_lib.stream_ptr(), C.byref(args)), "grl_image_metrics")
    return out


# ---- CPU restatement -------------------------------------------------------------------------------------------------------
def _psnr(p: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    return -10.0 * (p - t).pow(2).mean(dim=(1, 2, 3)).log10()


def _ssim(p: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    Cc = p.shape[1]
    w = ssim_window()[0].to(p.device, torch.float64).expand(Cc, 1, 11, 11)
    conv = lambda x: F.conv2d(x, w, padding=5, groups=Cc)
    mu1, mu2 = conv(p), conv(t)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(p * p) - mu1_sq, conv(t * t) - mu2_sq, conv(p * t) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return m.mean(dim=(1, 2, 3))


def _bef(im: torch.Tensor) -> torch.Tensor:
    """psnrb.py:22-100 (blocking_effect_factor) of (B, 1, H, W)."""
    H, W = im.shape[-2:]
    dh = (im[..., :, :-1] - im[..., :, 1:]).pow(2)          # column j: pixel j against j + 1
    dv = (im[..., :-1, :] - im[..., 1:, :]).pow(2)
    bh = torch.arange(W - 1, device=im.device) % 8 == 7
    bv = torch.arange(H - 1, device=im.device) % 8 == 7
    s = lambda x: x.sum(dim=(1, 2, 3))
    n_bh, n_bv = H * (W // 8 - 1), W * (H // 8 - 1)
    bd = (s(dh[..., bh]) + s(dv[..., bv, :])) / (n_bh + n_bv)
    nbd = (s(dh[..., ~bh]) + s(dv[..., ~bv, :])) / ((H * (W - 1) - n_bh) + (W * (H - 1) - n_bv))
    scaler = 3.0 / math.log2(min(H, W)) if min(H, W) > 1 else math.inf
    bef = scaler * (bd - nbd)
    bef[bd <= nbd] = 0
    return bef


def _psnrb(p: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    total = 0
    for c in range(p.shape[1]):
        mse = (p[:, c] - t[:, c]).pow(2).flatten(1).mean(1)
        total = total + 10 * torch.log10(1 / (mse + _bef(p[:, c : c + 1])))
    return total / p.shape[1]


def _torch_metrics(restored, target, keys, border) -> Dict[str, torch.Tensor]:
    r = shave(tensor_round(restored.float()), border)
    t = shave(tensor_round(target.float()), border)
    planes = {"": (r.double(), t.double())}
    if any(k.endswith("_y") for k in keys):
        planes["_y"] = (rgb_to_y(r).double(), rgb_to_y(t).double())
    fn = {"val_psnr": _psnr, "val_ssim": _ssim, "val_psnrb": _psnrb}
    out = {}
    for k in keys:
        base, y = (k[:-2], "_y") if k.endswith("_y") else (k, "")
        out[k] = fn[base](*planes[y])
    return out
