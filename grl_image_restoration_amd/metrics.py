"""The reference's validation metrics: PSNR, SSIM and PSNR-B, on RGB and on the matlab Y channel (config/metric/*.yaml).

``image_metrics(restored, target, group)`` computes one metric group per image, keyed by the names the reference logs, after the
steps engines/base.py:256-271 takes first: ``tensor_round`` of both images and, for SR (``scale > 1``), a shave of ``scale`` pixels.

  group                 metrics                                                     reference tasks
  restorer              val_psnr, val_psnr_y, val_ssim, val_ssim_y                  SR, colour denoising, deblurring, demosaicking
  restorer_gray         val_psnr, val_ssim                                          grayscale denoising
  restorer_jpeg         restorer + val_psnrb, val_psnrb_y                           colour JPEG artifact removal
  restorer_jpeg_gray    val_psnr, val_ssim, val_psnrb                               grayscale JPEG artifact removal
  restorer_niqe         val_niqe (no reference: ``target`` is ignored, no shave)    blind / real-world SR (``niqe`` below)
  restorer_perceptual   restorer + val_lpips, val_niqe (RGB only; needs the LPIPS   real-world SR, GAN stage (``lpips`` below,
                        model and the NIQE model: PERCEPTUAL_GROUPS)                lpips.py)

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
import os
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from . import ops
from . import switches as SW
from .evaluate import rgb_to_y, shave, tensor_round

GROUPS = {
    "restorer": ("val_psnr", "val_psnr_y", "val_ssim", "val_ssim_y"),
    "restorer_gray": ("val_psnr", "val_ssim"),
    "restorer_jpeg": ("val_psnr", "val_psnr_y", "val_ssim", "val_ssim_y", "val_psnrb", "val_psnrb_y"),
    "restorer_jpeg_gray": ("val_psnr", "val_ssim", "val_psnrb"),
}
# groups that score the restored image alone (no ground truth): kept apart from GROUPS, whose every entry compares a pair
NO_REFERENCE_GROUPS = {"restorer_niqe": ("val_niqe",)}
ALL_GROUPS = {**GROUPS, **NO_REFERENCE_GROUPS}
# groups that need user-supplied models on top of a pair (an ``lpips.LPIPS`` and the NIQE pristine model): kept apart from ALL_GROUPS,
# whose every entry is computable from the images alone or with the NIQE model alone.  The command lines offer both tables
PERCEPTUAL_GROUPS = {"restorer_perceptual": ("val_psnr", "val_psnr_y", "val_ssim", "val_ssim_y", "val_lpips", "val_niqe")}
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


def image_metrics(restored: torch.Tensor, target: Optional[torch.Tensor], group: str = "restorer", scale: int = 1,
                  niqe_params=None, lpips_model=None) -> Dict[str, torch.Tensor]:
    """Per-image metrics of ``group`` as the reference's validation step reports them: {name: float64 tensor of shape (B,)}.
    ``restored`` and ``target`` are (B, C, H, W) images in [0, 1] (values outside are clamped by the rounding), C = 3 or, for the
    *_gray groups, 1; ``scale > 1`` shaves ``scale`` pixels off every side first (SR).  PSNR is +inf for identical images;
    PSNR-B is finite there and -inf for sides below 16 (the reference's counts are 0).  Group "restorer_niqe" scores ``restored``
    alone (``target`` may be None; no shave: the reference's border is 0) against the pristine model ``niqe_params`` (see ``niqe``).
    Group "restorer_perceptual" (RGB only): the four ``restorer`` values, then ``val_lpips`` from ``lpips_model`` (an ``lpips.LPIPS``)
    and ``val_niqe`` against ``niqe_params``, both on the rounded, shaved images every metric of the validation step is handed."""
    if group in NO_REFERENCE_GROUPS:
        return {"val_niqe": niqe(restored, niqe_params)}
    if group in PERCEPTUAL_GROUPS:
        if lpips_model is None:
            raise ValueError(f"metric group {group!r} needs the LPIPS model: pass lpips_model (lpips.load_lpips(vgg16 file, lin file); "
                             "--lpips-vgg / --lpips-lin)")
        if niqe_params is None and not SW.text(NIQE_ENV):
            raise ValueError(f"metric group {group!r} needs the NIQE pristine model: pass niqe_params (--niqe-params), or set the "
                             f"environment variable {NIQE_ENV}")
        if restored.dim() != 4 or restored.shape[1] != 3:
            raise ValueError(f"group {group!r} is for RGB images (B, 3, H, W), got {tuple(restored.shape)}")
        out = image_metrics(restored, target, "restorer", scale)
        out["val_lpips"] = lpips(restored, target, lpips_model, scale)
        out["val_niqe"] = niqe(shave(tensor_round(restored.float()), scale if scale > 1 else 0), niqe_params)
        return out
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
    ws = ops.empty(max(ws_bytes, 8), dtype=torch.uint8, device=r.device)
    out = ops.empty(B, _lib.METRIC_COUNT, dtype=torch.float64, device=r.device)
    taps = ssim_window()[1]
    ycoef = torch.tensor(Y_COEF, dtype=torch.float32) / 255.0     # evaluate.rgb_to_y's fp32 coefficients
    args = _lib.GrlMetricArgs(
        restored=r.data_ptr(), restored_stride=(C.c_int64 * 4)(*r.stride()), shape=(C.c_int32 * 4)(*r.shape),
        target=t.data_ptr(), target_stride=(C.c_int64 * 4)(*t.stride()), target_shape=(C.c_int32 * 4)(*t.shape),
        border=border, metrics=bits, taps=(C.c_double * 11)(*taps.tolist()), y_coef=(C.c_float * 3)(*ycoef.tolist()),
        workspace=ws.data_ptr(), workspace_bytes=ws_bytes, out=out.data_ptr())
    _lib.launch("grl_image_metrics", args)
    return out


def lpips(restored: torch.Tensor, target: torch.Tensor, lpips_model, scale: int = 1) -> torch.Tensor:
    """``val_lpips`` alone, as the reference's validation step reports it: ``lpips_model`` (an ``lpips.LPIPS``) on ``tensor_round`` of
    both images, shaved by ``scale`` pixels for SR: (B,) float64, lower is better."""
    border = scale if scale > 1 else 0
    if restored.dim() != 4 or restored.shape != target.shape or 2 * border >= min(restored.shape[-2:]):
        raise ValueError(f"restored {tuple(restored.shape)} and target {tuple(target.shape)}: need two equal (B, 3, H, W) shapes larger "
                         f"than the shave of {border}")
    return lpips_model(shave(tensor_round(restored.float()), border), shave(tensor_round(target.float()), border))


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


# ---- NIQE (utils/metrics/niqe.py) ------------------------------------------------------------------------------------------------
# The reference's only validation metric for blind SR (config/metric/restorer_niqe.yaml): no ground truth.  ``niqe`` scores the
# 8-bit rounded image against a pristine multivariate Gaussian model, which is user data like a checkpoint: the reference's
# utils/metrics/niqe_pris_params.npz, given as a path, as arrays, or through the environment variable GRL_NIQE_PARAMS.
#
# CUDA tensors take the features from ``grl_image_niqe_features`` (csrc/niqe.hip); there is no torch fallback for them.  CPU tensors
# take ``niqe_features_torch``, the same definitions in float64 torch.  Both evaluate in float64 what the reference evaluates in
# fp32; the 36 x 36 tail (nanmean, covariance, pinv, quadratic form; niqe.py:475-490) is float64 torch on the features' device.
NIQE_ENV = "GRL_NIQE_PARAMS"
NIQE_BLOCK = 96
NIQE_FEATURES = 36
_NIQE_SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
_NIQE_WINDOW = None
_NIQE_GRID = None
_NIQE_DEVICE = {}


def niqe_window() -> torch.Tensor:
    """(7, 7) float64: MATLAB's fspecial('gaussian', 7, 7/6), the ``gaussian_window`` of the reference's parameter file."""
    global _NIQE_WINDOW
    if _NIQE_WINDOW is None:
        sigma = 7.0 / 6.0
        x = torch.arange(-3, 4, dtype=torch.float64)
        h = torch.exp(-(x.view(7, 1) ** 2 + x.view(1, 7) ** 2) / (2 * sigma * sigma))
        h[h < torch.finfo(torch.float64).eps * h.max()] = 0
        _NIQE_WINDOW = h / h.sum()
    return _NIQE_WINDOW


def niqe_grid() -> torch.Tensor:
    """(5, 9801) float64: estimate_aggd_param's search grid ``gam = arange(0.2, 10.001, 0.001)``, its ``r_gam`` (niqe.py:352-356), and
    gamma(1 / gam), gamma(2 / gam), gamma(3 / gam) as niqe.py:368-369,395 evaluate them at the chosen alpha.  SciPy's gamma when it
    is installed (what the reference calls), math.gamma otherwise."""
    global _NIQE_GRID
    if _NIQE_GRID is None:
        import numpy as np

        try:
            from scipy.special import gamma
        except ImportError:
            gamma = np.vectorize(math.gamma, otypes=[np.float64])
        gam = np.arange(0.2, 10.001, 0.001)
        rec = np.reciprocal(gam)
        r_gam = np.square(gamma(rec * 2)) / (gamma(rec) * gamma(rec * 3))
        _NIQE_GRID = torch.from_numpy(np.stack([gam, r_gam, gamma(1 / gam), gamma(2 / gam), gamma(3 / gam)]).astype(np.float64))
    return _NIQE_GRID


def load_niqe_params(params=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mu (36,), cov (36, 36)) float64 CPU tensors of the pristine model.  ``params``: a path to the reference's
    niqe_pris_params.npz, a mapping with ``mu_pris_param`` and ``cov_pris_param``, a ``(mu, cov)`` pair, or None for the file that
    the environment variable GRL_NIQE_PARAMS names."""
    import numpy as np

    if params is None:
        params = SW.text(NIQE_ENV)
        if not params:
            raise ValueError(f"NIQE needs the pristine model (the reference's utils/metrics/niqe_pris_params.npz): pass its path as "
                             f"--niqe-params / niqe_params, or set the environment variable {NIQE_ENV}")
    if isinstance(params, (str, os.PathLike)):
        if not os.path.isfile(params):
            raise ValueError(f"NIQE parameter file {os.fspath(params)!r} not found (--niqe-params / niqe_params, or the environment "
                             f"variable {NIQE_ENV})")
        with np.load(params) as f:
            params = {k: f[k] for k in ("mu_pris_param", "cov_pris_param")}
    if hasattr(params, "keys"):
        params = (params["mu_pris_param"], params["cov_pris_param"])
    mu, cov = (torch.as_tensor(np.asarray(p.detach().cpu() if torch.is_tensor(p) else p), dtype=torch.float64) for p in params)
    mu = mu.reshape(-1)
    if mu.shape != (NIQE_FEATURES,) or cov.shape != (NIQE_FEATURES, NIQE_FEATURES):
        raise ValueError(f"NIQE parameters: mu {tuple(mu.shape)} and cov {tuple(cov.shape)}, need (36,) and (36, 36)")
    return mu, cov


def _check_niqe(x: torch.Tensor):
    if x.dim() != 4 or x.shape[1] not in (1, 3) or x.shape[0] < 1:
        raise ValueError(f"NIQE needs a (B, C, H, W) batch with C = 1 or 3, got {tuple(x.shape)}")
    if min(x.shape[-2:]) < NIQE_BLOCK:
        raise ValueError(f"NIQE works on 96 x 96 blocks: a {tuple(x.shape[-2:])} image has none")


def niqe(restored: torch.Tensor, params=None) -> torch.Tensor:
    """NIQE of every image of a (B, C, H, W) batch in [0, 1] as the reference's validation reports it (NaturalImageQualityEvaluator,
    niqe.py:549-583): (B,) float64, lower is better.  ``params``: the pristine model, see ``load_niqe_params``.  Raises ValueError
    for an image whose blocks are all flat (the reference fails there with "SVD did not converge")."""
    _check_niqe(restored)
    mu, cov = load_niqe_params(params)
    feat = niqe_features(restored)
    return _niqe_tail(feat, mu.to(feat.device), cov.to(feat.device))


def niqe_features(restored: torch.Tensor) -> torch.Tensor:
    """The reference's ``distparam`` of every image: (B, blocks, 36) float64, blocks with columns outer and rows inner."""
    _check_niqe(restored)
    if restored.is_cuda:
        return hip_niqe_features(restored)
    return niqe_features_torch(restored)


def _niqe_tail(feat: torch.Tensor, mu: torch.Tensor, cov: torch.Tensor) -> torch.Tensor:
    """niqe.py:475-490 per image."""
    out = []
    for b, f in enumerate(feat):
        rows = f[~torch.isnan(f).any(dim=1)]
        if rows.shape[0] < 2:
            raise ValueError(f"NIQE: image {b} has {rows.shape[0]} block(s) with defined features out of {f.shape[0]} (a flat image, "
                             "or a single textured block): its feature covariance does not exist")
        d = mu - torch.nanmean(f, dim=0)
        inv = torch.linalg.pinv((cov + torch.cov(rows.t())) / 2)
        out.append(torch.sqrt(d @ inv @ d))
    return torch.stack(out)


def _niqe_tables(Hc: int, Wc: int, device):
    """Device copies of the grid and of the half-scale resize tables (cached)."""
    from . import tasks

    key = (str(device),)
    if key not in _NIQE_DEVICE:
        _NIQE_DEVICE[key] = niqe_grid().to(device).contiguous()
    rows = tasks._device_tables((Hc, Hc // 2, 0.5, True), device)
    cols = tasks._device_tables((Wc, Wc // 2, 0.5, True), device)
    return _NIQE_DEVICE[key], rows, cols


def hip_niqe_features(restored: torch.Tensor) -> torch.Tensor:
    """One ``grl_image_niqe_features`` call (five launches): (B, blocks, 36) float64.  The image is read in place (any strides); the
    library checks the arguments."""
    from . import _lib

    L = _lib.lib()
    r = restored if restored.dtype == torch.float32 else restored.float()
    B, _, H, W = r.shape
    nbh, nbw = H // NIQE_BLOCK, W // NIQE_BLOCK
    grid, (wh, ih), (ww, iw) = _niqe_tables(nbh * NIQE_BLOCK, nbw * NIQE_BLOCK, r.device)
    ws_bytes = int(L.grl_image_niqe_workspace_bytes(B, H, W))
    ws = ops.empty(max(ws_bytes, 16), dtype=torch.uint8, device=r.device)
    out = ops.empty(B, nbh * nbw, NIQE_FEATURES, dtype=torch.float64, device=r.device)
    args = _lib.GrlNiqeArgs(
        img=r.data_ptr(), stride=(C.c_int64 * 4)(*r.stride()), shape=(C.c_int32 * 4)(*r.shape),
        window=(C.c_double * 49)(*niqe_window().flatten().tolist()), grid=grid.data_ptr(), ngrid=grid.shape[1],
        taps_h=wh.shape[1], taps_w=ww.shape[1], wh=wh.data_ptr(), ih=ih.data_ptr(), ww=ww.data_ptr(), iw=iw.data_ptr(),
        workspace=ws.data_ptr(), workspace_bytes=ws_bytes, out=out.data_ptr())
    _lib.launch("grl_image_niqe_features", args)
    return out


# ---- NIQE, torch restatement (any device; the CPU path) ---------------------------------------------------------------------------
def niqe_plane(restored: torch.Tensor) -> torch.Tensor:
    """(B, 1, H, W) fp32 integer levels: the plane calculate_niqe scores (niqe.py:493-546) for what the validation step hands it,
    ``tensor_round(output) * 255`` as a CHW **RGB** array.  For C = 3 the reference's to_y_channel assumes BGR (niqe.py:143-156,573),
    so the plane is 24.966 R + 128.553 G + 65.481 B + 16 -- red and blue swapped against rgb2ycbcr.  The published numbers were
    computed this way; it is reproduced rounding for rounding: the dot product in float64 on fp32 samples, / 255 cast to fp32,
    x 255 in fp32, round half to even."""
    k = (restored.float().clamp(0.0, 1.0) * 255.0).round()
    if k.shape[1] == 1:
        return k
    u = ((k / 255.0) * 255.0 / 255.0).double()                    # tensor_round, x 255, to_y_channel's / 255, all fp32
    y = (u[:, 0] * 24.966 + u[:, 1] * 128.553) + u[:, 2] * 65.481 + 16.0
    return ((y / 255.0).float() * 255.0).round().unsqueeze(1)


def _mscn(plane: torch.Tensor) -> torch.Tensor:
    """(img - mu) / (sigma + 1) of ``plane`` (B, 1, h, w) in float64, window 7 x 7 with edge replication (niqe.py:447-455).  The
    moments are taken of the differences to the centre sample, which changes nothing where the window has texture and gives the exact
    zero the reference's fp32 ``mu`` gives where it is flat (csrc/niqe.hip, "Flat windows")."""
    x = plane.double()
    h, w = x.shape[-2:]
    pad = F.pad(x, (3, 3, 3, 3), mode="replicate")
    win = niqe_window()
    s1, s2 = torch.zeros_like(x), torch.zeros_like(x)
    for a in range(7):
        for e in range(7):
            d = pad[..., a : a + h, e : e + w] - x
            s1 += float(win[a, e]) * d
            s2 += float(win[a, e]) * (d * d)
    sigma = torch.sqrt(torch.abs(s2 - s1 * s1))
    return -s1 / (sigma + 1.0)


def _aggd_features(blocks: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """compute_feature (niqe.py:341-397) of (N, bs, bs) MSCN blocks: (N, 18) float64."""
    q = [blocks] + [blocks * torch.roll(blocks, s, dims=(1, 2)) for s in _NIQE_SHIFTS]
    q = torch.stack(q, 1).flatten(2)                              # (N, 5, bs * bs)
    n = q.shape[-1]
    neg, pos, sq = q < 0, q > 0, q * q
    left = torch.sqrt((sq * neg).sum(-1) / neg.sum(-1))           # 0 / 0 = nan without negative samples, as the reference
    right = torch.sqrt((sq * pos).sum(-1) / pos.sum(-1))
    gammahat = left / right
    rhat = (q.abs().sum(-1) / n) ** 2 / (sq.sum(-1) / n)
    g2 = gammahat * gammahat
    rhatnorm = (rhat * (g2 * gammahat + 1) * (gammahat + 1)) / ((g2 + 1) * (g2 + 1))
    flat = rhatnorm.flatten()
    idx = torch.empty_like(flat, dtype=torch.long)
    for i in range(0, flat.numel(), 1024):                        # np.argmin((r_gam - rhatnorm) ** 2): the first minimum
        idx[i : i + 1024] = torch.argmin((grid[1].unsqueeze(0) - flat[i : i + 1024].unsqueeze(1)) ** 2, dim=1)
    idx = torch.where(torch.isnan(flat), torch.zeros_like(idx), idx).view_as(rhatnorm)   # all-nan distances: argmin answers 0
    alpha, ga1, ga2, ga3 = grid[0][idx], grid[2][idx], grid[3][idx], grid[4][idx]
    ratio = torch.sqrt(ga1 / ga3)
    bl, br = left * ratio, right * ratio
    mean = (br - bl) * (ga2 / ga1)
    cols = [alpha[:, 0], (bl[:, 0] + br[:, 0]) / 2]
    for k in range(1, 5):
        cols += [alpha[:, k], mean[:, k], bl[:, k], br[:, k]]
    return torch.stack(cols, 1)


def niqe_features_torch(restored: torch.Tensor) -> torch.Tensor:
    """niqe() up to ``distparam`` (niqe.py:400-473) in float64 torch, on the device of ``restored``: (B, blocks, 36)."""
    from . import tasks

    _check_niqe(restored)
    B, _, H, W = restored.shape
    nbh, nbw = H // NIQE_BLOCK, W // NIQE_BLOCK
    yk = niqe_plane(restored)[..., : nbh * NIQE_BLOCK, : nbw * NIQE_BLOCK].contiguous()
    grid = niqe_grid().to(restored.device)
    feats = []
    for plane, bs in ((yk, NIQE_BLOCK), (None, NIQE_BLOCK // 2)):
        if plane is None:       # niqe.py:469-471: imresize(img / 255, 0.5) * 255 = imresize(img, 0.5) up to a rounding; kept in float64
            Hc, Wc = yk.shape[-2:]
            plane = tasks._torch_resize(yk, tasks.resize_tables(Hc, Hc // 2, 0.5, True), tasks.resize_tables(Wc, Wc // 2, 0.5, True))
        m = _mscn(plane)
        blocks = m.view(B, nbh, bs, nbw, bs).permute(0, 3, 1, 2, 4).reshape(B * nbw * nbh, bs, bs)
        feats.append(_aggd_features(blocks, grid).view(B, nbw * nbh, NIQE_FEATURES // 2))
    return torch.cat(feats, dim=2)
