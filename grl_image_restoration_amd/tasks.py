"""Front ends of the tasks whose degraded (LQ) input the reference builds from the ground truth (GT) itself.

  mosaic_bayer   utils/utils_mosaic.py:114-133      RGB -> packed RGGB mosaic (CFA4: planes R, G, G, B at half resolution),
                 (mosaic_CFA_Bayer)                 what data/datasets/restoration_dm.py:25-35 feeds the demosaicking model
  dm_matlab      utils/utils_mosaic.py:36-111       MATLAB's gradient-corrected linear demosaic of a CFA4 batch, applied by
                                                    engines/base.py:126-128 before ``self.model(x)`` (training and evaluation)
  demosaic_gt    both of the above                  the demosaicking LQ of a GT batch
  modcrop        data/datasets/base_image.py:419-425   the validation GT crop to a multiple of ``modulo`` (8)
  dn_noise_key   data/datasets/restoration_dn.py:133-143   the validation noise of the denoising task: numpy's MT19937 seeded
  dn_noise                                          with the SHA-256 of the image name, drawn as N(0, sigma / 255)
  resize_tables  utils/matlab_functions.py:20-88    weights and (reflected, zero-based) input indices of MATLAB's bicubic resize along
                 (calculate_weights_indices)        one axis, float64; the symmetric padding of lines 137-148 / 161-172 is in the indices
  imresize       utils/matlab_functions.py:91-188   MATLAB's antialiased bicubic ``imresize`` of a batch, rows then columns
  sr_lq          data/datasets/restoration_sr.py:130-141   the classical-SR LQ of a GT batch: modcrop to the scale, imresize by
                                                    1 / scale, 8-bit quantisation (``tensor_round``: what an LQ image file holds)
  gaussian_blur_kernel  utils/utils_deblur.py:54-65  MATLAB's ``fspecial('gaussian', 25, 1.6)``, float64
  load_blur_kernel   utils/utils_deblur.py:116-125  the blur kernel of non-blind deblurring: the Gaussian, or kernel n of a Levin09 file
                                                    that the user supplies (the package ships none)
  blur_taps          utils/utils_deblur.py:127      the correlation taps handed to ``conv2d``: the fp32 kernel flipped over both axes
  blur               engines/base.py:131-142        depthwise K x K correlation of an image batch with one tap table, zero padded
                                                    ("same", validation) or the valid region ("valid", the training branch's crop),
                                                    plus the noise; ``want_center`` also returns the cropped target
  db_noise           data/datasets/restoration_db.py:40-43   the deblurring validation noise: numpy's generator seeded 0 for EVERY image
  db_lq                                             the deblurring LQ of a GT batch: ``blur(gt, taps, "same", add=noise)``
  jpeg_tables        libjpeg's jpeg_set_quality           the two baseline quantisation tables of a quality, natural (row-major) order
  jpeg_roundtrip     data/datasets/restoration_jpeg.py:62-79   the JPEG artifact-removal LQ: ``cv2.imencode(".jpg", img, [IMWRITE_JPEG_QUALITY,
                                                    q])`` followed by ``cv2.imdecode``, restated as libjpeg's integer arithmetic (the
                                                    entropy coding is lossless and left out)
  usm_taps           cv2.getGaussianKernel(K, 0)         the 1-D Gaussian of ``usm_sharp``: K = 51, sigma = 8 at the reference's radius 50
  usm_sharp          utils/utils_bsr/utils_usm.py:34-60  unsharp-mask sharpening of a GT batch (``cv2.GaussianBlur`` twice, reflect-101
                                                    borders): the target of the real-world-SR PSNR stage, restoration_sr.py:105-109
                                                    (validation, ``use_usm``) and restoration_bsr.py:56-59 (training, ``use_usm_pixel``)
  VAL_LQ, TRAIN_STORE_LQ, TRAIN_PAIR                the LQ of each task from the front ends above, per side: a validation image, a
                                                    training store made once, a training batch (at the end of the module; what a
                                                    task accepts is ``task_rules.RULES``)

CUDA fp32 tensors go through ``grl_demosaic_matlab`` of libgrl_hip.so (csrc/demosaic.hip); there is no torch fallback for them.
``demosaic_gt`` on CUDA is a single launch that reads the RGB image in place on the RGGB lattice, without forming the mosaic.  CPU
tensors take the float64 torch restatement below, cast back to the input dtype.  On 8-bit inputs both paths are exact (the filter
weights are dyadic) and therefore bitwise equal to each other and to the reference run in float64.  The noise is CPU numpy by
design: only the reference's own generator stream reproduces its denoising PSNRs.  ``imresize`` follows the same rule: CUDA fp32
tensors go through ``grl_imresize`` (csrc/imresize.hip, one launch, fp64 sums, one rounding), CPU tensors through a float64 gather
and sum by the same tables; the two agree to an fp32 rounding, not bitwise (cubic weights are not dyadic).  ``blur`` on CUDA is one
``grl_blur_depthwise`` launch (csrc/blur.hip: an fp32 fmaf chain per output in a fixed order, deterministic); on the CPU the taps are
summed in float64 and rounded once.  The two agree within the forward error of a K x K-term fp32 sum, (K^2 + 2) 2^-24 max|x|.
``jpeg_roundtrip`` on CUDA is one ``grl_jpeg_roundtrip`` call (csrc/jpeg.hip, two launches, int32); on the CPU ``_torch_jpeg``
restates the same integer arithmetic in int64.  Both are libjpeg-turbo's defaults (4:2:0, ``JDCT_ISLOW``, baseline tables, fancy
upsampling) bit for bit, so the two paths and the library agree in every byte.  ``usm_sharp`` on CUDA is one ``grl_usm_sharp`` call
(csrc/usm.hip, two launches, fp32 fmaf chains in a fixed order); on the CPU the two blurs and the mask are float64.  The two agree
within the forward error of two 51-term fp32 chains wherever the masks agree; bit equality with OpenCV's summation order is not
claimed.
"""
import ctypes as C
import hashlib
import math
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F


def _ops():
    """ops.empty / ops.empty_like: every output and workspace of a launch is poisonable (GRL_POISON); imported late, as _lib is."""
    from . import ops

    return ops


# ---- demosaicking --------------------------------------------------------------------------------------------------------------
def mosaic_bayer(rgb: torch.Tensor) -> torch.Tensor:
    """(N, 3, H, W) RGB -> (N, 4, H/2, W/2) packed RGGB mosaic: R at (even, even), G at (even, odd), G at (odd, even), B at
    (odd, odd).  H and W must be even (the reference's slicing fails on odd sides as well)."""
    _check_rgb(rgb)
    return torch.stack(_lattice(rgb), 1)


def _check_rgb(rgb: torch.Tensor):
    if rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError(f"need an (N, 3, H, W) RGB batch, got {tuple(rgb.shape)}")
    if rgb.shape[-2] % 2 or rgb.shape[-1] % 2:
        raise ValueError(f"the RGGB mosaic needs even sides, got {tuple(rgb.shape[-2:])}")


def _lattice(rgb: torch.Tensor):
    """The four RGGB planes of an RGB batch as strided views (no copy)."""
    return rgb[:, 0, 0::2, 0::2], rgb[:, 1, 0::2, 1::2], rgb[:, 1, 1::2, 0::2], rgb[:, 2, 1::2, 1::2]


def _check_packed(N: int, h: int, w: int):
    if h < 2 or w < 2:
        raise ValueError(f"dm_matlab needs a packed mosaic of at least 2 x 2 cells, got {h} x {w}")
    if N < 1:
        raise ValueError("empty batch")


def dm_matlab(cfa4: torch.Tensor) -> torch.Tensor:
    """(N, 4, h, w) packed RGGB mosaic -> (N, 3, 2h, 2w) RGB, as the reference's ``dm_matlab``: reflect padding by 2 of the
    full-resolution mosaic, MATLAB's four gradient-corrected 5x5 filters, native samples kept."""
    if cfa4.dim() != 4 or cfa4.shape[1] != 4:
        raise ValueError(f"need an (N, 4, h, w) packed mosaic, got {tuple(cfa4.shape)}")
    N, _, h, w = cfa4.shape
    _check_packed(N, h, w)
    if cfa4.is_cuda:
        return hip_demosaic([cfa4[:, i] for i in range(4)])
    return _torch_dm_matlab(cfa4)


def demosaic_gt(rgb: torch.Tensor) -> torch.Tensor:
    """``dm_matlab(mosaic_bayer(rgb))``: the demosaicking task's model input for a GT batch.  On CUDA one launch reads ``rgb`` on
    the RGGB lattice in place."""
    _check_rgb(rgb)
    N, _, H, W = rgb.shape
    _check_packed(N, H // 2, W // 2)
    if rgb.is_cuda:
        return hip_demosaic(list(_lattice(rgb)))
    return dm_matlab(mosaic_bayer(rgb))


def hip_demosaic(planes) -> torch.Tensor:
    """One ``grl_demosaic_matlab`` launch on four (N, h, w) fp32 CUDA views with equal strides (R, G, G, B); the sizes are checked
    by the library."""
    from . import _lib

    p0 = planes[0]
    if any(p.dtype != torch.float32 for p in planes):
        raise TypeError(f"grl_demosaic_matlab takes fp32 tensors, got {p0.dtype}")
    if any(p.shape != p0.shape or p.stride() != p0.stride() or p.device != p0.device for p in planes):
        raise ValueError("the four mosaic planes need one shape, one stride triple and one device")
    N, h, w = p0.shape
    out = _ops().empty(N, 3, 2 * h, 2 * w, dtype=torch.float32, device=p0.device)
    args = _lib.GrlDemosaicArgs(plane=(C.c_void_p * 4)(*[p.data_ptr() for p in planes]), stride=(C.c_int64 * 3)(*p0.stride()),
                                N=N, h=h, w=w, out=out.data_ptr())
    _lib.launch("grl_demosaic_matlab", args)
    return out


_KERNELS = None


def matlab_kernels() -> torch.Tensor:
    """(4, 1, 5, 5) float64: the four 5x5 filters of utils_mosaic.py:44-86 (all scaled by 1/8) as correlation kernels, indexed
    [dy + 2][dx + 2]: 0 G at R / B sites, 1 R / B at G sites along the row, 2 its transpose (along the column), 3 R at B / B at
    R sites."""
    global _KERNELS
    if _KERNELS is None:
        k = torch.zeros(4, 5, 5, dtype=torch.float64)
        cross1 = [(1, 2), (3, 2), (2, 1), (2, 3)]          # the four neighbours at distance 1
        cross2 = [(0, 2), (4, 2), (2, 0), (2, 4)]          # ... and at distance 2
        diag = [(1, 1), (1, 3), (3, 1), (3, 3)]
        k[0, 2, 2] = 4
        for i, j in cross1:
            k[0, i, j] = 2
        for i, j in cross2:
            k[0, i, j] = -1
        k[1, 2, 2] = 5
        k[1, 2, 1] = k[1, 2, 3] = 4
        k[1, 2, 0] = k[1, 2, 4] = -1
        k[1, 0, 2] = k[1, 4, 2] = 0.5
        for i, j in diag:
            k[1, i, j] = -1
        k[2] = k[1].t()
        k[3, 2, 2] = 6
        for i, j in diag:
            k[3, i, j] = 2
        for i, j in cross2:
            k[3, i, j] = -1.5
        _KERNELS = (k / 8).unsqueeze(1)
    return _KERNELS


def _torch_dm_matlab(cfa4: torch.Tensor) -> torch.Tensor:
    N, _, h, w = cfa4.shape
    x = cfa4.double()
    mosaic = torch.empty(N, 1, 2 * h, 2 * w, dtype=torch.float64, device=x.device)
    for i, (r, c) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        mosaic[:, 0, r::2, c::2] = x[:, i]
    conv = F.conv2d(F.pad(mosaic, (2, 2, 2, 2), mode="reflect"), matlab_kernels().to(x.device))
    rgb = mosaic.repeat(1, 3, 1, 1)
    # (channel, cell row, cell column) <- filter; the remaining entry of each site is its native sample
    fill = [(1, 0, 0, 0), (1, 1, 1, 0),                     # G at R and B sites
            (0, 0, 1, 1), (0, 1, 0, 2), (0, 1, 1, 3),       # R at the G sites and at B
            (2, 0, 1, 2), (2, 1, 0, 1), (2, 0, 0, 3)]       # B at the G sites and at R
    for ch, r, c, k in fill:
        rgb[:, ch, r::2, c::2] = conv[:, k, r::2, c::2]
    return rgb.to(cfa4.dtype)


# ---- validation crop and denoising noise ---------------------------------------------------------------------------------------
def modcrop(img: torch.Tensor, modulo: int = 8) -> torch.Tensor:
    """Top-left crop of the last two dimensions to multiples of ``modulo`` (a view)."""
    H, W = img.shape[-2:]
    return img[..., : H // modulo * modulo, : W // modulo * modulo]


# the reference's test-set names (restoration_dn.py:69-84): they start the noise seed key, case included
DN_TEST_SETS = ("Set12", "BSD68", "CBSD68", "Kodak24", "McMaster", "Urban100")


def dn_test_set_name(folder: str) -> str:
    """The reference's name of a denoising test set from a folder name, matched case-insensitively ("kodak24" -> "Kodak24"); other
    names are returned as they are."""
    return {n.lower(): n for n in DN_TEST_SETS}.get(folder.lower(), folder)


def dn_noise_key(name: str) -> str:
    """The string the reference seeds an image's validation noise with: its name up to the first underscore (the reference's names
    are ``"<TestSet>/<path in test.json>"``)."""
    return name.split("_")[0]


def dn_noise(shape, sigma: float, key: str) -> torch.Tensor:
    """The reference's validation noise for one (C, H, W) image, bit for bit: numpy's RandomState seeded with the SHA-256 digest of
    ``key`` read as eight uint32 words, ``normal(0, sigma / 255, shape)`` in float64, cast to fp32 (CPU)."""
    seed = np.frombuffer(hashlib.sha256(key.encode("utf-8")).digest(), dtype="uint32")
    noise = np.random.RandomState(seed).normal(0, sigma / 255, tuple(shape))
    return torch.from_numpy(noise).float()


# ---- MATLAB bicubic imresize and the classical-SR LQ ---------------------------------------------------------------------------
def _cubic(x: torch.Tensor) -> torch.Tensor:
    """matlab_functions.py:10-17, same operation order."""
    absx = torch.abs(x)
    absx2 = absx**2
    absx3 = absx**3
    return (1.5 * absx3 - 2.5 * absx2 + 1) * ((absx <= 1).type_as(absx)) + (-0.5 * absx3 + 2.5 * absx2 - 4 * absx + 2) * (
        ((absx > 1) * (absx <= 2)).type_as(absx))


_TABLES = {}
_DEVICE_TABLES = {}


def resize_tables(in_len: int, out_len: int, scale: float, antialiasing: bool = True, axis: str = "axis"):
    """(weights float64 (out_len, taps), indices int64 (out_len, taps)) of MATLAB's bicubic resize along one axis:
    ``out[o] = sum_t weights[o, t] * in[indices[o, t]]``.  The reference's calculate_weights_indices in float64, operation for
    operation; of its ``ceil(kernel_width) + 2`` tap columns the first and the last carry no weight (their distance to the centre
    is at least half the kernel width) and are dropped as the reference drops them.  The indices are zero-based and already
    reflected the way ``imresize`` pads symmetrically (-1 -> 0, -2 -> 1, n -> n-1, n+1 -> n-2).  An axis shorter than that padding
    raises ValueError (the reference fails in a ``copy_`` there).  ``axis`` only names the axis in that message.  Cached."""
    key = (int(in_len), int(out_len), float(scale), bool(antialiasing))
    if key in _TABLES:
        return _TABLES[key]
    if in_len < 1 or out_len < 1 or not scale > 0:
        raise ValueError(f"resize_tables: need positive lengths and scale, got {in_len}, {out_len}, {scale}")
    f64 = torch.float64
    kernel_width = 4.0
    shrink = scale < 1 and antialiasing
    if shrink:
        kernel_width = kernel_width / scale
    x = torch.linspace(1, out_len, out_len, dtype=f64)
    u = x / scale + 0.5 * (1 - 1 / scale)
    left = torch.floor(u - kernel_width / 2)
    p = math.ceil(kernel_width) + 2
    indices = left.view(out_len, 1).expand(out_len, p) + torch.linspace(0, p - 1, p, dtype=f64).view(1, p).expand(out_len, p)
    distance = u.view(out_len, 1).expand(out_len, p) - indices
    weights = scale * _cubic(distance * scale) if shrink else _cubic(distance)
    weights = weights / torch.sum(weights, 1).view(out_len, 1).expand(out_len, p)
    if float(weights[:, 0].abs().max()) > 1e-15 or float(weights[:, -1].abs().max()) > 1e-15:
        raise AssertionError("resize_tables: an outer tap column carries weight")
    weights = weights[:, 1 : p - 1].contiguous()
    idx = indices[:, 1 : p - 1].long() - 1                         # zero-based, before the reflection
    need = max(int(-idx.min()), int(idx.max()) - (in_len - 1), 0)
    if need > in_len:
        raise ValueError(f"imresize: {axis} has {in_len} pixels, but its symmetric padding at scale {scale:g} takes {need}: "
                         f"the minimum length is {need}")
    idx = torch.where(idx < 0, -idx - 1, idx)
    idx = torch.where(idx >= in_len, 2 * in_len - 1 - idx, idx).contiguous()
    _TABLES[key] = (weights, idx)
    return _TABLES[key]


def _device_tables(key, device):
    k = key + (str(device),)
    if k not in _DEVICE_TABLES:
        w, i = resize_tables(*key)
        _DEVICE_TABLES[k] = (w.to(device), i.to(torch.int32).to(device))
    return _DEVICE_TABLES[k]


def _round8(img: torch.Tensor) -> torch.Tensor:
    """The reference's ``tensor_round`` (utils/utils_image.py:30-33), out of place."""
    return (img.clamp(0.0, 1.0) * 255.0).round() / 255.0


def imresize(img: torch.Tensor, scale: float, antialiasing: bool = True, quantize: bool = False) -> torch.Tensor:
    """MATLAB's bicubic ``imresize`` of an (N, C, H, W) or (C, H, W) image by ``scale`` (both axes): output
    ``ceil(H * scale) x ceil(W * scale)``, rows first, then columns, as the reference.  ``quantize`` applies ``tensor_round``
    (8-bit levels) to the result.  CUDA tensors must be fp32 and take one ``grl_imresize`` launch, in place on any strided view;
    CPU tensors are gathered and summed in float64 and cast back to their dtype."""
    squeeze = img.dim() == 3
    if squeeze:
        img = img.unsqueeze(0)
    if img.dim() != 4:
        raise ValueError(f"need an (N, C, H, W) or (C, H, W) image, got {tuple(img.shape)}")
    N, Cn, H, W = img.shape
    if N < 1 or Cn < 1:
        raise ValueError("empty batch")
    out_h, out_w = math.ceil(H * scale), math.ceil(W * scale)
    kh, kw = (H, out_h, float(scale), bool(antialiasing)), (W, out_w, float(scale), bool(antialiasing))
    resize_tables(*kh, axis="the height")
    resize_tables(*kw, axis="the width")
    if img.is_cuda:
        out = hip_resize(img, _device_tables(kh, img.device), _device_tables(kw, img.device), quantize)
    else:
        out = _torch_resize(img, resize_tables(*kh), resize_tables(*kw)).to(img.dtype)
        if quantize:
            out = _round8(out)
    return out[0] if squeeze else out


def _torch_resize(img: torch.Tensor, rows, cols) -> torch.Tensor:
    """Float64 restatement: gather by the index table, multiply, sum; rows then columns.  Works on any device."""
    (wh, ih), (ww, iw) = rows, cols
    x = img.double()
    N, Cn, H, W = x.shape
    wh, ih, ww, iw = wh.to(x.device), ih.to(x.device).long(), ww.to(x.device), iw.to(x.device).long()
    x = (x[:, :, ih.reshape(-1), :].view(N, Cn, ih.shape[0], ih.shape[1], W) * wh.view(1, 1, *wh.shape, 1)).sum(3)
    return (x[..., iw.reshape(-1)].view(N, Cn, ih.shape[0], iw.shape[0], iw.shape[1]) * ww).sum(-1)


def hip_resize(img: torch.Tensor, rows, cols, quantize: bool = False) -> torch.Tensor:
    """One ``grl_imresize`` launch: ``img`` an (N, C, H, W) fp32 CUDA tensor or view, ``rows`` / ``cols`` (float64 weights, int32
    indices) on the same device, (out_len, taps) each.  The sizes are checked by the library."""
    from . import _lib

    if img.dtype != torch.float32:
        raise TypeError(f"grl_imresize takes fp32 tensors, got {img.dtype}")
    (wh, ih), (ww, iw) = rows, cols
    for w, i in (rows, cols):
        if w.dtype != torch.float64 or i.dtype != torch.int32 or w.shape != i.shape or w.dim() != 2 or w.device != img.device:
            raise ValueError("resize tables: float64 weights and int32 indices of one (out_len, taps) shape on the image's device")
    wh, ih, ww, iw = wh.contiguous(), ih.contiguous(), ww.contiguous(), iw.contiguous()
    N, Cn, H, W = img.shape
    out = _ops().empty(N, Cn, wh.shape[0], ww.shape[0], dtype=torch.float32, device=img.device)
    args = _lib.GrlResizeArgs(src=img.data_ptr(), stride=(C.c_int64 * 4)(*img.stride()), N=N, C=Cn, H=H, W=W,
                              out_h=wh.shape[0], out_w=ww.shape[0], taps_h=wh.shape[1], taps_w=ww.shape[1],
                              wh=wh.data_ptr(), ih=ih.data_ptr(), ww=ww.data_ptr(), iw=iw.data_ptr(), out=out.data_ptr(),
                              quantize=int(bool(quantize)))
    _lib.launch("grl_imresize", args)
    return out


def sr_lq(gt: torch.Tensor, scale: int, quantize: bool = True):
    """The classical-SR LQ of a GT batch as the reference builds it: ``modcrop(gt, scale)``, then ``imresize`` by ``1 / scale``,
    8-bit quantised by default.  Returns ``(lq, gt_cropped)``; ``gt_cropped`` is a view of ``gt``."""
    scale = int(scale)
    if scale < 1:
        raise ValueError(f"sr_lq: scale must be a positive integer, got {scale}")
    gtc = modcrop(gt, scale)
    lq = imresize(gtc, 1 / scale, True, quantize)
    if lq.shape[-2] * scale != gtc.shape[-2] or lq.shape[-1] * scale != gtc.shape[-1]:
        raise RuntimeError(f"sr_lq: LQ {tuple(lq.shape[-2:])} x {scale} != GT {tuple(gtc.shape[-2:])}")
    return lq, gtc


# ---- non-blind deblurring ------------------------------------------------------------------------------------------------------
def gaussian_blur_kernel(size: int = 25, sigma: float = 1.6) -> torch.Tensor:
    """MATLAB's ``fspecial('gaussian', size, sigma)`` as the reference runs it (utils_deblur.py:54-65), operation for operation in
    float64: ``exp(-(x^2 + y^2) / (2 sigma^2))``, entries below ``eps * max`` zeroed (``eps`` is ``np.finfo(float).eps``: the
    reference's ``scipy.finfo`` was an alias of it), divided by the sum.  (size, size) float64."""
    siz = (size - 1.0) / 2.0
    x, y = np.meshgrid(np.arange(-siz, siz + 1), np.arange(-siz, siz + 1))
    h = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    h[h < np.finfo(float).eps * h.max()] = 0
    sumh = h.sum()
    if sumh != 0:
        h = h / sumh
    return torch.from_numpy(h)


def _check_blur_kernel(k: np.ndarray, what: str) -> np.ndarray:
    k = np.asarray(k)
    if k.dtype == object or k.ndim != 2 or k.shape[0] != k.shape[1] or k.shape[0] % 2 == 0 or not 1 <= k.shape[0] <= 31:
        raise ValueError(f"{what}: a blur kernel is a square 2-D array with an odd side of 1 .. 31, got {k.dtype} {k.shape}")
    return k.astype(np.float64)


def load_blur_kernel(kernel_type: str = "gaussian", path=None) -> torch.Tensor:
    """The (K, K) float64 blur kernel of ``config/data_module/db.yaml``'s ``kernel_type``, before the flip of ``blur_taps``:
    "gaussian" is ``gaussian_blur_kernel()``; "real1" .. "real8" read kernel n from ``path``, a file the user supplies: the
    reference's ``utils/blur_kernels/Levin09.npy`` (an object array (1, 8); only this layout is opened with ``allow_pickle``) or a
    plain 2-D ``.npy`` holding that one kernel."""
    if kernel_type == "gaussian":
        return gaussian_blur_kernel()
    if not (isinstance(kernel_type, str) and len(kernel_type) == 5 and kernel_type.startswith("real") and kernel_type[4] in "12345678"):
        raise ValueError(f"unknown blur kernel {kernel_type!r}: gaussian or real1 .. real8")
    if path is None:
        raise ValueError(f"blur kernel {kernel_type} is read from a file (the reference's Levin09.npy, or a 2-D .npy); none was given")
    try:
        k = np.load(path, allow_pickle=False)
    except ValueError:                                   # an object array: the reference's Levin09 layout
        k = np.load(path, allow_pickle=True)
        if k.dtype != object or k.shape != (1, 8):
            raise ValueError(f"{path}: an object array of shape {k.shape}, not the (1, 8) Levin09 layout")
        k = k[0, int(kernel_type[4]) - 1]
    return torch.from_numpy(_check_blur_kernel(k, str(path)))


def blur_taps(kernel) -> torch.Tensor:
    """The (K, K) fp32 correlation taps the reference hands to ``conv2d`` (utils_deblur.py:127): the kernel cast to fp32 and flipped
    over BOTH axes (``np.flip`` without an axis)."""
    k = _check_blur_kernel(kernel.detach().cpu().numpy() if torch.is_tensor(kernel) else kernel, "blur_taps")
    return torch.from_numpy(np.flip(k.astype(np.float32)).copy())


def blur(x: torch.Tensor, taps: torch.Tensor, pad: str = "same", add: Optional[torch.Tensor] = None, want_center: bool = False):
    """Depthwise correlation of an (N, C, H, W) fp32 batch with ONE (K, K) fp32 tap table for all channels, K odd and at most 31:
    ``out = fl32(sum taps[ky][kx] * x[oy - p + ky][ox - p + kx]) + add``.  ``pad`` "same": p = K // 2, zeros outside, output H x W
    (the reference's validation path); "valid": p = 0, output (H - K + 1) x (W - K + 1) (its training path: blur, then crop by
    K // 2).  ``add``: an fp32 tensor that broadcasts to the output (the noise).  ``want_center`` ("valid" only): returns
    ``(out, x[..., K//2 : K//2 + Ho, K//2 : K//2 + Wo])``, the cropped target, contiguous.  CUDA tensors take one
    ``grl_blur_depthwise`` launch, in place on any strided view; CPU tensors sum in float64 and round once to fp32."""
    if pad not in ("same", "valid"):
        raise ValueError(f"blur: pad is 'same' or 'valid', got {pad!r}")
    if x.dim() != 4 or x.shape[0] < 1 or x.shape[1] < 1 or x.shape[2] < 1 or x.shape[3] < 1:
        raise ValueError(f"blur: need a non-empty (N, C, H, W) batch, got {tuple(x.shape)}")
    if x.dtype != torch.float32 or taps.dtype != torch.float32:
        raise TypeError(f"blur takes fp32 images and taps, got {x.dtype} and {taps.dtype}")
    if taps.dim() != 2 or taps.shape[0] != taps.shape[1] or taps.shape[0] % 2 == 0 or taps.shape[0] > 31:
        raise ValueError(f"blur: the taps are a square table with an odd side of at most 31, got {tuple(taps.shape)}")
    K = taps.shape[0]
    N, Cn, H, W = x.shape
    if pad == "valid" and (H < K or W < K):
        raise ValueError(f"blur: a {H} x {W} image has no valid region under a {K} x {K} kernel")
    if want_center and pad != "valid":
        raise ValueError("blur: the centre crop belongs to pad='valid'")
    Ho, Wo = (H, W) if pad == "same" else (H - K + 1, W - K + 1)
    if add is not None:
        if add.dtype != torch.float32 or add.device != x.device:
            raise TypeError("blur: add is an fp32 tensor on the image's device")
        add = add.expand(N, Cn, Ho, Wo)
    if x.is_cuda:
        return hip_blur(x, taps.to(x.device), K // 2 if pad == "same" else 0, add, want_center)
    p = K // 2 if pad == "same" else 0
    w = taps.double().view(1, 1, K, K).expand(Cn, 1, K, K)
    out = F.conv2d(x.double(), w, padding=p, groups=Cn).float()
    if add is not None:
        out = out + add
    if want_center:
        return out, x[..., K // 2 : K // 2 + Ho, K // 2 : K // 2 + Wo].contiguous()
    return out


def hip_blur(x: torch.Tensor, taps: torch.Tensor, pad: int, add: Optional[torch.Tensor] = None, want_center: bool = False):
    """One ``grl_blur_depthwise`` launch: ``x`` an (N, C, H, W) fp32 CUDA tensor or view, ``taps`` (K, K) fp32 on its device, ``pad``
    K // 2 or 0, ``add`` a view of the output's shape (any batch / channel / row strides; a column stride other than 1 is copied).
    K, the padding and the sizes are checked by the library."""
    from . import _lib

    if x.dtype != torch.float32 or taps.dtype != torch.float32 or (add is not None and add.dtype != torch.float32):
        raise TypeError(f"grl_blur_depthwise takes fp32 tensors, got {x.dtype}")
    if taps.dim() != 2 or taps.shape[0] != taps.shape[1] or taps.device != x.device:
        raise ValueError("blur taps: a square (K, K) table on the image's device")
    taps = taps.contiguous()
    K = taps.shape[0]
    N, Cn, H, W = x.shape
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    shape = (N, Cn, max(Ho, 0), max(Wo, 0))
    out = _ops().empty(shape, dtype=torch.float32, device=x.device)
    center = _ops().empty(shape, dtype=torch.float32, device=x.device) if want_center else None
    add_ptr, add_stride = None, (0, 0, 0)
    if add is not None:
        if tuple(add.shape) != shape or add.device != x.device:
            raise ValueError(f"blur add: shape {tuple(add.shape)}, the output is {shape}")
        if add.stride(3) != 1 and Wo > 1:
            add = add.contiguous()
        add_ptr, add_stride = add.data_ptr(), add.stride()[:3]
    args = _lib.GrlBlurArgs(x=x.data_ptr(), stride=(C.c_int64 * 4)(*x.stride()), N=N, C=Cn, H=H, W=W, taps=taps.data_ptr(), K=K,
                            pad=pad, add=add_ptr, add_stride=(C.c_int64 * 3)(*add_stride), out=out.data_ptr(),
                            center=center.data_ptr() if want_center else None)
    _lib.launch("grl_blur_depthwise", args)
    return (out, center) if want_center else out


def db_noise(shape, sigma: float) -> torch.Tensor:
    """The reference's deblurring validation noise for one (C, H, W) image, bit for bit (restoration_db.py:40-43):
    ``np.random.seed(0)`` before EVERY image -- unlike denoising, the same stream for all of them --
    ``normal(0, sigma / 255, shape)`` in float64, cast to fp32 (CPU)."""
    noise = np.random.RandomState(0).normal(0, sigma / 255.0, tuple(shape))
    return torch.from_numpy(noise.astype(np.float32))


def db_lq(gt: torch.Tensor, taps: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The deblurring LQ of a GT batch as the engine builds it for validation (engines/base.py:131-139): the noise plus the GT
    blurred with zero padding.  ``noise`` broadcasts to the batch and lives on the GT's device."""
    return blur(gt, taps, "same", add=noise)


# ---- JPEG compression artifacts ------------------------------------------------------------------------------------------------
# JPEG Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
_JPEG_STD = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
     100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99)
    + (99,) * 32,
)


def jpeg_tables(q: int) -> torch.Tensor:
    """(2, 64) int64: the luminance and the chrominance quantisation table of quality ``q`` (clamped to 1 .. 100) in natural
    (row-major) order, as libjpeg's ``jpeg_set_quality(q, force_baseline=TRUE)`` scales the Annex K tables."""
    q = min(max(int(q), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return ((torch.tensor(_JPEG_STD, dtype=torch.int64) * s + 50) // 100).clamp(1, 255)


def _jpeg_qualities(quality, N: int) -> torch.Tensor:
    """``quality`` (an int, or a sequence or integer tensor of length N) as an int32 (N,) tensor, unclamped, on its own device."""
    if torch.is_tensor(quality):
        if quality.dtype not in (torch.int32, torch.int64) or quality.dim() > 1:
            raise TypeError("jpeg_roundtrip: a quality tensor is int32 with one entry per sample")
        quality = quality.to(torch.int32).reshape(-1)
    elif isinstance(quality, (int, np.integer)):
        quality = torch.full((N,), int(quality), dtype=torch.int32)
    else:
        quality = torch.tensor([int(v) for v in quality], dtype=torch.int32)
    if quality.shape[0] != N:
        raise ValueError(f"jpeg_roundtrip: {quality.shape[0]} qualities for a batch of {N}")
    return quality


def jpeg_roundtrip(x: torch.Tensor, quality) -> torch.Tensor:
    """JPEG compression and decompression of an (N, C, H, W) fp32 batch of 8-bit levels ``k / 255``, C = 3 (RGB) or 1, as
    libjpeg-turbo does it with OpenCV's and Pillow's defaults: 4:2:0 chroma, the ``islow`` integer DCT, baseline tables, fancy
    upsampling.  ``quality``: an int, or a sequence or int32 tensor with one entry per sample; values outside 1 .. 100 are
    clamped.  Returns fp32 ``k' / 255``.  CUDA tensors take ``grl_jpeg_roundtrip`` (a quality tensor on the device is read by the
    kernel when it runs, so a captured call follows later changes of it); CPU tensors take ``_torch_jpeg``."""
    if x.dim() != 4 or x.shape[1] not in (1, 3) or min(x.shape) < 1:
        raise ValueError(f"jpeg_roundtrip: need a non-empty (N, C, H, W) batch with C = 1 or 3, got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TypeError(f"jpeg_roundtrip takes fp32 images, got {x.dtype}")
    q = _jpeg_qualities(quality, x.shape[0])
    if x.is_cuda:
        return hip_jpeg(x, q.to(x.device))
    return _torch_jpeg(x, q.cpu())


def hip_jpeg(x: torch.Tensor, quality: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One ``grl_jpeg_roundtrip`` call: ``x`` an (N, C, H, W) fp32 CUDA tensor, ``quality`` an int32 (N,) tensor on its device.  The
    workspace of the decoded component planes is a fresh uint8 tensor.  The sizes are checked by the library."""
    from . import _lib

    L = _lib.lib()
    if x.dtype != torch.float32 or quality.dtype != torch.int32:
        raise TypeError(f"grl_jpeg_roundtrip takes fp32 images and int32 qualities, got {x.dtype} and {quality.dtype}")
    if quality.device != x.device or quality.dim() != 1 or quality.shape[0] != x.shape[0]:
        raise ValueError("jpeg qualities: an int32 (N,) tensor on the image's device")
    x, quality = x.contiguous(), quality.contiguous()
    N, Cn, H, W = x.shape
    if out is None:
        out = _ops().empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out: a contiguous fp32 tensor of the input's shape on its device")
    ws = _ops().empty(max(int(L.grl_jpeg_workspace_bytes(N, Cn, H, W)), 1), dtype=torch.uint8, device=x.device)
    args = _lib.GrlJpegArgs(x=x.data_ptr(), quality=quality.data_ptr(), N=N, C=Cn, H=H, W=W, workspace=ws.data_ptr(),
                            out=out.data_ptr())
    _lib.launch("grl_jpeg_roundtrip", args)
    return out


def _jd(x, n: int):
    """libjpeg's DESCALE: a rounding arithmetic right shift."""
    return (x + (1 << (n - 1))) >> n


def _jpeg_fdct8(x: torch.Tensor, dim: int, first: bool) -> torch.Tensor:
    """One 1-D pass of jfdctint.c along ``dim`` (length 8): the row pass (``first``) or the column pass."""
    d = x.unbind(dim)
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0], o[4] = ((t10 + t11) << 2, (t10 - t11) << 2) if first else (_jd(t10 + t11, 2), _jd(t10 - t11, 2))
    z1 = (t12 + t13) * 4433
    o[2], o[6] = _jd(z1 + t13 * 6270, n), _jd(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _jd(t4 + z1 + z3, n), _jd(t5 + z2 + z4, n), _jd(t6 + z2 + z3, n), _jd(t7 + z1 + z4, n)
    return torch.stack(o, dim)


def _jpeg_idct8(x: torch.Tensor, dim: int, first: bool) -> torch.Tensor:
    """One 1-D pass of jidctint.c along ``dim``: the column pass (``first``, descale 11) or the row pass (descale 18)."""
    d = x.unbind(dim)
    z1 = (d[2] + d[6]) * 4433
    t2, t3 = z1 - d[6] * 15137, z1 + d[2] * 6270
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = 11 if first else 18
    return torch.stack([_jd(t10 + t3, n), _jd(t11 + t2, n), _jd(t12 + t1, n), _jd(t13 + t0, n),
                        _jd(t13 - t0, n), _jd(t12 - t1, n), _jd(t11 - t2, n), _jd(t10 - t3, n)], dim)


def _jpeg_plane(p: torch.Tensor, Q: torch.Tensor) -> torch.Tensor:
    """An (N, 8a, 8b) int64 component plane through forward DCT, quantisation with the (N, 64) table ``Q``, dequantisation and
    inverse DCT, block by block; returns the decoded samples 0 .. 255."""
    N, Hp, Wp = p.shape
    b = p.view(N, Hp // 8, 8, Wp // 8, 8).permute(0, 1, 3, 2, 4) - 128          # (N, block row, block column, row, column)
    c = _jpeg_fdct8(_jpeg_fdct8(b, 4, True), 3, False)
    Q = Q.view(N, 1, 1, 8, 8)
    v = Q * 8
    m = c.abs() + (v >> 1)
    k = torch.where(m >= v, torch.div(m, v, rounding_mode="floor"), torch.zeros_like(m)) * c.sign()
    s = _jpeg_idct8(_jpeg_idct8(k * Q, 3, True), 4, False)
    return (s + 128).clamp(0, 255).permute(0, 1, 3, 2, 4).reshape(N, Hp, Wp)


def _edge_pad(p: torch.Tensor, Hp: int, Wp: int) -> torch.Tensor:
    """(N, H, W) -> (N, Hp, Wp) by replicating the last row and column."""
    N, H, W = p.shape
    r = torch.arange(Hp).clamp(max=H - 1)
    c = torch.arange(Wp).clamp(max=W - 1)
    return p[:, r][:, :, c]


def _torch_jpeg(x: torch.Tensor, quality: torch.Tensor) -> torch.Tensor:
    """The round trip in plain torch int64, vectorised over the batch and the blocks (CPU)."""
    N, Cn, H, W = x.shape
    k = (x * 255.0).round().clamp(0, 255).to(torch.int64)
    Q = torch.stack([jpeg_tables(int(q)) for q in quality.tolist()])                   # (N, 2, 64)
    Hp, Wp = -(-H // 8) * 8, -(-W // 8) * 8
    if Cn == 1:
        return (_jpeg_plane(_edge_pad(k[:, 0], Hp, Wp), Q[:, 0])[:, None, :H, :W].to(torch.float32) / 255).contiguous()
    R, G, B = k[:, 0], k[:, 1], k[:, 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    Y = _jpeg_plane(_edge_pad(Y, Hp, Wp), Q[:, 0])[:, :H, :W]
    h2, w2 = -(-H // 2), -(-W // 2)
    Hc, Wc = -(-h2 // 8) * 8, -(-w2 // 8) * 8
    bias = torch.tensor([1, 2]).repeat(Wc // 2)
    planes = []
    for p in (Cb, Cr):
        f = _edge_pad(p, 2 * h2, 2 * Wc)                                               # full resolution: columns to 2 Wc, rows to 2 h2
        d = (f[:, 0::2, 0::2] + f[:, 0::2, 1::2] + f[:, 1::2, 0::2] + f[:, 1::2, 1::2] + bias) >> 2
        d = _jpeg_plane(_edge_pad(d, Hc, Wc), Q[:, 1])[:, :h2, :w2]                    # ... then the rows of the small plane to Hc
        planes.append(_jpeg_upsample(d)[:, :H, :W])
    cb, cr = planes[0] - 128, planes[1] - 128
    rgb = torch.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                       Y + ((116130 * cb + 32768) >> 16)], 1).clamp(0, 255)
    return (rgb.to(torch.float32) / 255).contiguous()


def _jpeg_upsample(d: torch.Tensor) -> torch.Tensor:
    """libjpeg's h2v2 fancy ("triangle") upsampling of an (N, h2, w2) plane to (N, 2 h2, 2 w2).  A plane of at most two columns
    (an image of at most four) is replicated 2 x 2 instead: libjpeg picks its plain upsampler there (jdsample.c, jinit_upsampler:
    ``do_fancy && compptr->downsampled_width > 2``)."""
    N, h2, w2 = d.shape
    if w2 <= 2:
        return d.repeat_interleave(2, 1).repeat_interleave(2, 2)
    y = torch.arange(2 * h2)
    r = y // 2
    rn = torch.where(y % 2 == 0, r - 1, r + 1).clamp(0, h2 - 1)
    s = 3 * d[:, r] + d[:, rn]                                                         # (N, 2 h2, w2)
    c = torch.arange(w2)
    even = (3 * s + s[:, :, (c - 1).clamp(min=0)] + 8) >> 4
    odd = (3 * s + s[:, :, (c + 1).clamp(max=w2 - 1)] + 7) >> 4
    return torch.stack([even, odd], 3).reshape(N, 2 * h2, 2 * w2)


# ---- USM-sharpened targets ----------------------------------------------------------------------------------------------------
# cv2.getGaussianKernel(n, sigma <= 0) returns these fixed tables for n <= 7 (imgproc/src/smooth.dispatch.cpp, small_gaussian_tab)
_SMALL_GAUSSIAN = {1: (1.0,), 3: (0.25, 0.5, 0.25), 5: (0.0625, 0.25, 0.375, 0.25, 0.0625),
                   7: (0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125)}
_USM_TAPS = {}


def usm_taps(radius: int = 50) -> torch.Tensor:
    """The (K,) fp32 taps of ``usm_sharp``'s blur: ``cv2.getGaussianKernel(K, 0)`` restated, K = ``radius``, plus one when it is
    even (utils_usm.py:50-51: 50 -> 51).  ``sigma = 0.3 ((K - 1) / 2 - 1) + 0.8`` (8.0 at K = 51), ``exp(-(i - (K - 1) / 2)^2 /
    (2 sigma^2))`` normalised by its sum in float64, then cast to fp32, as ``cv2.GaussianBlur`` builds its fp32 filter; K <= 7 are
    OpenCV's fixed tables.  K is at most 63, what ``grl_usm_sharp`` takes."""
    K = int(radius) + (1 if int(radius) % 2 == 0 else 0)
    if not 1 <= K <= 63:
        raise ValueError(f"usm_taps: the kernel size is 1 .. 63, got {K} (radius {radius})")
    if K in _SMALL_GAUSSIAN:
        return torch.tensor(_SMALL_GAUSSIAN[K], dtype=torch.float32)
    sigma = 0.3 * ((K - 1) * 0.5 - 1) + 0.8
    i = np.arange(K, dtype=np.float64) - (K - 1) * 0.5
    k = np.exp(-(i * i) / (2 * sigma * sigma))
    return torch.from_numpy((k / k.sum()).astype(np.float32))


def usm_device_taps(radius: int, device) -> torch.Tensor:
    """``usm_taps(radius)`` on ``device``, made once per radius and device.  The first call copies the table from the host, which a
    stream capture does not allow: it raises there instead of breaking the capture; call it (or ``usm_sharp``) once before."""
    key = (int(radius), str(torch.device(device)))
    if key not in _USM_TAPS:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"usm_sharp: the taps of radius {radius} are not on {device} yet and cannot be copied there during a "
                               "stream capture; call tasks.usm_device_taps(radius, device) or usm_sharp once before capturing")
        _USM_TAPS[key] = usm_taps(radius).to(device)
    return _USM_TAPS[key]


def usm_sharp(x: torch.Tensor, weight: float = 0.5, radius: int = 50, threshold: float = 10.0, quantise: bool = False,
              parts: bool = False):
    """The reference's ``usm_sharp`` (utils_usm.py:34-60) on an (N, C, H, W) fp32 batch in [0, 1], C = 1 or 3, every plane on its own:

        blur = G(x);  res = x - blur;  m = |res| * 255 > threshold;  soft = G(m)
        out  = soft * clamp(x + weight * res, 0, 1) + (1 - soft) * x

    G is the separable ``usm_taps(radius)`` blur with reflect-101 borders (``cv2.GaussianBlur``'s default), reflected as often as a
    side shorter than K / 2 needs.  ``quantise``: the result as 8-bit levels / 255 (``single2uint`` then ``to_tensor``,
    restoration_sr.py:108-115), bitwise ``image8.pack8`` of the plain result divided by 255.  ``parts``: returns
    ``(out, blur, m)``.  CUDA tensors take one ``grl_usm_sharp`` call (two launches, fp32 fmaf chains; there is no fallback); CPU
    tensors take the torch restatement: blur, mask and blend in float64, the result rounded once to fp32.  The call can be captured
    once the taps are on the device (``usm_device_taps``: any earlier call with this radius, or that function itself)."""
    if x.dim() != 4 or x.shape[1] not in (1, 3) or min(x.shape) < 1:
        raise ValueError(f"usm_sharp: need a non-empty (N, C, H, W) batch with C = 1 or 3, got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TypeError(f"usm_sharp takes fp32 images, got {x.dtype}")
    if x.is_cuda:
        return hip_usm(x, usm_device_taps(radius, x.device), weight, threshold, quantise, parts)
    return _torch_usm(x, usm_taps(radius), weight, threshold, quantise, parts)


def hip_usm(x: torch.Tensor, taps: torch.Tensor, weight: float = 0.5, threshold: float = 10.0, quantise: bool = False,
            parts: bool = False, out: Optional[torch.Tensor] = None):
    """One ``grl_usm_sharp`` call: ``x`` an (N, C, H, W) fp32 CUDA tensor, ``taps`` (K,) fp32 on its device (read by the kernels when
    they run).  The workspace is a fresh tensor; ``parts`` returns its two halves, blur and the 0 / 1 mask, next to the result.  K and
    the sizes are checked by the library."""
    from . import _lib

    L = _lib.lib()
    if x.dtype != torch.float32 or taps.dtype != torch.float32:
        raise TypeError(f"grl_usm_sharp takes fp32 tensors, got {x.dtype} and {taps.dtype}")
    if taps.dim() != 1 or taps.device != x.device:
        raise ValueError("usm taps: a (K,) table on the image's device")
    x, taps = x.contiguous(), taps.contiguous()
    N, Cn, H, W = x.shape
    if out is None:
        out = _ops().empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out: a contiguous fp32 tensor of the input's shape on its device")
    ws = _ops().empty((2,) + tuple(x.shape), dtype=torch.float32, device=x.device)
    if int(L.grl_usm_workspace_bytes(N, Cn, H, W)) != ws.numel() * 4:
        raise ValueError(f"grl_usm_sharp does not take a batch of shape {tuple(x.shape)}")
    args = _lib.GrlUsmArgs(x=x.data_ptr(), taps=taps.data_ptr(), N=N, C=Cn, H=H, W=W, K=taps.shape[0], quantise=int(bool(quantise)),
                           weight=float(weight), threshold=float(threshold), workspace=ws.data_ptr(), out=out.data_ptr())
    _lib.launch("grl_usm_sharp", args)
    return (out, ws[0], ws[1]) if parts else out


def _reflect101(n: int, half: int) -> torch.Tensor:
    """Source index of positions -half .. n - 1 + half under cv2's BORDER_REFLECT_101, reflected repeatedly."""
    if n == 1:
        return torch.zeros(1 + 2 * half, dtype=torch.int64)
    p = 2 * (n - 1)
    j = torch.arange(-half, n + half, dtype=torch.int64) % p
    return torch.where(j >= n, p - j, j)


def _usm_blur64(a: torch.Tensor, taps: torch.Tensor) -> torch.Tensor:
    """The separable blur of a float64 (N, C, H, W) batch with float64 taps, rows then columns."""
    N, Cn, H, W = a.shape
    K = taps.shape[0]
    a = a.reshape(N * Cn, 1, H, W)
    a = F.conv2d(a[..., _reflect101(W, K // 2)], taps.view(1, 1, 1, K))
    a = F.conv2d(a[..., _reflect101(H, K // 2), :], taps.view(1, 1, K, 1))
    return a.reshape(N, Cn, H, W)


def _torch_usm(x, taps, weight, threshold, quantise, parts):
    x64, t64 = x.double(), taps.double()
    blur = _usm_blur64(x64, t64)
    res = x64 - blur
    mask = (res.abs() * 255.0 > float(threshold)).double()
    soft = _usm_blur64(mask, t64)
    sharp = (x64 + float(weight) * res).clamp(0.0, 1.0)
    out = (soft * sharp + (1.0 - soft) * x64).float()
    if quantise:
        out = _round8(out)
    return (out, blur, mask) if parts else out


# ---- the LQ of each task: validation images, training stores, training batches ----------------------------------------------------
# Validation (``evaluate.task_inputs``): (gt (1, C, H, W) on the CPU, already cropped by the rule; file name; the options resolved by
# ``task_rules.resolve`` plus ``taps`` and ``noise_prefix``; device) -> lq.
def _dn_val_lq(gt, name, o, device):
    """The reference's seeded validation noise, keyed by ``<test set>/<file name>``; on the CPU, in fp32, as the data set does."""
    return gt + dn_noise(gt.shape[1:], o.sigma, dn_noise_key(f"{o.noise_prefix}/{name}")).unsqueeze(0)


def _db_val_lq(gt, name, o, device):
    """Blurred on ``device`` with zero padding; the noise (seeded 0 for every image) is made on the CPU and added by the blur kernel."""
    return db_lq(gt.to(device), o.taps, db_noise(gt.shape[1:], o.sigma).unsqueeze(0).to(device))


VAL_LQ = {
    "dn": _dn_val_lq,
    "dm": lambda gt, name, o, device: demosaic_gt(gt.to(device)),
    "sr_bicubic": lambda gt, name, o, device: sr_lq(gt.to(device), int(o.scale))[0],
    "db": _db_val_lq,
    "jpeg": lambda gt, name, o, device: jpeg_roundtrip(gt.to(device), o.quality),
}

# Training, once per image at construction (``data.PatchSampler``): (gt (1, C, H, W) fp32 on the store's device, cropped by the rule;
# the sampler's resolved options) -> lq of 8-bit levels, kept as an 8-bit LQ store and then sampled like a paired folder.
#   sr_bicubic  the QUANTISED LQ -- what an offline LR folder holds and what validation scores -- not the float LQ that
#               restoration_sr.py:130-141 resizes per item without rounding
#   jpeg        at a fixed quality (the reference's default, ``patchwise: False``) every image is compressed WHOLE: patches sit at
#               arbitrary phases of the 8 x 8 block grid, and small images are zero padded after compression
TRAIN_STORE_LQ = {
    "sr_bicubic": lambda gt, o: sr_lq(gt, o.scale)[0],
    "jpeg": lambda gt, o: jpeg_roundtrip(gt, o.quality),
}


# Training, per batch: (the sampler ``s``; gt (B, C, draw_patch, draw_patch); the per-sample draws or None; ``noise`` of ``next``)
# -> (lq, gt).
def _dn_pair(s, gt, sigmas, noise):
    """``lq = gt + sigma / 255 * randn`` from the sampler's seeded generator; sigma fixed, or one per sample from the sigma range
    (restoration_dn.py:126-143, the training branch)."""
    if s.sigma_range is not None:
        if sigmas is None or len(sigmas) != gt.shape[0]:
            raise ValueError("dn with a sigma range: one sigma per sample of an explicit work list")
        level = torch.tensor(list(sigmas), dtype=torch.float32).view(-1, 1, 1, 1).to(s.device) / 255
    else:
        level = s.sigma / 255
    noise = torch.randn(gt.shape, generator=s.gen, device=s.device, dtype=torch.float32)
    return gt + noise * level, gt


def _db_pair(s, gt, sigmas, noise):
    """``gt`` comes at the reference's enlarged patch P' = patch + K - 1 (restoration_db.py:19-21), so the zero padding of small
    images follows P' as well; ONE ``blur`` launch over the valid region gives ``lq`` at ``patch`` with the noise added by the
    kernel, and the target as the centre crop (engines/base.py:131-142).  The noise is ``sigma / 255 * randn`` at patch x patch from
    the sampler's generator, or ``noise`` scaled the same way.  The reference draws its training noise from the unseeded
    ``np.random`` at P' x P' and crops it, so there is no stream to reproduce bit for bit; the distribution is the same."""
    shape = (gt.shape[0], 3, s.patch, s.patch)
    if noise is None:
        noise = torch.randn(shape, generator=s.gen, device=s.device, dtype=torch.float32)
    elif tuple(noise.shape) != shape or noise.dtype != torch.float32:
        raise ValueError(f"db noise: an fp32 tensor of shape {shape}")
    return blur(gt, s.taps, "valid", add=noise.to(s.device) * (s.sigma / 255), want_center=True)


def _jpeg_pair(s, gt, sigmas, noise):
    """With a quality range (``patchwise: True``, restoration_jpeg.py:30-46) the patch is cropped and augmented first and ONE
    ``jpeg_roundtrip`` call compresses the batch at a quality per sample; the qualities sit in the sampler's own device tensor, so
    a captured step replays the call while they change."""
    if sigmas is None or len(sigmas) != gt.shape[0]:
        raise ValueError("jpeg with a quality range: one quality per sample of an explicit work list")
    q = s.in_place(s.qualities, torch.tensor([int(v) for v in sigmas], dtype=torch.int32))
    return jpeg_roundtrip(gt, q), gt


TRAIN_PAIR = {"dn": _dn_pair, "dm": lambda s, gt, sigmas, noise: (demosaic_gt(gt), gt), "db": _db_pair, "jpeg": _jpeg_pair}
