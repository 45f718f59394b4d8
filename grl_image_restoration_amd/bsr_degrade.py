"""Blind-SR training pairs made on the device: the reference's ``degradation_sr2`` (utils/utils_bsr/utils_sisr.py:293-464), the
BSRGAN-style random degradation that ``BSRDataset`` runs per sample on a 400 x 400 GT crop (data/datasets/restoration_bsr.py:83-110).

  cv_resize, blur_items          the two image operations on LISTS of (C, h, w) images whose sizes differ.  CUDA tensors take one
                                 ``grl_cv_resize`` / ``grl_blur_items`` launch for the whole list (csrc/cvresize.hip,
                                 csrc/blur_items.hip; there is no fallback); CPU tensors take the float64 torch restatements
                                 below, which are the yardstick of the kernels
  fspecial_gaussian, anisotropic_gaussian, shift_kernel
                                 the blur kernels, on the host in float64 (utils_sisr.py:169-180, 39-74, 77-103)
  draw_plan                      every scalar draw of ``degradation_sr2`` for one sample, from one ``random.Random``
  apply_plans                    a batch (N, C, crop, crop) through its plans -> (N, C, crop / scale, crop / scale) on the k / 255 grid
  add_noise                      the three noise stages as torch expressions with a ``torch.Generator``

``cv_resize`` is OpenCV's sampling rule (INTER_LINEAR, INTER_CUBIC, INTER_AREA; include/grl_hip.h states it) with float64
coordinates.  OpenCV rounds the coordinate to fp32 first, which moves a weight by up to n * 2^-24; equality with OpenCV's bytes is
not claimed (OpenCV is not a dependency).

Stage 2 of the reference, the ISP camera-noise model (utils_sisr.py:365-370), is opt-in: it needs the camera profiles, which are the
user's data (``isp.CameraBank.load``).  With ``camera=None`` the stage is a no-op and its draw is not made: every draw stream, plan
and output is then what it was before the stage existed.  With a bank, ``draw_plan`` makes the stage's draws and ``apply_plans``
runs it through ``isp`` (csrc/isp.hip on CUDA).  The ``ColorJitter`` of restoration_bsr.py:66-68,100 acts on the GT crop before
this module sees it: ``jitter.py``, ``PatchSampler(jitter=True)``, ``train --jitter``.  The frozen-set command line below has none,
as the reference's validation has none.
Scales 2 and 4 only (``int(1 / sf * n)`` is then exact), three channels (the correlated noise has a 3 x 3 covariance), ``crop`` a
multiple of 4 and at least ``4 * scale``.

    python -m grl_image_restoration_amd.bsr_degrade --gt DIR --out DIR --scale 4 --seed S [--crop 400] [--camera-profiles DIR]

writes a frozen validation set: every image centre-cropped and degraded once, ``<out>/LQ/<stem>.png`` and ``<out>/GT/<stem>.png``
(the reference's ``with_gt: True`` validation, restoration_bsr.py:113-114; with ``--camera-profiles`` the GT written is the one
the camera stage's HR pass returns, as there).  ``train --val-lq / --val-gt`` and ``evaluate`` read the two folders as they are.
"""
import argparse
import functools
import math
import os
import random
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import item_lists, ops

INTER_LINEAR, INTER_CUBIC, INTER_AREA = 1, 2, 3
STAGES = tuple(range(9))
KMAX = 31


# ---- cv2.resize -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=256)
def _axis_matrix(n: int, no: int, mode: str) -> torch.Tensor:
    """(no, n) float64: row d holds the weights of output d on one axis; taps outside the image are added at the clamped index."""
    W = np.zeros((no, n), dtype=np.float64)
    scale = n / no
    rows = np.arange(no)
    d = rows.astype(np.float64)
    if mode == "area_table":
        for j in range(no):
            f1 = j * scale
            f2 = f1 + scale
            cell = min(scale, n - f1)
            s1, s2 = math.ceil(f1), min(math.floor(f2), n - 1)
            s1 = min(s1, s2)
            if s1 - f1 > 1e-3:
                W[j, s1 - 1] += (s1 - f1) / cell
            for s in range(s1, s2):
                W[j, s] += 1.0 / cell
            if f2 - s2 > 1e-3:
                W[j, s2] += min(min(f2 - s2, 1.0), cell) / cell
        return torch.from_numpy(W)
    if mode == "area_linear":
        i = np.floor(d * scale)
        t = (d + 1) - (i + 1) / scale
        t = np.where(t <= 0, 0.0, t - np.floor(t))
    else:
        f = (d + 0.5) * scale - 0.5
        i = np.floor(f)
        t = f - i
    i = i.astype(np.int64)
    if mode == "cubic":
        A = -0.75
        c0 = ((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A
        c1 = ((A + 2) * t - (A + 3)) * t * t + 1
        u = 1 - t
        c2 = ((A + 2) * u - (A + 3)) * u * u + 1
        for k, c in enumerate((c0, c1, c2, 1.0 - c0 - c1 - c2)):
            np.add.at(W, (rows, np.clip(i - 1 + k, 0, n - 1)), c)
    else:
        lo, hi = i < 0, i >= n - 1
        t = np.where(lo | hi, 0.0, t)
        i = np.where(lo, 0, np.where(hi, n - 1, i))
        np.add.at(W, (rows, i), 1.0 - t)
        np.add.at(W, (rows, np.clip(i + 1, 0, n - 1)), t)
    return torch.from_numpy(W)


def _resize_mode(interp: int, h: int, w: int, ho: int, wo: int) -> str:
    if interp == INTER_LINEAR:
        return "linear"
    if interp == INTER_CUBIC:
        return "cubic"
    if interp == INTER_AREA:
        return "area_table" if h >= ho and w >= wo else "area_linear"
    raise ValueError(f"cv_resize: interp is 1 (linear), 2 (cubic) or 3 (area), got {interp}")


def resize_taps(interp: int, h: int, w: int, ho: int, wo: int):
    """(n_y, n_x): the largest number of taps one output of ``(h, w) -> (ho, wo)`` reads on each axis -- what the error bound of
    the kernel counts."""
    mode = _resize_mode(interp, h, w, ho, wo)
    if mode == "area_table":
        return tuple(int((_axis_matrix(n, no, mode) != 0).sum(1).max()) for n, no in ((h, ho), (w, wo)))
    return (4, 4) if mode == "cubic" else (2, 2)


def cv_resize(imgs: Sequence[torch.Tensor], sizes: Sequence, interps: Sequence[int]) -> List[torch.Tensor]:
    """``cv2.resize(img, (wo, ho), interpolation=interp)`` for every image of a list: ``imgs[i]`` (C, h, w) -> (C, *sizes[i]) with
    ``sizes[i] = (ho, wo)`` and ``interps[i]`` 1, 2 or 3.  CUDA (fp32): one ``grl_cv_resize`` launch.  CPU: float64 weights and sums,
    the result in the input's dtype."""
    imgs = list(imgs)
    item_lists.check_images(imgs, "cv_resize")
    sizes = [(int(s[0]), int(s[1])) for s in sizes]
    interps = [int(i) for i in interps]
    if len(sizes) != len(imgs) or len(interps) != len(imgs):
        raise ValueError("cv_resize: one size and one interp per image")
    modes = [_resize_mode(ip, im.shape[1], im.shape[2], ho, wo) for im, (ho, wo), ip in zip(imgs, sizes, interps)]
    if any(ho < 1 or wo < 1 for ho, wo in sizes):
        raise ValueError("cv_resize: sizes are positive")
    if imgs[0].is_cuda:
        Cn = imgs[0].shape[0]
        shapes = [(Cn, ho, wo) for ho, wo in sizes]
        (src, so), (dst, do) = item_lists.pack(imgs), item_lists.empty(shapes, imgs[0].device)
        hip_cv_resize(src, dst, [(a, d, im.shape[1], im.shape[2], ho, wo, ip, 0)
                                 for a, d, im, (ho, wo), ip in zip(so, do, imgs, sizes, interps)], Cn)
        return item_lists.views(dst, do, shapes)
    out = []
    for im, (ho, wo), mode in zip(imgs, sizes, modes):
        wy, wx = _axis_matrix(im.shape[1], ho, mode), _axis_matrix(im.shape[2], wo, mode)
        out.append(torch.matmul(wy, torch.matmul(im.double(), wx.t())).to(im.dtype))
    return out


_items_tensor = item_lists.table


def hip_cv_resize(src: torch.Tensor, dst: torch.Tensor, items, Cn: int) -> None:
    """One ``grl_cv_resize`` launch.  ``src`` / ``dst``: flat fp32 CUDA arenas (they may be one tensor); ``items``: host tuples
    (src_off, dst_off, h, w, ho, wo, interp, 0).  This wrapper is what vouches for the item list: the grid maxima are taken from
    the items themselves, and the callers hand out disjoint destinations."""
    item_lists.launch("grl_cv_resize", src, dst, _items_tensor(items, src.device), C=Cn, max_ho=max(it[4] for it in items),
                      max_wo=max(it[5] for it in items))


# ---- blur -------------------------------------------------------------------------------------------------------------------------
def _mirror(idx: np.ndarray, n: int) -> np.ndarray:
    """scipy's ``mirror`` (reflect-101) of integer positions, folded as often as needed."""
    if n == 1:
        return np.zeros_like(idx)
    p = 2 * (n - 1)
    j = np.mod(idx, p)
    return np.where(j >= n, p - j, j)


def blur_items(imgs: Sequence[torch.Tensor], taps: Sequence[torch.Tensor], strides: Sequence[int]) -> List[torch.Tensor]:
    """``scipy.ndimage.correlate(img, taps, mode="mirror")[::s, ::s]`` per channel for every image of a list: ``taps[i]`` (K, K), K odd
    and at most 31 -- correlation taps, i.e. the kernel of ``ndimage.convolve`` flipped over both axes, as ``tasks.blur_taps`` makes
    them -- and ``strides[i] >= 1``; (C, h, w) -> (C, ceil(h / s), ceil(w / s)).  CUDA (fp32 images and taps): one ``grl_blur_items``
    launch, an fp32 fmaf chain per output.  CPU: float64 sums, the result in the input's dtype."""
    imgs, taps = list(imgs), list(taps)
    item_lists.check_images(imgs, "blur_items")
    strides = [int(s) for s in strides]
    if len(taps) != len(imgs) or len(strides) != len(imgs):
        raise ValueError("blur_items: one tap table and one stride per image")
    for t in taps:
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != t.shape[1] or t.shape[0] % 2 == 0 or t.shape[0] > KMAX:
            raise ValueError(f"blur_items: the taps are square tables with an odd side of at most {KMAX}")
    if any(s < 1 for s in strides):
        raise ValueError("blur_items: strides are at least 1")
    if imgs[0].is_cuda:
        Cn, dev = imgs[0].shape[0], imgs[0].device
        if any(t.dtype != torch.float32 for t in taps):
            raise TypeError("grl_blur_items takes fp32 taps")
        shapes = [(Cn, -(-im.shape[1] // s), -(-im.shape[2] // s)) for im, s in zip(imgs, strides)]
        (src, so), (tbuf, to), (dst, do) = item_lists.pack(imgs), item_lists.pack(taps), item_lists.empty(shapes, dev)
        hip_blur_items(src, dst, tbuf.to(dev), [(a, d, im.shape[1], im.shape[2], t.shape[0], s, k, 0)
                                                for a, d, k, im, t, s in zip(so, do, to, imgs, taps, strides)], Cn)
        return item_lists.views(dst, do, shapes)
    out = []
    for im, t, s in zip(imgs, taps, strides):
        Cn, h, w = im.shape
        K, half = t.shape[0], t.shape[0] // 2
        ho, wo = -(-h // s), -(-w // s)
        ry = torch.from_numpy(_mirror(np.arange(-half, (ho - 1) * s + half + 1), h))
        rx = torch.from_numpy(_mirror(np.arange(-half, (wo - 1) * s + half + 1), w))
        x = im.double()[:, ry][:, :, rx]
        y = F.conv2d(x[None], t.double().view(1, 1, K, K).expand(Cn, 1, K, K), stride=s, groups=Cn)[0]
        out.append(y.to(im.dtype))
    return out


def hip_blur_items(src: torch.Tensor, dst: torch.Tensor, taps: torch.Tensor, items, Cn: int) -> None:
    """One ``grl_blur_items`` launch.  ``src`` / ``dst``: flat fp32 CUDA arenas (they may be one tensor), ``taps``: the flat fp32 taps
    buffer on that device; ``items``: host tuples (src_off, dst_off, h, w, K, s, taps_off, 0).  As ``hip_cv_resize``, this wrapper
    vouches for the list: the maxima come from the items, the callers hand out disjoint destinations."""
    item_lists.launch("grl_blur_items", src, dst, _items_tensor(items, src.device), taps=taps.data_ptr(), taps_elems=taps.numel(), C=Cn,
                      max_ho=max(-(-it[2] // it[5]) for it in items), max_wo=max(-(-it[3] // it[5]) for it in items),
                      max_K=max(it[4] for it in items))


# ---- the blur kernels (host, float64) ---------------------------------------------------------------------------------------------
def fspecial_gaussian(hsize: int, sigma: float) -> np.ndarray:
    """MATLAB's ``fspecial('gaussian', hsize, sigma)`` as utils_sisr.py:169-180 restates it: (hsize, hsize) float64."""
    from .tasks import gaussian_blur_kernel

    return gaussian_blur_kernel(int(hsize), float(sigma)).numpy()


def anisotropic_gaussian(ksize: int = 15, theta: float = math.pi, l1: float = 6.0, l2: float = 6.0) -> np.ndarray:
    """utils_sisr.py:39-74: the density of N(0, V diag(l1, l2) V^-1), V = [[c, s], [s, -c]] for the angle ``theta``, at the points
    (x - (ksize - 1) / 2, y - (ksize - 1) / 2), divided by its sum.  The density is evaluated directly (the normalising constant
    drops out in the division); tests hold it against ``scipy.stats.multivariate_normal.pdf``."""
    c, s = math.cos(theta), math.sin(theta)
    V = np.array([[c, s], [s, -c]])
    sigma = V @ np.diag([float(l1), float(l2)]) @ np.linalg.inv(V)
    inv = np.linalg.inv(sigma)
    g = np.arange(ksize, dtype=np.float64) - (ksize / 2.0 + 0.5) + 1
    cx, cy = np.meshgrid(g, g)                         # k[y, x] is the density at (cx, cy)
    q = inv[0, 0] * cx * cx + (inv[0, 1] + inv[1, 0]) * cx * cy + inv[1, 1] * cy * cy
    k = np.exp(-0.5 * q)
    return k / k.sum()


def shift_kernel(k: np.ndarray, sf: int) -> np.ndarray:
    """``shift_pixel(k, sf)`` (utils_sisr.py:77-103): ``k`` interpolated bilinearly at ``min(i + (sf - 1) / 2, K - 1)`` on both axes
    (the reference's ``scipy.interpolate.interp2d``, which current scipy no longer has, did exactly that on its unit grid)."""
    k = np.asarray(k, dtype=np.float64)
    K = k.shape[0]
    p = np.minimum(np.arange(K) + (sf - 1) * 0.5, K - 1)
    i0 = np.floor(p).astype(np.int64)
    i1 = np.minimum(i0 + 1, K - 1)
    t = p - i0
    rows = k[i0] * (1 - t)[:, None] + k[i1] * t[:, None]
    return rows[:, i0] * (1 - t) + rows[:, i1] * t


def _taps32(k: np.ndarray) -> torch.Tensor:
    """The kernel of ``ndimage.convolve`` as fp32 correlation taps: cast and flipped over both axes (``tasks.blur_taps``)."""
    return torch.from_numpy(np.flip(np.asarray(k).astype(np.float32)).copy())


# ---- the draws --------------------------------------------------------------------------------------------------------------------
def _check_geometry(scale: int, crop: int):
    if scale not in (2, 4):
        raise ValueError(f"the degradation pipeline is built for scales 2 and 4 (int(1 / sf * n) is then exact), got {scale}")
    if crop % 4 or crop < 4 * scale:
        raise ValueError(f"the degradation crop is a multiple of 4 and at least 4 * scale = {4 * scale}, got {crop}")


def _corr_noise(rng) -> dict:
    """The channel-correlated covariance of utils_sisr.py:385-391: D = diag(rand(3)), U = orth(rand(3, 3)), conv = U^T D U,
    cov = |L^2 conv| with L = 25 / 255 -- twelve ``rng.random()`` draws, D first -- and the factor ``sqrt(s)[:, None] * v`` of its
    SVD through which ``numpy.random.multivariate_normal`` colours unit normals."""
    L = 25 / 255.0
    D = np.diag([rng.random() for _ in range(3)])
    A = np.array([[rng.random() for _ in range(3)] for _ in range(3)])
    U = np.linalg.svd(A)[0]                          # scipy.linalg.orth of a full-rank matrix: its left singular vectors
    cov = np.abs(L ** 2 * (U.T @ D @ U))
    _, sv, v = np.linalg.svd(cov)
    return {"cov": cov.tolist(), "transform": (np.sqrt(sv)[:, None] * v).tolist()}


def draw_plan(rng: random.Random, scale: int, crop: int, stages: Optional[Sequence[int]] = None, camera=None) -> List[dict]:
    """The degradation of ONE sample: every scalar draw of ``degradation_sr2`` from ``rng`` (the reference mixes ``random`` and
    ``np.random``; here all come from the one ``random.Random``), in the reference's order of decisions.  A pure function of the
    generator's state.  Returns a list of ops in execution order, each a dict with ``pos`` (0: the initial halving, 1 .. 9: the
    place in the shuffle, 10: the final JPEG), ``stage`` (-1, the stage number 0 .. 8, 9), ``op``, its parameters, and ``size``:
    the side of the square image after the op.

    Order of the draws, with sf = scale, n = crop:
      initial halving (sf == 4 only)  random() < 0.1: random() < 0.5 ? resize to n / 2 with choice([1, 2, 3]) : MATLAB imresize by
                      1 / 2; clip; n = n / 2, sf = 2
      the shuffle     sample(range(9), 9); stages 1 and 6 are swapped if 6 comes first, so stage 6 always follows stage 1
      per stage, in shuffled order (wd2 = 4 + sf, wd = 2 + 0.2 sf):
        0 blur        random() < 0.5 ? anisotropic: l1 = wd2 random(), l2 = wd2 random(), K = 2 randint(2, 11) + 3, theta = pi random()
                                     : isotropic: K = 2 randint(2, 11) + 3, sigma = wd random()
        1 downsample  a = n; random() < 0.5 ? sf1 = uniform(1, 2 sf), resize to int(n / sf1) with choice([1, 2, 3])
                                            : sigma = uniform(0.1, 0.4 sf), the 25 x 25 Gaussian shifted by (sf - 1) / 2 and
                                              renormalised, blur with stride sf;  clip
        2 camera noise  ``camera`` (an ``isp.CameraBank``) is None: no draw, no op.  Else random() > 0.75: choice of the 11 cameras,
                      choice of the 11 tone curves, FW = random(), d_r = 1.2 + 1.2 random(), d_b = 1.2 + 1.2 random(),
                      e = 0.2 random() - 0.1 (utils_isp.py:484-529), log_shot = uniform(log10(1e-4), log10(0.006)),
                      log_read = 2.275 log_shot + 1.47 + gauss(0, 0.25) clamped to +-1.5 (utils_noise.py:60-74); the op carries the
                      draws, shot = 10 ** log_shot, read = 10 ** log_read and ``params``, the record ``camera.params`` makes of
                      them.  No clip follows: the stage clamps.  A side below 3 raises (the demosaic reflects by 2).  One
                      deliberate difference: the reference keeps one camera, curve and exposure for 64 consecutive calls of a
                      data-loader worker (``self.count % 64``, an artefact of worker state) and redraws only the noise levels;
                      here every acting sample draws its own, so that a plan stays a pure function of the generator's state
        3 Gaussian noise  level = randint(2, 25); r = random(): r > 0.5 per pixel, r < 0.4 one value per pixel for all channels,
                      else channel-correlated (twelve random(): ``_corr_noise``); clip
        4 JPEG        random() < 0.9: quality = randint(20, 95)
        5 blur        isotropic: K = 2 randint(2, 11) + 3, sigma = wd random()
        6 downsample  resize to a / sf with choice([1, 2, 3]); clip
        7 speckle     level = randint(2, 24) (np.random.randint(2, 25)); random() > 0.5: clip; r = random(): r > 0.6 per pixel,
                      r < 0.4 gray, else correlated (twelve random()); clip
        8 Poisson     random() > 0.5: clip; vals = 10 ** (2 random() + 2); clip
      final JPEG      quality = randint(20, 95)

    ``stages``: the stage numbers that may act (default: all).  Every draw is made either way, so the stream does not depend on
    it; the ops of the other stages are left out (without stage 6 the plan does not end at crop / scale).  The initial halving and
    the final JPEG are not stages and always act.
    """
    scale, crop = int(scale), int(crop)
    _check_geometry(scale, crop)
    allowed = set(STAGES if stages is None else (int(s) for s in stages))
    if not allowed <= set(STAGES):
        raise ValueError(f"stages are numbers of 0 .. 8, got {sorted(allowed)}")
    ops: List[dict] = []
    sf, n = scale, crop

    def emit(pos, stage, op, size, **kw):
        ops.append(dict(pos=pos, stage=stage, op=op, size=size, **kw))

    if sf == 4 and rng.random() < 0.1:
        if rng.random() < 0.5:
            emit(0, -1, "resize", n // 2, interp=rng.choice([1, 2, 3]))
        else:
            emit(0, -1, "imresize_half", n // 2)
        emit(0, -1, "clip", n // 2)
        n, sf = n // 2, 2

    order = rng.sample(range(9), 9)
    i1, i6 = order.index(1), order.index(6)
    if i1 > i6:
        order[i1], order[i6] = order[i6], order[i1]
    wd2, wd = 4.0 + sf, 2.0 + 0.2 * sf
    a = n
    for pos, ii in enumerate(order, start=1):
        first = len(ops)
        if ii == 0:
            if rng.random() < 0.5:
                l1 = wd2 * rng.random()
                l2 = wd2 * rng.random()
                K = 2 * rng.randint(2, 11) + 3
                k = anisotropic_gaussian(K, rng.random() * math.pi, l1, l2)
            else:
                K = 2 * rng.randint(2, 11) + 3
                k = fspecial_gaussian(K, wd * rng.random())
            emit(pos, ii, "blur", n, kernel=k, stride=1)
        elif ii == 1:
            a = n
            if rng.random() < 0.5:
                sf1 = rng.uniform(1, 2 * sf)
                m = int(1 / sf1 * n)
                emit(pos, ii, "resize", m, interp=rng.choice([1, 2, 3]))
            else:
                k = shift_kernel(fspecial_gaussian(25, rng.uniform(0.1, 0.4 * sf)), sf)
                m = n // sf
                emit(pos, ii, "blur", m, kernel=k / k.sum(), stride=sf)
            emit(pos, ii, "clip", m)
            if ii in allowed:
                n = m
        elif ii == 2 and camera is not None:
            if rng.random() > 0.75:
                d = dict(camera=rng.choice(range(11)), curve=rng.choice(range(11)), fw=rng.random(), d_r=1.2 + 1.2 * rng.random(),
                         d_b=1.2 + 1.2 * rng.random(), e=0.2 * rng.random() - 0.1)
                log_shot = rng.uniform(math.log10(1e-4), math.log10(0.006))
                log_read = 2.275 * log_shot + 1.47 + min(max(rng.gauss(0.0, 0.25), -1.5), 1.5)
                d.update(shot=10 ** log_shot, read=10 ** log_read)
                if ii in allowed and n < 3:
                    raise ValueError(f"plan: the camera stage meets a side of {n}; its demosaic reflects by 2 and needs at least 3")
                emit(pos, ii, "camera", n, params=camera.params(d), **d)
        elif ii == 3:
            level = rng.randint(2, 25)
            r = rng.random()
            form = "pixel" if r > 0.5 else "gray" if r < 0.4 else "corr"
            emit(pos, ii, "gauss", n, level=level, form=form, **(_corr_noise(rng) if form == "corr" else {}))
            emit(pos, ii, "clip", n)
        elif ii == 4:
            if rng.random() < 0.9:
                emit(pos, ii, "jpeg", n, quality=rng.randint(20, 95))
        elif ii == 5:
            K = 2 * rng.randint(2, 11) + 3
            emit(pos, ii, "blur", n, kernel=fspecial_gaussian(K, wd * rng.random()), stride=1)
        elif ii == 6:
            m = a // sf
            emit(pos, ii, "resize", m, interp=rng.choice([1, 2, 3]))
            emit(pos, ii, "clip", m)
            if ii in allowed:
                n = m
        elif ii == 7:
            level = rng.randint(2, 24)
            if rng.random() > 0.5:
                emit(pos, ii, "clip", n)
                r = rng.random()
                form = "pixel" if r > 0.6 else "gray" if r < 0.4 else "corr"
                emit(pos, ii, "speckle", n, level=level, form=form, **(_corr_noise(rng) if form == "corr" else {}))
                emit(pos, ii, "clip", n)
        elif ii == 8:
            if rng.random() > 0.5:
                emit(pos, ii, "clip", n)
                emit(pos, ii, "poisson", n, vals=10 ** (2 * rng.random() + 2.0))
                emit(pos, ii, "clip", n)
        if ii not in allowed:
            del ops[first:]
    emit(10, 9, "jpeg_final", n, quality=rng.randint(20, 95))
    return ops


# ---- the noise stages -------------------------------------------------------------------------------------------------------------
def add_noise(img: torch.Tensor, op: dict, gen: Optional[torch.Generator] = None) -> torch.Tensor:
    """Stages 3, 7 and 8 (utils_sisr.py:372-453) on one (C, h, w) fp32 image, out of place, unclipped, with draws from ``gen`` on the
    image's device.  ``op``: an op of ``draw_plan`` -- "gauss" / "speckle" with ``level`` and ``form``: "pixel" (a normal draw per
    value at sigma = level / 255), "gray" (one per pixel, shared by the channels) or "corr" (three unit normals per pixel coloured
    by ``transform``, ``sqrt(s)[:, None] * v`` of the SVD of the covariance, as ``numpy.random.multivariate_normal`` does); speckle
    multiplies the noise by the image.  "poisson": ``poisson(img * vals) / vals``."""
    Cn, h, w = img.shape
    if op["op"] == "poisson":
        vals = float(op["vals"])
        return torch.poisson(img * vals, generator=gen) / vals
    randn = lambda c: torch.randn(c, h, w, generator=gen, device=img.device, dtype=torch.float32)
    if op["form"] == "pixel":
        noise = randn(Cn) * (op["level"] / 255.0)
    elif op["form"] == "gray":
        noise = randn(1) * (op["level"] / 255.0)
    else:
        if Cn != 3:
            raise ValueError("the channel-correlated noise is defined for three channels")
        T = torch.tensor(op["transform"], dtype=torch.float32, device=img.device)
        noise = torch.einsum("kc,khw->chw", T, randn(3))
    return img + (img * noise if op["op"] == "speckle" else noise)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------
class _Arenas:
    """Two arenas of N slots of C * crop * crop floats in one tensor.  Image b lives at the start of slot b of the arena
    ``side[b]``, contiguous (C, h, w); an op that changes the image's size or cannot run in place writes into the same slot of the
    other arena (no image of the pipeline is larger than the crop).  Offsets are in elements of the whole tensor."""

    def __init__(self, x: torch.Tensor):
        self.N, self.C, self.S = x.shape[0], x.shape[1], x.shape[2]
        self.slot = self.C * self.S * self.S
        self.buf = ops.empty(2, self.N, self.slot, dtype=torch.float32, device=x.device)
        self.buf[0].copy_(x.reshape(self.N, -1))
        self.flat = self.buf.view(-1)
        self.side = [0] * self.N
        self.size = [self.S] * self.N

    def offset(self, b: int, side: int) -> int:
        return (side * self.N + b) * self.slot

    def view(self, b: int, side: Optional[int] = None, size: Optional[int] = None) -> torch.Tensor:
        side = self.side[b] if side is None else side
        n = self.size[b] if size is None else size
        return self.buf[side, b, : self.C * n * n].view(self.C, n, n)

    def moved(self, b: int, size: int):
        self.side[b], self.size[b] = 1 - self.side[b], size


def _run_items(ar: _Arenas, group, on_device, on_host):
    """One image op for the samples of ``group``, each from its side of the arenas into the other.  CUDA: ``on_device(heads)`` with
    the items' (src_off, dst_off, h, w).  CPU: ``on_host(images)`` returns the results, which are copied over.  Then the samples
    have moved."""
    if ar.buf.is_cuda:
        on_device([(ar.offset(b, ar.side[b]), ar.offset(b, 1 - ar.side[b]), ar.size[b], ar.size[b]) for b, _ in group])
    else:
        for (b, op), o in zip(group, on_host([ar.view(b) for b, _ in group])):
            ar.view(b, 1 - ar.side[b], op["size"]).copy_(o)
    for b, op in group:
        ar.moved(b, op["size"])


def _run_resize(ar: _Arenas, group):
    sizes, interps = [op["size"] for _, op in group], [op["interp"] for _, op in group]
    _run_items(ar, group,
               lambda heads: hip_cv_resize(ar.flat, ar.flat, [(*hd, n, n, ip, 0) for hd, n, ip in zip(heads, sizes, interps)], ar.C),
               lambda imgs: cv_resize(imgs, [(n, n) for n in sizes], interps))


def _run_blur(ar: _Arenas, group):
    taps, strides = [_taps32(op["kernel"]) for _, op in group], [op["stride"] for _, op in group]
    for b, op in group:
        if -(-ar.size[b] // op["stride"]) != op["size"]:
            raise ValueError(f"plan: a stride-{op['stride']} blur of side {ar.size[b]} does not give side {op['size']}")

    def on_device(heads):
        tbuf, to = item_lists.pack(taps)
        hip_blur_items(ar.flat, ar.flat, tbuf.to(ar.buf.device),
                       [(*hd, t.shape[0], s, k, 0) for hd, t, s, k in zip(heads, taps, strides, to)], ar.C)

    _run_items(ar, group, on_device, lambda imgs: blur_items(imgs, taps, strides))


def _camera_normals(gen, side: int, device) -> torch.Tensor:
    """The unit normals of one item of the camera stage: one ``randn`` of (side, side) from ``gen``."""
    return torch.randn(side, side, generator=gen, device=device, dtype=torch.float32)


def _run_camera(ar: _Arenas, group, gen, hr):
    """Stage 2 for the samples of ``group``: normals from ``gen``, one draw per item in batch order, then one ``isp.camera_noise``
    over the arenas -- on CUDA the raw plane goes into the item's slot of the other arena and the result back into its own, and the
    HR pass rewrites the items' images of ``hr`` in place."""
    from . import isp

    params = [op["params"] for _, op in group]
    if any(ar.size[b] < isp.MIN_SIDE for b, _ in group):
        raise ValueError(f"plan: the camera stage needs sides of at least {isp.MIN_SIDE}")
    z = [_camera_normals(gen, ar.size[b], ar.buf.device) for b, _ in group]
    if ar.buf.is_cuda:
        heads = [(ar.offset(b, ar.side[b]), ar.offset(b, 1 - ar.side[b]), ar.size[b]) for b, _ in group]
        normals, zo = item_lists.pack(z)
        isp.hip_isp("grl_isp_unprocess", ar.flat, ar.flat, [(here, there, n, n, o) for (here, there, n), o in zip(heads, zo)], params, normals)
        isp.hip_isp("grl_isp_process", ar.flat, ar.flat, [(there, here, n, n, 0) for here, there, n in heads], params)
        if hr is not None:
            S, flat = hr.shape[2], hr.view(-1)
            isp.hip_isp("grl_isp_roundtrip", flat, flat, [(b * 3 * S * S, b * 3 * S * S, S, S, 0) for b, _ in group], params)
    else:
        lq, sharp = isp.camera_noise([ar.view(b) for b, _ in group], None if hr is None else [hr[b] for b, _ in group], params, z)
        for i, (b, _) in enumerate(group):
            ar.view(b).copy_(lq[i])
            if hr is not None:
                hr[b].copy_(sharp[i])


def apply_plans(x: torch.Tensor, plans: Sequence[List[dict]], gen: Optional[torch.Generator] = None, parts: bool = False,
                hr: Optional[torch.Tensor] = None):
    """A batch ``x`` (N, C, crop, crop) fp32 in [0, 1] through the plans of ``draw_plan`` (one per sample): walks the positions of the
    shuffles; at each position the samples are grouped by op, and each kind of image op is ONE call with an item list over two
    ping-pong arenas (``grl_cv_resize``, ``grl_blur_items`` on CUDA; the float64 restatements, rounded to fp32 per op, on the CPU).
    The mid-pipeline JPEG goes through ``tasks.jpeg_roundtrip`` per group of equal size, the noise stages are torch expressions
    drawing from ``gen`` (a generator on ``x``'s device), the final JPEG is one batch with a quality per sample.  Returns
    (N, C, m, m) with m the plans' common final side (crop / scale) on the k / 255 grid; with ``parts`` also the batch before the
    final JPEG and the int32 qualities: ``(out, pre, q)`` with ``out == tasks.jpeg_roundtrip(pre, q)``.
    The samples whose op at a position is ``camera`` (``draw_plan`` with a bank) form one group: ``_run_camera``.  ``hr``: a CLONE of
    the batch, fp32 contiguous of ``x``'s shape and device -- the reference hands the stage the HR next to the LQ and takes both back
    (utils_sisr.py:369; restoration_bsr.py:107-108, 114 make it the target).  The stage's HR pass rewrites the images of the acting
    samples in place, and ``hr`` is returned as the last element: ``(out, hr)`` / ``(out, pre, q, hr)``.  Without ``hr`` the HR
    pass is not run and the return value is as above."""
    from . import tasks

    if x.dim() != 4 or x.shape[2] != x.shape[3] or x.shape[1] not in (1, 3) or x.shape[0] < 1 or x.dtype != torch.float32:
        raise ValueError(f"apply_plans: need an fp32 (N, C, crop, crop) batch with C = 1 or 3, got {x.dtype} {tuple(x.shape)}")
    if len(plans) != x.shape[0]:
        raise ValueError(f"apply_plans: {len(plans)} plans for a batch of {x.shape[0]}")
    if hr is not None and (hr.shape != x.shape or hr.dtype != x.dtype or hr.device != x.device or not hr.is_contiguous() or x.shape[1] != 3):
        raise ValueError("apply_plans: hr is a contiguous clone of the batch (three channels)")
    ar = _Arenas(x)
    for pos in range(10):
        per = [[op for op in plan if op["pos"] == pos] for plan in plans]
        for b, ops in enumerate(per):
            if any(op["op"] in ("resize", "blur", "jpeg", "camera") for op in ops[1:]):
                raise ValueError("plan: an image op, a JPEG or the camera stage is the first op of its position")
        for kind, run in (("resize", _run_resize), ("blur", _run_blur)):
            group = [(b, ops[0]) for b, ops in enumerate(per) if ops and ops[0]["op"] == kind]
            if group:
                run(ar, group)
        group = [(b, ops[0]) for b, ops in enumerate(per) if ops and ops[0]["op"] == "camera"]
        if group:
            _run_camera(ar, group, gen, hr)
        by_size = {}
        for b, ops in enumerate(per):
            if ops and ops[0]["op"] == "jpeg":
                by_size.setdefault(ar.size[b], []).append((b, ops[0]))
        for group in by_size.values():
            out = tasks.jpeg_roundtrip(torch.stack([ar.view(b) for b, _ in group]), [op["quality"] for _, op in group])
            for (b, _), o in zip(group, out):
                ar.view(b).copy_(o)
        for b, ops in enumerate(per):
            for op in ops:
                if op["op"] == "clip":
                    ar.view(b).clamp_(0.0, 1.0)
                elif op["op"] in ("gauss", "speckle", "poisson"):
                    ar.view(b).copy_(add_noise(ar.view(b), op, gen))
                elif op["op"] == "imresize_half":
                    o = tasks.imresize(ar.view(b), 0.5)
                    ar.view(b, 1 - ar.side[b], op["size"]).copy_(o)
                    ar.moved(b, op["size"])
                elif op["op"] not in ("resize", "blur", "jpeg", "camera"):
                    raise ValueError(f"plan: unknown op {op['op']!r}")
    final = [[op for op in plan if op["pos"] == 10] for plan in plans]
    if any(len(f) != 1 or f[0]["op"] != "jpeg_final" for f in final) or len(set(ar.size)) != 1:
        raise ValueError("apply_plans: every plan ends with one final JPEG, and all of them at one size")
    pre = torch.stack([ar.view(b) for b in range(ar.N)])
    q = torch.tensor([f[0]["quality"] for f in final], dtype=torch.int32)
    out = tasks.jpeg_roundtrip(pre, q)
    ret = (out, pre, q) if parts else (out,)
    if hr is not None:
        ret += (hr,)
    return ret if len(ret) > 1 else out


# ---- a frozen validation set ------------------------------------------------------------------------------------------------------
def main(argv: Optional[List[str]] = None):
    from PIL import Image

    from .evaluate import gt_images
    from .image8 import ImageWriter

    ap = argparse.ArgumentParser(description="A frozen blind-SR validation set: every GT image centre-cropped and degraded once")
    ap.add_argument("--gt", required=True, help="folder of clean images")
    ap.add_argument("--out", required=True, help="receives LQ/<stem>.png and GT/<stem>.png")
    ap.add_argument("--scale", type=int, default=4, choices=[2, 4])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--crop", type=int, default=400, help="side of the centre crop (a multiple of 4, at least 4 * scale)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--camera-profiles", default=None,
                    help="the reference's utils/cameraprofile folder: turns on stage 2, the camera-noise model (isp.CameraBank.load)")
    a = ap.parse_args(argv)
    try:
        _check_geometry(a.scale, a.crop)
        if a.camera_profiles is not None and a.crop < 32:
            raise ValueError(f"with --camera-profiles the crop is at least 32 (no side of the pipeline may fall below 3), got {a.crop}")
    except ValueError as e:
        ap.error(str(e))
    camera = None
    if a.camera_profiles is not None:
        from .isp import CameraBank

        camera = CameraBank.load(a.camera_profiles)
    device = torch.device(a.device)
    rng = random.Random(a.seed)
    gen = torch.Generator(device=device).manual_seed(a.seed)
    for sub in ("LQ", "GT"):
        os.makedirs(os.path.join(a.out, sub), exist_ok=True)
    written = []
    with ImageWriter() as writer:
        for path in gt_images(a.gt):
            im = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
            H, W = im.shape[:2]
            if H < a.crop or W < a.crop:
                ap.error(f"{path}: {H} x {W} is smaller than the crop {a.crop}")
            y, x = (H - a.crop) // 2, (W - a.crop) // 2
            gt = torch.from_numpy(im[y : y + a.crop, x : x + a.crop].copy()).permute(2, 0, 1)[None].float().div(255).to(device)
            if camera is None:
                lq = apply_plans(gt, [draw_plan(rng, a.scale, a.crop)], gen)
            else:
                lq, gt = apply_plans(gt, [draw_plan(rng, a.scale, a.crop, camera=camera)], gen, hr=gt.clone())
            stem = os.path.splitext(os.path.basename(path))[0]
            writer.write(os.path.join(a.out, "LQ", stem + ".png"), lq)
            writer.write(os.path.join(a.out, "GT", stem + ".png"), gt)
            written.append(stem)
    print(f"{len(written)} pairs at x{a.scale} under {a.out}", flush=True)
    return written


if __name__ == "__main__":
    main()
