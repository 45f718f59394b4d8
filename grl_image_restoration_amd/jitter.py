"""The colour jitter of the reference's blind-SR training branch: ``T.ColorJitter(brightness=0.2, contrast=0.2, saturation=0.2,
hue=0.05)`` on every GT crop before anything else happens to it (data/datasets/restoration_bsr.py:66-68,100).  The transform is
torchvision's ``ColorJitter.forward`` on a float RGB tensor in [0, 1]; its arithmetic is stated in include/grl_hip.h
(grl_color_jitter), written from torchvision's published source.  torchvision is not a dependency of this package and no run of it
backs the tests: the kernels are held to the float64 evaluation of that statement below, and its hue step to Python's ``colorsys``.
Not claimed: bit equality with a torchvision run, and the summation order of ``torch.mean`` behind the contrast mean.

  draw_jitter     one parameter set ``(order, b, c, s, h)`` as ``ColorJitter.get_params`` draws it: ``torch.randperm(4)``, then
                  three ``uniform_(0.8, 1.2)`` and one ``uniform_(-0.05, 0.05)`` of ``torch.empty(1)``, all from one CPU generator.
                  The reference draws from torch's global generator, a stream apart from the Python ``random`` of the degradation.
  color_jitter    lists of (3, h, w) images through the transform, one parameter set each.  CUDA tensors (fp32): one
                  ``grl_color_jitter`` call for the whole list (csrc/jitter.hip; there is no fallback).  CPU tensors: the torch
                  restatement below in the tensors' dtype, every operation rounded to it -- in float64 the yardstick of the
                  kernels, in fp32 the arithmetic of torchvision's own functions.
  JitterLists     the device lists of a fixed batch of equal crops (item table, factors, partial sums, means), rewritten in place
                  per batch so that a captured launch reads the same addresses; ``PatchSampler(jitter=True)`` owns one.
"""
from typing import List, Sequence, Tuple

import torch

from . import item_lists, ops

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
RANGES = ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.05, 0.05))          # b, c, s, h of the reference's ColorJitter
JitterParams = Tuple[Tuple[int, int, int, int], float, float, float, float]


def draw_jitter(gen: torch.Generator) -> JitterParams:
    """``ColorJitter.get_params``: the order of the four ops (0 brightness, 1 contrast, 2 saturation, 3 hue) and the factors b, c, s,
    h -- fp32 values as Python floats -- by five draws from the CPU generator ``gen``, in that order."""
    order = torch.randperm(4, generator=gen)
    b, c, s, h = (float(torch.empty(1).uniform_(lo, hi, generator=gen)) for lo, hi in RANGES)
    return tuple(order.tolist()), b, c, s, h


# ---- the torch restatement (a (3, h, w) tensor; every operation in its dtype) --------------------------------------------------
def gray(x: torch.Tensor) -> torch.Tensor:
    return 0.2989 * x[0] + 0.587 * x[1] + 0.114 * x[2]


def blend(x: torch.Tensor, y, f: float) -> torch.Tensor:
    return (f * x + (1.0 - f) * y).clamp(0, 1)


def brightness(x: torch.Tensor, f: float) -> torch.Tensor:
    return blend(x, torch.zeros_like(x), f)


def contrast_mean(x: torch.Tensor) -> torch.Tensor:
    return gray(x).mean()


def contrast(x: torch.Tensor, f: float) -> torch.Tensor:
    return blend(x, contrast_mean(x), f)


def saturation(x: torch.Tensor, f: float) -> torch.Tensor:
    return blend(x, gray(x)[None], f)


def rgb2hsv(x: torch.Tensor) -> torch.Tensor:
    r, g, b = x.unbind(0)
    maxc, minc = x.max(0).values, x.min(0).values
    eq = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eq, ones, maxc)
    d = torch.where(eq, ones, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return torch.stack([h, s, maxc])


def hsv2rgb(x: torch.Tensor) -> torch.Tensor:
    h, s, v = x.unbind(0)
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - s * f)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    rows = torch.stack([torch.stack([v, q, p, p, t, v]), torch.stack([t, v, v, q, p, p]), torch.stack([p, p, t, v, v, q])])
    return rows.gather(1, i[None, None].expand(3, 1, *i.shape))[:, 0]


def hue(x: torch.Tensor, f: float) -> torch.Tensor:
    hsv = rgb2hsv(x)
    return hsv2rgb(torch.stack([torch.remainder(hsv[0] + f, 1.0), hsv[1], hsv[2]]))


_OPS = (brightness, contrast, saturation, hue)


def jitter_image(x: torch.Tensor, params: JitterParams, with_mean: bool = False):
    """One (3, h, w) image through the chain of ``params`` in its dtype; with ``with_mean`` also the contrast mean as it is taken."""
    order, factors = params[0], params[1:]
    mean = None
    for op in order:
        if op == CONTRAST:
            mean = contrast_mean(x)
        x = _OPS[op](x, factors[op])
    return (x, mean) if with_mean else x


# ---- the transform on lists of images ------------------------------------------------------------------------------------------
def _check_params(params: Sequence[JitterParams], n: int) -> None:
    if len(params) != n:
        raise ValueError("color_jitter: one parameter set (order, b, c, s, h) per image")
    for p in params:
        if len(p) != 5 or sorted(int(o) for o in p[0]) != [0, 1, 2, 3]:
            raise ValueError(f"color_jitter: a parameter set is (order, b, c, s, h) with order a permutation of 0 .. 3, got {p!r}")


def item_rows(items, params: Sequence[JitterParams]):
    """Host tuples (src_off, dst_off, h, w) and their parameter sets as the (n, 8) int64 item table and the (n, 4) fp32 factors."""
    rows = item_lists.table([[so, do, h, w, *p[0]] for (so, do, h, w), p in zip(items, params)], "cpu")
    return rows, torch.tensor([list(p[1:]) for p in params], dtype=torch.float32).reshape(-1, 4)


def num_workgroups(max_h: int, max_w: int) -> int:
    from . import _lib

    n = _lib.lib().grl_color_jitter_num_workgroups(int(max_h), int(max_w))
    _lib.check(min(n, 0), "grl_color_jitter_num_workgroups")
    return n


def hip_color_jitter(src: torch.Tensor, dst: torch.Tensor, rows: torch.Tensor, factors: torch.Tensor, partial: torch.Tensor,
                     means: torch.Tensor, max_h: int, max_w: int) -> None:
    """One ``grl_color_jitter`` call.  ``src`` / ``dst``: flat fp32 CUDA arenas (they may be one tensor); ``rows`` / ``factors``: the
    device tables of ``item_rows``; ``partial`` / ``means``: fp64 device buffers of at least n * ``num_workgroups(max_h, max_w)`` and n
    elements.  The caller vouches for the list: ``max_h`` / ``max_w`` bound the items, the destinations are disjoint."""
    item_lists.launch("grl_color_jitter", src, dst, rows, params=factors.data_ptr(), partial=partial.data_ptr(), n_partial=partial.numel(),
                      means=means.data_ptr(), C=3, max_h=max_h, max_w=max_w)


def color_jitter(imgs: Sequence[torch.Tensor], params: Sequence[JitterParams], with_means: bool = False):
    """``ColorJitter.forward`` for every image of a list: ``imgs[i]`` (3, h, w) in [0, 1], ``params[i]`` of ``draw_jitter``.  Returns
    new tensors of the inputs' shapes; with ``with_means`` also the contrast means, a float64 tensor on the images' device.
    CUDA (fp32 only): one ``grl_color_jitter`` call.  CPU: the restatement in the tensors' dtype."""
    imgs, params = list(imgs), list(params)
    item_lists.check_images(imgs, "color_jitter (RGB; the hue op needs three channels)", (3,))
    _check_params(params, len(imgs))
    if not imgs[0].is_cuda:
        res = [jitter_image(im, p, with_mean=True) for im, p in zip(imgs, params)]
        out = [r[0] for r in res]
        return (out, torch.stack([r[1].double() for r in res])) if with_means else out
    dev = imgs[0].device
    src, offs = item_lists.pack(imgs, align=4)                           # every image starts on 16 bytes: the float4 path
    dst = ops.empty_like(src)
    rows, factors = item_rows([(o, o, im.shape[1], im.shape[2]) for o, im in zip(offs, imgs)], params)
    max_h, max_w = max(im.shape[1] for im in imgs), max(im.shape[2] for im in imgs)
    partial = ops.empty(len(imgs) * num_workgroups(max_h, max_w), dtype=torch.float64, device=dev)
    means = ops.empty(len(imgs), dtype=torch.float64, device=dev)
    hip_color_jitter(src, dst, rows.to(dev), factors.to(dev), partial, means, max_h, max_w)
    out = item_lists.views(dst, offs, [im.shape for im in imgs])
    return (out, means) if with_means else out


class JitterLists:
    """The device lists of ``batch`` crops (3, side, side) that lie one after the other in one tensor.  ``run_`` jitters such a batch
    in place: on CUDA the parameter sets are written into the lists (same addresses every batch) and ``grl_color_jitter`` runs over
    the batch's own memory, src == dst; on the CPU the restatement."""

    def __init__(self, batch: int, side: int, device):
        self.batch, self.side, self.device = int(batch), int(side), torch.device(device)
        if self.device.type == "cuda":
            self.rows = torch.zeros(batch, 8, dtype=torch.int64, device=self.device)
            self.factors = torch.zeros(batch, 4, dtype=torch.float32, device=self.device)
            self.partial = torch.zeros(batch * num_workgroups(side, side), dtype=torch.float64, device=self.device)
            self.means = torch.zeros(batch, dtype=torch.float64, device=self.device)

    def run_(self, crops: torch.Tensor, params: Sequence[JitterParams]) -> torch.Tensor:
        B, S = crops.shape[0], self.side
        if crops.shape[1:] != (3, S, S) or not crops.is_contiguous():
            raise ValueError(f"jitter: a contiguous batch of (3, {S}, {S}) crops, got {tuple(crops.shape)}")
        _check_params(params, B)
        if not crops.is_cuda:
            for b in range(B):
                crops[b] = jitter_image(crops[b], params[b])
            return crops
        rows, factors = item_rows([(b * 3 * S * S, b * 3 * S * S, S, S) for b in range(B)], params)
        own = self if B == self.batch else JitterLists(B, S, crops.device)
        own.rows.copy_(rows)
        own.factors.copy_(factors)
        flat = crops.view(-1)
        hip_color_jitter(flat, flat, own.rows, own.factors, own.partial, own.means, S, S)
        return crops
