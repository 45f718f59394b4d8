"""Tiled whole-image inference, sharded over the GPUs of a node (BASELINE config 4).

Reference semantics (engines/base.py:90-116, ``forward_tile``): tiles of side ``tile`` start at
``range(0, dim - tile, tile - overlap) + [dim - tile]`` on both axes; every tile runs the full model
(its own reflect-pad and its own squeeze-excite pooling); outputs are summed into a canvas E, a
count canvas W gets ones, and the result is E / W (uniform averaging in the overlaps).

MI355X design: tiles are independent units.  The row-major tile list (the reference's loop order)
is cut into contiguous chunks, one per rank; a rank pushes its chunk through the network as
batches (B > 1 fills the 256 CUs much better than the reference's one-tile-at-a-time loop); ONE
collective -- an all-gather of the fixed-shape tile outputs over RCCL/xGMI (<= 13 MB per tile,
latency-bound, one shot) -- gives every rank all tiles, and every rank stitches them in the
reference's loop order, so the result is bitwise the serial loop's result for the same per-tile
outputs.  No other data-path collective exists.

The stitch of fp32 tile outputs on the GPU is one HIP launch per chunk (csrc/stitch.hip, grl_tile_stitch): every canvas pixel is
written once, the tile outputs are read in place and dropped chunk by chunk, and an optional blending window (``blend_window``:
linear or cosine ramps over the overlap) feathers the seams that uniform averaging leaves between tiles that disagree by an offset.
With a window of ones the kernel gives the bits of ``stitch``.
"""
import math
from typing import Callable, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import ops
from .geometry import tile_origins


def tile_list(h: int, w: int, tile: int, overlap: int) -> Tuple[int, List[Tuple[int, int]]]:
    """(effective tile side, [(h_idx, w_idx)] in the reference's row-major loop order)."""
    tile = min(tile, h, w)
    return tile, [(hi, wi) for hi in tile_origins(h, tile, overlap) for wi in tile_origins(w, tile, overlap)]


def shard_bounds(n: int, rank: int, world: int) -> Tuple[int, int, int]:
    """Contiguous chunk [lo, hi) of n tiles for ``rank`` and the padded per-rank count of the all-gather.  Balanced: the first
    n % world ranks take one tile more than the others, so no rank idles while another holds two tiles more than it needs to
    (the reference's default GoPro split, 6 tiles of 480, on 4 ranks: 2 2 1 1, not 2 2 2 0; 8 tiles of 384 on 8 ranks: one each).
    Whole tiles are the unit -- the tile list is the reference's and so is the result -- so with fewer tiles than ranks
    (6 tiles on 8 GPUs) the last ranks only take part in the collective."""
    q, r = divmod(n, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0), q + (1 if r else 0)


def shard_of_tile(t: int, n: int, world: int) -> Tuple[int, int]:
    """(rank, index inside the rank's chunk) of tile t under shard_bounds."""
    q, r = divmod(n, world)
    if t < r * (q + 1):
        return divmod(t, q + 1)
    k, i = divmod(t - r * (q + 1), max(q, 1))
    return r + k, i


BLENDS = ("uniform", "linear", "cosine")


def blend_window(kind: str, ts: int, ramp: int) -> torch.Tensor:
    """The 1-D blending window of a tile output of side ``ts`` (fp32, built on the host): with R = ``ramp`` = overlap * scale and
    m(i) = min(i + 1, ts - i, R), ``uniform`` (and any kind with R <= 1) is all ones, ``linear`` is fp32(m) / fp32(R) and ``cosine``
    is sin^2(pi m / (2 R)), evaluated in float64 and rounded.  Both ramps are 1 on the plateau and strictly positive at the rim, so
    a tile edge on the image border still carries its pixel alone.  A pixel's weight is the product of the window at its row and
    at its column inside the tile."""
    if kind not in BLENDS:
        raise ValueError(f"blend is one of {', '.join(BLENDS)}, got {kind!r}")
    if ts < 1:
        raise ValueError(f"a window of {ts} elements")
    if kind == "uniform" or ramp <= 1:
        return torch.ones(ts, dtype=torch.float32)
    i = torch.arange(ts, dtype=torch.int64)
    m = torch.minimum(torch.minimum(i + 1, ts - i), torch.tensor(int(ramp)))
    if kind == "linear":
        return m.to(torch.float32) / torch.tensor(float(ramp), dtype=torch.float32)
    return torch.sin(m.to(torch.float64) * (math.pi / (2 * int(ramp)))).square().to(torch.float32)


def check_window(window: torch.Tensor, ts: int) -> torch.Tensor:
    """A caller's window: a 1-D fp32 tensor of ``ts`` strictly positive, finite elements -- else ValueError."""
    if not torch.is_tensor(window) or window.dim() != 1 or window.dtype != torch.float32 or window.numel() != ts:
        raise ValueError(f"window: a 1-D fp32 tensor of {ts} elements (tile * scale)")
    if not bool((torch.isfinite(window) & (window > 0)).all()):
        raise ValueError("window: every element is finite and above 0")
    return window


def stitch(outs: Sequence[torch.Tensor], origins: Sequence[Tuple[int, int]], shape, tile: int, scale: int,
           window: Optional[torch.Tensor] = None) -> torch.Tensor:
    """E / W accumulation in the reference's order (engines/base.py:100-116).  ``window`` (1-D fp32, tile * scale elements): every
    tile output is weighted by w2 = window[:, None] * window[None, :] and W sums the weights -- the statement grl_tile_stitch is
    held to (include/grl_hip.h); without one, the reference's uniform average."""
    b, c, h, w = shape
    E = torch.zeros(b, c, h * scale, w * scale, dtype=outs[0].dtype, device=outs[0].device)
    Wt = torch.zeros_like(E)
    if window is not None:
        window = window.to(device=E.device, dtype=E.dtype)
        w2 = window[:, None] * window[None, :]
        for o, (hi, wi) in zip(outs, origins):
            E[..., hi * scale : (hi + tile) * scale, wi * scale : (wi + tile) * scale].add_(o * w2)
            Wt[..., hi * scale : (hi + tile) * scale, wi * scale : (wi + tile) * scale].add_(w2)
        return E.div_(Wt)
    for o, (hi, wi) in zip(outs, origins):
        E[..., hi * scale : (hi + tile) * scale, wi * scale : (wi + tile) * scale].add_(o)
        Wt[..., hi * scale : (hi + tile) * scale, wi * scale : (wi + tile) * scale].add_(torch.ones_like(o))
    return E.div_(Wt)


def _on_kernel(t: torch.Tensor) -> bool:
    """grl_tile_stitch takes fp32 CUDA tile outputs; everything else -- and outputs that autograd follows -- goes through ``stitch``."""
    return t.is_cuda and t.dtype == torch.float32 and not t.requires_grad


def forward_tiled(model: Callable[[torch.Tensor], torch.Tensor], x: torch.Tensor, tile: int, overlap: int, scale: int,
                  out_channels: Optional[int] = None, tile_batch: int = 8, group=None, force_collective: bool = False,
                  blend: str = "uniform", window: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Tiled inference of ``x`` (b, c, h, w).  With an initialised process group every rank passes the
    SAME ``x`` and receives the SAME stitched output; without one it is the single-GPU batched loop.
    ``force_collective``: run the all-gather branch even at world size 1 (RCCL smoke test on a single GPU).
    ``blend``: how overlapping tiles are mixed -- ``uniform`` (the reference's plain average, the default), ``linear`` or ``cosine``
    (``blend_window`` with a ramp of overlap * scale: feathered seams); ``window``: the caller's own 1-D fp32 window of tile * scale
    strictly positive elements instead.  fp32 CUDA tile outputs are stitched by grl_tile_stitch, each ``tile_batch`` chunk right
    after its forward into an uninitialised canvas (peak memory: the canvas and one chunk); other tensors by ``stitch``."""
    b, c, h, w = x.shape
    oc = out_channels or c
    tile, origins = tile_list(h, w, tile, overlap)
    n = len(origins)
    ts = tile * scale
    if window is not None:
        win = check_window(window, ts)
    else:
        win = blend_window(blend, ts, overlap * scale)
        if blend == "uniform" or overlap * scale <= 1:
            win = None
    distributed = dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or force_collective)
    rank, world = (dist.get_rank(group), dist.get_world_size(group)) if distributed else (0, 1)
    lo, hi, per = shard_bounds(n, rank, world)
    oy, ox = tile_origins(h, tile, overlap), tile_origins(w, tile, overlap)
    win_dev = None

    def kernel_stitch(canvas, outs, first):
        nonlocal win_dev
        if win is not None and win_dev is None:
            win_dev = win.to(outs[0].device)
        if canvas is None:
            canvas = ops.empty(b, oc, h * scale, w * scale, dtype=torch.float32, device=outs[0].device)
        ops.tile_stitch(canvas, outs, oy, ox, tile, scale, first, win_dev)
        return canvas

    mine, canvas = [], None
    for s in range(lo, hi, tile_batch):
        chunk = origins[s : min(s + tile_batch, hi)]
        # tiles of all b images are stacked on the batch axis: (len(chunk)*b, c, tile, tile)
        patch = torch.cat([x[..., hi_ : hi_ + tile, wi_ : wi_ + tile] for hi_, wi_ in chunk], dim=0)
        out = model(patch)
        del patch
        if not distributed and _on_kernel(out):
            assert not mine, "the model's outputs changed device or dtype between chunks"
            canvas = kernel_stitch(canvas, out.split(b, dim=0), s)      # read in place; the chunk's outputs die here
        else:
            assert canvas is None, "the model's outputs changed device or dtype between chunks"
            mine.extend(out.split(b, dim=0))
        del out
    if not distributed:
        return canvas if canvas is not None else stitch(mine, origins, (b, oc, h, w), tile, scale, win)

    # one fixed-shape all-gather of this rank's tile outputs (padded to `per` tiles)
    dev = x.device
    dtype = mine[0].dtype if mine else x.dtype
    send = torch.zeros(per, b, oc, ts, ts, dtype=dtype, device=dev)
    for i, o in enumerate(mine):
        send[i].copy_(o)
    recv = torch.empty(world * per, b, oc, ts, ts, dtype=dtype, device=dev)
    dist.all_gather_into_tensor(recv, send, group=group)
    outs = []
    for t in range(n):
        r, i = shard_of_tile(t, n, world)
        outs.append(recv[r * per + i])                                  # views into recv: the stitch reads them in place
    if _on_kernel(recv):
        return kernel_stitch(None, outs, 0)
    return stitch(outs, origins, (b, oc, h, w), tile, scale, win)
