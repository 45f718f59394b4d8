"""The host half of the item-list entries (include/grl_hip.h, "ITEM LIST"; csrc/item_list.h): ``grl_cv_resize``, ``grl_blur_items``,
``grl_isp_unprocess`` / ``_process`` / ``_roundtrip`` and ``grl_color_jitter`` work on lists of images whose sizes differ -- flat fp32
arenas, and a device table of eight int64 per item: src_off, dst_off, h, w and four slots the entry names.  Whoever calls ``launch``
vouches for the list: the maxima it passes bound the items, and the destinations are disjoint.

  check_images   the validation of a list of (C, h, w) tensors
  pack, views    a list of tensors as one flat arena plus element offsets, and the results sliced back out
  empty          an arena that is yet to be written, for results of given shapes, and their offsets
  table          host rows -> the (n, 8) int64 device table
  args, launch   the fields every entry shares (src, dst, src_elems, dst_elems, items, n_items) filled in, and the call
"""
import math
from typing import List, Sequence, Tuple

import torch

from . import _lib, ops

ROW = 8


def check_images(imgs, what: str, channels: Sequence[int] = (1, 3), min_side: int = 1) -> None:
    """``imgs``: at least one (C, h, w) tensor, one C of ``channels``, sides of at least ``min_side``, one device and dtype -- else
    ValueError; CUDA tensors that are not fp32: TypeError."""
    shape = f"({channels[0]}, h, w)" if len(channels) == 1 else f"(C, h, w) with one C of {' or '.join(map(str, channels))}"
    if len(imgs) < 1:
        raise ValueError(f"{what}: no images")
    for im in imgs:
        if not torch.is_tensor(im) or im.dim() != 3 or im.shape[0] != imgs[0].shape[0] or im.shape[0] not in channels:
            raise ValueError(f"{what}: a list of {shape} tensors")
        if min(im.shape[1:]) < min_side:
            raise ValueError(f"{what}: a side is at least {min_side}, got {tuple(im.shape[1:])}")
        if im.device != imgs[0].device or im.dtype != imgs[0].dtype:
            raise ValueError(f"{what}: the images share one device and dtype")
    if imgs[0].is_cuda and imgs[0].dtype != torch.float32:
        raise TypeError(f"{what} takes fp32 CUDA tensors, got {imgs[0].dtype}")


def _layout(counts: Sequence[int], align: int) -> Tuple[List[int], int]:
    """Element offsets of consecutive blocks of ``counts`` elements, each starting on a multiple of ``align``, and the total."""
    offs, at = [], 0
    for n in counts:
        offs.append(at)
        at += -(-n // align) * align
    return offs, at


def pack(tensors: Sequence[torch.Tensor], align: int = 1) -> Tuple[torch.Tensor, List[int]]:
    """The tensors, flattened, in one arena: ``(arena, offsets)``.  ``align`` > 1: every tensor starts on a multiple of ``align``
    elements and the gaps are zero."""
    offs, total = _layout([t.numel() for t in tensors], align)
    if align == 1:
        return torch.cat([t.reshape(-1) for t in tensors]), offs
    arena = torch.zeros(total, dtype=tensors[0].dtype, device=tensors[0].device)
    for t, o in zip(tensors, offs):
        arena[o : o + t.numel()] = t.reshape(-1)
    return arena, offs


def empty(shapes: Sequence[Sequence[int]], device, align: int = 1) -> Tuple[torch.Tensor, List[int]]:
    """An uninitialised fp32 arena for tensors of ``shapes``, laid out as ``pack`` would: ``(arena, offsets)``."""
    offs, total = _layout([math.prod(s) for s in shapes], align)
    return ops.empty(total, dtype=torch.float32, device=device), offs


def views(arena: torch.Tensor, offsets: Sequence[int], shapes: Sequence[Sequence[int]]) -> List[torch.Tensor]:
    """``arena[offsets[i] :]`` as a tensor of ``shapes[i]``, for every i."""
    return [arena[o : o + math.prod(s)].view(*s) for o, s in zip(offsets, shapes)]


def table(rows, device) -> torch.Tensor:
    """Host rows of eight integers as the (n, 8) int64 device table."""
    return torch.tensor(rows, dtype=torch.int64).reshape(-1, ROW).to(device)


def args(entry: str, src: torch.Tensor, dst: torch.Tensor, items: torch.Tensor, **fields):
    """The argument struct of ``entry`` over the flat arenas ``src`` / ``dst`` (they may be one tensor) and the device table
    ``items``; ``fields``: the entry's own."""
    struct = _lib.SIGNATURES[entry][1][1]._type_
    return struct(src=src.data_ptr(), dst=dst.data_ptr(), src_elems=src.numel(), dst_elems=dst.numel(), items=items.data_ptr(),
                  n_items=items.shape[0], **fields)


def launch(entry: str, src: torch.Tensor, dst: torch.Tensor, items: torch.Tensor, **fields) -> None:
    """One call of ``entry`` on the current stream; raises unless it returns 0."""
    _lib.launch(entry, args(entry, src, dst, items, **fields))
