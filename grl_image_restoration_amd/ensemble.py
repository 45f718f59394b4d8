"""Geometric self-ensemble at test time, the "+" rows of restoration tables: the image is restored under the eight flips and
rotations of the square, each result is mapped back, and the eight are averaged.

The transforms are the reference's ``Augment_RGB_torch.transform0 .. transform7`` (utils/dataset_utils.py:6-39:
``torch.rot90(t, k, dims=[-1, -2])``, with ``.flip(-2)`` after it for k >= 4); the reference lists them and never calls them from
its engine.  As index maps, ``y = T_k(x)`` for ``x`` of H rows and W columns:

    k   y[i, j] =               shape of y   inverse
    0   x[i, j]                 H x W        T0
    1   x[H-1-j, i]             W x H        T3
    2   x[H-1-i, W-1-j]         H x W        T2
    3   x[j, W-1-i]             W x H        T1
    4   x[H-1-i, j]             H x W        T4
    5   x[H-1-j, W-1-i]         W x H        T5
    6   x[i, W-1-j]             H x W        T6
    7   x[j, i]                 W x H        T7

Group A (0, 2, 4, 6) keeps the shape, group B (1, 3, 5, 7) transposes it.  The ensemble is

    out = (((m0 + m1) + (m2 + m3)) + ((m4 + m5) + (m6 + m7))) * 0.125,     m_k = T_k^-1(f(T_k(x)))

with the adds in exactly this order: the scaling by a power of two is exact, so the kernels and the torch restatement below give the
same bits.

  dihedral_pack    x -> (a, b): the group-A and the group-B transforms, each a member-major batch.  CUDA: one ``grl_dihedral_pack``
                   launch (csrc/ensemble.hip) that reads ``x`` once through its strides; CPU: ``transform`` and a ``cat``
  dihedral_merge   the eight member outputs -> their mean on the untransformed grid.  CUDA: one ``grl_dihedral_merge`` launch that
                   reads every member where the model left it (any strides, fp32 or fp16); CPU: ``transform`` and the sum above
  SelfEnsemble     a model wrapped so that every call is the ensemble; ``evaluate --self-ensemble``, ``restore --self-ensemble``

A CUDA tensor never takes the torch restatement: without libgrl_hip.so the launch raises, as everywhere else in the package.
"""
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import ops

GROUP_A: Tuple[int, ...] = (0, 2, 4, 6)
GROUP_B: Tuple[int, ...] = (1, 3, 5, 7)
INVERSE: Tuple[int, ...] = (0, 3, 2, 1, 4, 5, 6, 7)


def transform(x: torch.Tensor, k: int) -> torch.Tensor:
    """``T_k`` of the table above on the last two dimensions (a view or a copy; any dtype, any device)."""
    if k == 0:
        return x
    if k == 1:
        return x.flip(-2).transpose(-2, -1)
    if k == 2:
        return x.flip(-2, -1)
    if k == 3:
        return x.flip(-1).transpose(-2, -1)
    if k == 4:
        return x.flip(-2)
    if k == 5:
        return x.flip(-2, -1).transpose(-2, -1)
    if k == 6:
        return x.flip(-1)
    if k == 7:
        return x.transpose(-2, -1)
    raise ValueError(f"dihedral transforms are numbered 0 .. 7, got {k!r}")


def _check_image(x, what: str):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{what}: need a non-empty (B, C, H, W) tensor, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")


def _pack(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """``dihedral_pack`` and, for a square image, the (8B, C, H, H) buffer whose halves the two groups are (else None)."""
    _check_image(x, "dihedral_pack")
    B, C, H, W = x.shape
    if x.is_cuda and x.dtype != torch.float32:
        raise TypeError(f"dihedral_pack takes fp32 tensors on the GPU, got {x.dtype}")
    whole = None
    if H == W:
        whole = ops.empty((8 * B, C, H, W), dtype=x.dtype, device=x.device)
        a, b = whole[: 4 * B], whole[4 * B:]
    else:
        a = ops.empty((4 * B, C, H, W), dtype=x.dtype, device=x.device)
        b = ops.empty((4 * B, C, W, H), dtype=x.dtype, device=x.device)
    if x.is_cuda:
        ops.dihedral_pack(x, a, b)
    else:
        for group, dst in ((GROUP_A, a), (GROUP_B, b)):
            for n, k in enumerate(group):
                dst[n * B : (n + 1) * B].copy_(transform(x, k))
    return a, b, whole


def dihedral_pack(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(a, b) of an image batch (B, C, H, W): ``a`` (4B, C, H, W) holds T0, T2, T4, T6 of the batch and ``b`` (4B, C, W, H) holds T1,
    T3, T5, T7, member-major (``a[n * B + i]`` is the n-th transform of group A of image i), both contiguous; for H == W they are the
    two halves of one (8B, C, H, H) buffer.  A CUDA tensor (fp32, any strides: a crop or a channels-last view is read in place)
    takes one ``grl_dihedral_pack`` launch on the current stream; a CPU tensor takes ``transform`` in its own dtype."""
    a, b, _ = _pack(x)
    return a, b


def dihedral_merge(members: Sequence[torch.Tensor]) -> torch.Tensor:
    """The mean of the eight member outputs on the untransformed grid.  ``members[k]`` is what the model made of ``T_k(x)``:
    (B, C, Ho, Wo) for even k, (B, C, Wo, Ho) for odd k, any strides.  Each is mapped back by its inverse and
    ``(((m0 + m1) + (m2 + m3)) + ((m4 + m5) + (m6 + m7))) * 0.125`` is taken in that order -- not ``torch.mean``, whose order is
    unspecified -- so CPU and GPU agree to the bit; NaN and Inf propagate.  CUDA members (all fp32 or all fp16) take one
    ``grl_dihedral_merge`` launch and give fp32; CPU members are summed in their own dtype, 16-bit ones in fp32."""
    members = list(members)
    if len(members) != 8:
        raise ValueError(f"dihedral_merge takes the eight member outputs, got {len(members)}")
    _check_image(members[0], "dihedral_merge")
    B, C, Ho, Wo = members[0].shape
    dt, dev = members[0].dtype, members[0].device
    for k, m in enumerate(members):
        want = (B, C, Wo, Ho) if k % 2 else (B, C, Ho, Wo)
        if not isinstance(m, torch.Tensor):
            raise TypeError(f"dihedral_merge: member {k} is a {type(m).__name__}, not a tensor")
        if tuple(m.shape) != want or m.dtype != dt or m.device != dev:
            raise ValueError(f"dihedral_merge: member {k} should be {want} {dt} on {dev}, got {tuple(m.shape)} {m.dtype} on {m.device}")
    if members[0].is_cuda:
        if dt not in (torch.float32, torch.float16):
            raise TypeError(f"dihedral_merge takes fp32 or fp16 members on the GPU, got {dt}")
        out = ops.empty((B, C, Ho, Wo), dtype=torch.float32, device=dev)
        ops.dihedral_merge(members, out)
        return out
    acc = torch.float32 if dt in (torch.float16, torch.bfloat16) else dt
    m = [transform(t.to(acc), INVERSE[k]) for k, t in enumerate(members)]
    return (((m[0] + m[1]) + (m[2] + m[3])) + ((m[4] + m[5]) + (m[6] + m[7]))) * 0.125


class SelfEnsemble:
    """``model`` with the x8 self-ensemble around every call: ``SelfEnsemble(model)(x)`` packs ``x`` (B, C, H, W) into its eight
    transforms, runs ``model`` on them under ``no_grad`` and merges the eight outputs (fp32).  ``model`` is any callable from an
    image batch to an image batch whose output size follows the input's (any scale, any channel counts).

    Members are run whole, as many per forward as fit into ``max_batch`` images and at least one, so every member's B images sit
    in one output tensor: a square input with B = 1 is ONE forward of batch 8 -- the shape the chip is at its best on --, a
    non-square image is group A in one forward and group B in another.  A batch above ``max_batch`` goes through the whole
    ensemble in sub-batches of ``max_batch``.

    Dual-pixel pairs (6 channels in, 3 out) are transformed as ONE 6-channel image; the left and the right view are not swapped
    under a horizontal flip.  That is what the model was trained on: the training augmentation flips and rotates the two views and
    the target together.

    Passed to ``tiling.forward_tiled`` as its model, every tile gets its own ensemble: a chunk of square tiles becomes batches of
    eight transformed tiles, and the stitch is unchanged.  This is NOT the ensemble of eight whole tiled passes: the tile origins
    (``range(0, dim - tile, tile - overlap) + [dim - tile]``) are not symmetric under a flip, so a whole pass over a flipped image
    cuts other tiles.  The ensemble of whole tiled passes is ``SelfEnsemble(lambda x: forward_tiled(model, x, ...))``.

    ``out_channels`` is the wrapped model's; ``eval()`` and ``to()`` are passed on to it and return the wrapper."""

    def __init__(self, model: Callable[[torch.Tensor], torch.Tensor], max_batch: int = 8):
        if isinstance(max_batch, bool) or not isinstance(max_batch, int) or max_batch < 1:
            raise ValueError(f"SelfEnsemble: max_batch is a positive integer, got {max_batch!r}")
        self.model = model
        self.max_batch = max_batch

    @property
    def out_channels(self):
        return getattr(self.model, "out_channels", None)

    def eval(self):
        if hasattr(self.model, "eval"):
            self.model.eval()
        return self

    def to(self, *args, **kwargs):
        if hasattr(self.model, "to"):
            self.model = self.model.to(*args, **kwargs)
        return self

    @torch.no_grad()
    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        _check_image(x, "SelfEnsemble")
        B = x.shape[0]
        if B > self.max_batch:
            return torch.cat([self(x[s : s + self.max_batch]) for s in range(0, B, self.max_batch)], dim=0)
        a, b, whole = _pack(x)
        runs = [(whole, GROUP_A + GROUP_B)] if whole is not None else [(a, GROUP_A), (b, GROUP_B)]
        per = max(1, self.max_batch // B)                     # whole members per forward
        members: List[Optional[torch.Tensor]] = [None] * 8
        for batch, ks in runs:
            for s in range(0, len(ks), per):
                out = self.model(batch[s * B : (s + per) * B])
                for n, k in enumerate(ks[s : s + per]):
                    members[k] = out[n * B : (n + 1) * B]
        return dihedral_merge(members)
