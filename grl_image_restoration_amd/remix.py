"""Progressive training and MixUp: what the reference's engine does to every training batch between the loader and the model
(engines/base.py:144-169, utils/dataset_utils.py:43-60 ``MixUp_AUG``).  The transform is stated once, in include/grl_hip.h
(``grl_batch_remix``); in short, for ``lq`` (B, Cl, P, P) and ``gt`` (B, Cg, sP, sP):

  stage        ``bisect.bisect_left(S, n)`` of optimizer step ``n`` over the cumulative stage lengths ``S``: step ``n == S_0`` still
               belongs to stage 0, as in the reference
  mini-batch   ``idx = rng.sample(range(B), k=b)`` when ``b < B``; output sample i is input sample ``idx[i]``
  mini-patch   ``x0 = rng.randrange(P - p + 1)``, then ``y0`` likewise, when ``p < P``; LQ rows ``x0 : x0 + p``, columns
               ``y0 : y0 + p``, the target the same window times the scale
  MixUp        ``perm = randperm(b)``, ``lam = Beta(1.2, 1.2).rsample((b, 1))``; ``lam_i * x_i + (1 - lam_i) * x_perm[i]`` for lq and
               gt alike, on the already reduced batch; a fixed point of the permutation is still computed
  draw order   sample, x0, y0 from a ``random.Random``; then randperm, Beta from a CPU ``torch.Generator``

  stage_of      the stage of a step
  draw_remix    the draws of one step: a plan ``(idx, x0, y0, perm, lam)``
  batch_remix   a plan applied to a batch.  CUDA: one ``grl_batch_remix`` launch (csrc/remix.hip) for both tensors, each read in
                place through its strides; CPU: the torch restatement with the same operation order, bit-identical with the kernel
  BatchRemix    the two streams, the device table and the stage schedule of a training run (``train --stage-steps --batch-sizes
                --patch-sizes --mixup --mixup-after``)

Differences from the reference, on purpose: the draws come from two streams of the feature's own (the reference takes them from
the process-wide ``random`` and torch states; the sampler's streams are untouched here); MixUp is gated by the optimizer step
(``mixup_after``) where the reference gates by ``current_epoch > 5``; file names and indices are not carried.

A CUDA tensor never takes the torch restatement: without libgrl_hip.so the launch raises, as everywhere else in the package.
"""
import bisect
import itertools
import random
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import ops


class RemixPlan(NamedTuple):
    """The draws of one step.  ``idx``: the input samples of the output batch, in order, or None (all of them); ``x0`` / ``y0``:
    first LQ row / column of the window; ``perm`` (int64, (b,)) and ``lam`` (fp32, (b,)): the MixUp partner and weight of every
    output sample, or None and None."""
    idx: Optional[Tuple[int, ...]]
    x0: int
    y0: int
    perm: Optional[torch.Tensor]
    lam: Optional[torch.Tensor]


def stage_of(step: int, stage_steps: Sequence[int]) -> int:
    """The stage of optimizer step ``step`` for stages of ``stage_steps`` steps each: ``bisect_left`` over their cumulative sums,
    the reference's boundary -- step ``n == S_g`` still belongs to stage g.  Past the last stage this is ``len(stage_steps)``."""
    return bisect.bisect_left(list(itertools.accumulate(int(s) for s in stage_steps)), int(step))


def draw_remix(rng: random.Random, gen: Optional[torch.Generator], B: int, P: int, b: int, p: int, mixup: bool) -> RemixPlan:
    """One step's draws, in the reference's order.  Nothing is drawn for a part that is off: ``b == B`` leaves ``rng`` alone as far
    as the sample goes, ``p == P`` as far as the window goes, and without ``mixup`` ``gen`` is not touched."""
    if not (1 <= b <= B and 1 <= p <= P):
        raise ValueError(f"draw_remix: need 1 <= b <= B and 1 <= p <= P, got b={b} B={B} p={p} P={P}")
    idx = tuple(rng.sample(range(B), k=b)) if b < B else None
    x0 = y0 = 0
    if p < P:
        x0 = rng.randrange(P - p + 1)
        y0 = rng.randrange(P - p + 1)
    perm = lam = None
    if mixup:
        perm = torch.randperm(b, generator=gen)
        # Beta(1.2, 1.2).rsample((b, 1)) as torch.distributions draws it: the first component of a Dirichlet sample
        conc = torch.tensor([1.2, 1.2]).expand(b, 1, 1, 2)
        lam = torch._sample_dirichlet(conc, generator=gen).select(-1, 0).reshape(b)
    return RemixPlan(idx, x0, y0, perm, lam)


def _check_plan(plan, B: int, P: int, p: int):
    """(src_a, src_b or None, lam or None) of a valid plan; raises ValueError on one that would read outside the batch."""
    idx, x0, y0, perm, lam = plan
    src_a = list(range(B)) if idx is None else [int(i) for i in idx]
    b = len(src_a)
    if b < 1 or any(not 0 <= i < B for i in src_a):
        raise ValueError(f"batch_remix: idx must name at least one sample of range({B}), got {idx!r}")
    if not 1 <= p <= P:
        raise ValueError(f"batch_remix: the output patch must lie in 1 .. {P}, got {p}")
    if not (0 <= int(x0) <= P - p and 0 <= int(y0) <= P - p):
        raise ValueError(f"batch_remix: the window ({x0}, {y0}) + {p} leaves the patch of side {P}")
    if (perm is None) != (lam is None):
        raise ValueError("batch_remix: perm and lam come together")
    if perm is None:
        return src_a, None, None
    pm = [int(i) for i in perm]
    if sorted(pm) != list(range(b)):
        raise ValueError(f"batch_remix: perm must be a permutation of range({b}), got {pm}")
    lam = torch.as_tensor(lam, dtype=torch.float32).reshape(-1).cpu()
    if lam.numel() != b:
        raise ValueError(f"batch_remix: one lam per output sample ({b}), got {lam.numel()}")
    return src_a, [src_a[i] for i in pm], lam


def plan_table(plan, B: int, P: int, p: int) -> torch.Tensor:
    """The item table of include/grl_hip.h for a (validated) plan: CPU int32 (b, 5) -- src_a, src_b, x0, y0 and the bits of lam."""
    src_a, src_b, lam = _check_plan(plan, B, P, p)
    b = len(src_a)
    t = torch.zeros((b, 5), dtype=torch.int32)
    t[:, 0] = torch.tensor(src_a, dtype=torch.int32)
    t[:, 1] = torch.tensor(src_b if src_b is not None else src_a, dtype=torch.int32)
    t[:, 2], t[:, 3] = int(plan[1]), int(plan[2])
    if lam is not None:
        t[:, 4] = lam.view(torch.int32)
    return t


def batch_remix(lq: torch.Tensor, gt: torch.Tensor, plan, scale: int, out=None, patch: Optional[int] = None, _table=None):
    """``plan`` applied to ``lq`` (B, Cl, P, P) and ``gt`` (B, Cg, sP, sP), fp32: (lq', gt') of (b, Cl, p, p) and (b, Cg, sp, sp),
    contiguous.  ``patch`` is p; without it, that of ``out``, and without both P (no crop).  ``out=(lq_out, gt_out)`` writes into
    given contiguous buffers and returns them.  The plan is validated first: a sample outside the batch, a window outside the patch
    or a ``perm`` that is no permutation raises ValueError and nothing runs.

    CUDA tensors (any strides) take one ``grl_batch_remix`` launch on the current stream; there is no fallback.  CPU tensors take
    ``lam * a + (1 - lam) * b`` in torch, the kernel's operation order: the same bits."""
    for t, what in ((lq, "lq"), (gt, "gt")):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.dtype != torch.float32 or min(t.shape) < 1:
            raise ValueError(f"batch_remix: {what} is a non-empty fp32 (B, C, H, W) tensor")
    scale = int(scale)
    B, Cl, P, _ = lq.shape
    Cg = gt.shape[1]
    if lq.shape[3] != P or scale < 1 or tuple(gt.shape) != (B, Cg, scale * P, scale * P) or gt.device != lq.device:
        raise ValueError(f"batch_remix: lq {tuple(lq.shape)} and gt {tuple(gt.shape)} are no square pair of scale {scale}")
    if patch is None:
        patch = out[0].shape[-1] if out is not None else P
    p = int(patch)
    table = plan_table(plan, B, P, p)                          # validates
    b, mix = table.shape[0], plan[3] is not None
    shapes = ((b, Cl, p, p), (b, Cg, scale * p, scale * p))
    if out is None:
        out = tuple(ops.empty(s, dtype=torch.float32, device=lq.device) for s in shapes)
    for o, s in zip(out, shapes):
        if tuple(o.shape) != s or o.dtype != torch.float32 or o.device != lq.device or not o.is_contiguous():
            raise ValueError(f"batch_remix: out must be contiguous fp32 {s} on {lq.device}, got {tuple(o.shape)} {o.dtype} on {o.device}")
    if lq.is_cuda:
        if _table is None:                                     # an index table: never poisoned (ops.empty), every row is copied below
            _table = torch.empty((b, 5), dtype=torch.int32, device=lq.device)
        _table[:b].copy_(table)
        ops.batch_remix(lq, gt, _table, b, p, scale, mix, out[0], out[1])
        return out[0], out[1]
    x0, y0 = int(plan[1]), int(plan[2])
    src_a, src_b = table[:, 0].long(), table[:, 1].long()
    lam = plan[4].to(torch.float32).reshape(b, 1, 1, 1) if mix else None
    for x, o, k in ((lq, out[0], 1), (gt, out[1], scale)):
        win = x[:, :, x0 * k : (x0 + p) * k, y0 * k : (y0 + p) * k]
        if mix:
            torch.add(lam * win[src_a], (1 - lam) * win[src_b], out=o)
        else:
            o.copy_(win[src_a])
    return out[0], out[1]


def _int_list(v, what: str):
    v = [int(x) for x in v] if v is not None else []
    if any(x < 1 for x in v):
        raise ValueError(f"BatchRemix: {what} holds positive integers, got {v}")
    return v


class BatchRemix:
    """The progressive schedule and MixUp of one training run.  ``batch`` / ``patch``: what the sampler builds (B, P); stage g runs
    ``stage_steps[g]`` optimizer steps on ``batch_sizes[g] <= batch`` samples of LQ side ``patch_sizes[g] <= patch``; three empty
    lists are one stage of (B, P) without an end.  ``mixup``: blend from optimizer step ``mixup_after`` on.

    Holds the two streams -- ``random.Random(seed)`` for sample / x0 / y0, a CPU ``torch.Generator`` seeded ``seed`` for randperm /
    Beta; the sampler's streams are not touched -- and, on a CUDA ``device``, the item table, rewritten in place every step.

        lq, gt = remix(step, lq, gt)                  # or out=(lq_buf, gt_buf): a captured step's static buffers

    A step with nothing to do (full batch, full patch, no MixUp yet) draws nothing and launches nothing: the inputs are returned
    (copied into ``out`` when given)."""

    def __init__(self, batch: int, patch: int, scale: int, stage_steps=None, batch_sizes=None, patch_sizes=None, mixup: bool = False,
                 mixup_after: int = 0, seed: int = 0, device="cpu"):
        self.batch, self.patch, self.scale = int(batch), int(patch), int(scale)
        self.stage_steps = _int_list(stage_steps, "stage_steps")
        self.batch_sizes = _int_list(batch_sizes, "batch_sizes")
        self.patch_sizes = _int_list(patch_sizes, "patch_sizes")
        if not len(self.stage_steps) == len(self.batch_sizes) == len(self.patch_sizes):
            raise ValueError("BatchRemix: stage_steps, batch_sizes and patch_sizes have one entry per stage")
        if any(b > self.batch for b in self.batch_sizes) or any(p > self.patch for p in self.patch_sizes):
            raise ValueError(f"BatchRemix: a stage cannot exceed the loaded batch {self.batch} / patch {self.patch}")
        self.mixup, self.mixup_after = bool(mixup), int(mixup_after)
        if self.mixup_after < 0 or (self.mixup_after and not self.mixup):
            raise ValueError("BatchRemix: mixup_after is a step count and belongs to mixup")
        self.device = torch.device(device)
        self.rng = random.Random(seed)
        self.gen = torch.Generator().manual_seed(int(seed))
        self.table = torch.zeros((self.batch, 5), dtype=torch.int32, device=self.device) if self.device.type == "cuda" else None

    def sizes(self, step: int) -> Tuple[int, int]:
        """(batch, LQ patch) of optimizer step ``step``."""
        if not self.stage_steps:
            return self.batch, self.patch
        g = stage_of(step, self.stage_steps)
        if g >= len(self.stage_steps):
            raise ValueError(f"BatchRemix: step {step} lies past the last stage ({sum(self.stage_steps)} steps in all)")
        return self.batch_sizes[g], self.patch_sizes[g]

    def mixes(self, step: int) -> bool:
        return self.mixup and int(step) >= self.mixup_after

    def draw(self, step: int) -> Tuple[RemixPlan, int]:
        """(plan, p) of ``step``; advances the streams."""
        b, p = self.sizes(step)
        return draw_remix(self.rng, self.gen, self.batch, self.patch, b, p, self.mixes(step)), p

    def __call__(self, step: int, lq: torch.Tensor, gt: torch.Tensor, out=None):
        if tuple(lq.shape[::3]) != (self.batch, self.patch) or lq.shape[2] != self.patch:
            raise ValueError(f"BatchRemix: built for batches of {self.batch} x {self.patch} x {self.patch}, got {tuple(lq.shape)}")
        b, p = self.sizes(step)
        if b == self.batch and p == self.patch and not self.mixes(step):
            if out is None:
                return lq, gt
            out[0].copy_(lq)
            out[1].copy_(gt)
            return out[0], out[1]
        plan, p = self.draw(step)
        return batch_remix(lq, gt, plan, self.scale, out=out, patch=p, _table=self.table)

    def rng_state(self):
        """What a checkpoint keeps to continue the run's draws."""
        return {"draws": self.rng.getstate(), "mixup": self.gen.get_state()}

    def set_rng_state(self, state):
        from .data import _as_rng_state

        self.rng.setstate(_as_rng_state(state["draws"]))
        self.gen.set_state(state["mixup"].cpu())
