"""Data-parallel training of GRL over the GPUs of a node (replicas + gradient all-reduce).

The reference wraps the model in ``DistributedDataParallel(find_unused_parameters=False)`` through Lightning's DDPStrategy
(tools/trainer.py:135-142): one process per GPU, gradients all-reduced.  On MI355X that all-reduce is RCCL over xGMI
(torch.distributed backend "nccl"); GRL-Base has 77 MB of fp32 gradients in 1390 tensors.  xGMI is point-to-point (7 links per
GPU), ring collectives are per-link bound, so the gradients go out in few, large buckets (>= 25 MB: 3-4 collectives per step,
overlapped with the rest of the backward pass) and, optionally, compressed to bf16 on the wire (half the bytes; the sum is
formed in bf16, the optimizer state stays fp32).

``wrap`` is model-agnostic (it is exercised on CPU with the gloo backend in tests/test_ddp_gloo.py); every parameter of
``grl_image_restoration_amd.GRL`` receives a gradient each step, so find_unused_parameters stays False as in the reference.
"""
from typing import Optional

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel


def bf16_compress_hook(process_group, bucket):
    """Gradient bucket all-reduce in bf16 (mean over ranks), result copied back into the fp32 bucket."""
    group = process_group if process_group is not None else dist.group.WORLD
    world = dist.get_world_size(group)
    buf = bucket.buffer()
    comp = buf.to(torch.bfloat16).div_(world)
    fut = dist.all_reduce(comp, group=group, async_op=True).get_future()

    def done(f):
        buf.copy_(f.value()[0])
        return buf

    return fut.then(done)


def wrap(model: torch.nn.Module, device: Optional[torch.device] = None, bucket_mb: int = 32, compress_bf16: bool = False,
         process_group=None) -> DistributedDataParallel:
    """DistributedDataParallel with the reference's settings (find_unused_parameters=False) and xGMI-sized buckets."""
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("ddp.wrap needs an initialised process group (one process per GPU)")
    ids = [device.index] if device is not None and device.type == "cuda" else None
    ddp = DistributedDataParallel(model, device_ids=ids, find_unused_parameters=False, bucket_cap_mb=bucket_mb,
                                  gradient_as_bucket_view=True, process_group=process_group)
    if compress_bf16:
        ddp.register_comm_hook(process_group, bf16_compress_hook)
    return ddp


def broadcast_module_state(module: torch.nn.Module, group) -> None:
    """Parameters and floating-point buffers of ``module`` <- the group's rank 0 (what DistributedDataParallel does when it wraps a
    module).  Used by the steps that own their gradient all-reduce: train_graph.GraphedTrainStep and gan.GanStep."""
    src = dist.get_global_rank(group, 0) if hasattr(dist, "get_global_rank") else 0
    with torch.no_grad():
        ts = [p for p in module.parameters()] + [b for b in module.buffers() if b.is_floating_point()]
        for dt in {t.dtype for t in ts}:
            same = [t for t in ts if t.dtype == dt]
            flat = torch.cat([t.detach().reshape(-1) for t in same])
            dist.broadcast(flat, src=src, group=group)
            torch._foreach_copy_([t.detach() for t in same], [v.view_as(t) for v, t in zip(flat.split([t.numel() for t in same]), same)])
    torch.autograd.graph.increment_version(list(module.parameters()))
