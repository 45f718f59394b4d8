"""Writes tests/golden/tasks/remix.npz: MixUp of the UNMODIFIED reference on a few small batches.

``MixUp_AUG`` (utils/dataset_utils.py:43-60) is imported from the reference's tree (GRL_REFERENCE_ROOT, as for oracle/refshim.py).
Its ``aug`` moves ``lam`` to the GPU with ``Tensor.cuda``; that method is patched to return ``self`` for the call (and records the
tensor it was called on: that is ``lam``), and ``torch.randperm`` is wrapped to record the permutation.  Per case k the global torch
generator is seeded with ``seed[k]`` and ``aug(lq, gt)`` is called once, as engines/base.py:169 calls it.  Arrays per case:
``lq{k}`` / ``gt{k}`` (inputs, fp32), ``perm{k}`` (int64), ``lam{k}`` (fp32, (b,)), ``lq_out{k}`` / ``gt_out{k}``; ``seed`` holds the
seeds.  The cases cover unequal channel counts (6 / 3), one channel, scales 1, 2 and 3 and non-square images.

The archive is written with fixed time stamps: the same reference tree and the same torch give the same bytes.

    python tools/make_golden_remix.py [--reference DIR] [--out tests/golden/tasks]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402
from tools.make_golden_image8 import write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tasks")
CASES = [(0, (4, 3, 5, 7), (4, 3, 10, 14)), (1, (2, 6, 4, 4), (2, 3, 4, 4)), (7, (5, 1, 3, 3), (5, 1, 9, 9)), (2026, (1, 3, 2, 2), (1, 3, 2, 2))]


def build(mixup_cls):
    arrays, seen = {"seed": np.array([c[0] for c in CASES], dtype=np.int64)}, {}
    real_cuda, real_randperm = torch.Tensor.cuda, torch.randperm

    def cuda(self, *args, **kwargs):
        seen["lam"] = self.clone()
        return self

    def randperm(*args, **kwargs):
        seen["perm"] = real_randperm(*args, **kwargs)
        return seen["perm"]

    torch.Tensor.cuda, torch.randperm = cuda, randperm
    try:
        for k, (seed, lq_shape, gt_shape) in enumerate(CASES):
            g = torch.Generator().manual_seed(1000 + seed)
            lq, gt = torch.randn(lq_shape, generator=g), torch.randn(gt_shape, generator=g)
            torch.manual_seed(seed)
            lq_out, gt_out = mixup_cls().aug(lq, gt)
            arrays.update({f"lq{k}": lq.numpy(), f"gt{k}": gt.numpy(), f"perm{k}": seen["perm"].numpy(),
                           f"lam{k}": seen["lam"].reshape(-1).numpy(), f"lq_out{k}": lq_out.numpy(), f"gt_out{k}": gt_out.numpy()})
    finally:
        torch.Tensor.cuda, torch.randperm = real_cuda, real_randperm
    meta = {"cases": len(CASES), "torch": torch.__version__.split("+")[0],
            "source": "utils/dataset_utils.py:43-60 MixUp_AUG.aug(input_, target), torch.manual_seed(seed) before each call"}
    return arrays, meta


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=refshim.REFERENCE_ROOT)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args(argv)
    if a.reference not in sys.path:
        sys.path.insert(0, a.reference)
    from utils.dataset_utils import MixUp_AUG  # the reference's

    arrays, meta = build(MixUp_AUG)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "remix.npz")
    write_npz(path, dict(meta=np.array(json.dumps(meta)), **arrays))
    print(f"wrote {path}: {len(CASES)} MixUp cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
