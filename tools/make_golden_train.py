"""Records tests/golden/train/lr_schedule.npz: the learning rates of the reference's MultiStepLRWarmup (optim/multi_steplr.py) stepped
once per iteration, for base lr 2e-4, milestones 30+50+65+70+75, gamma 0.5, warm-up 10 from 1e-5, 80 steps.  Numbers only.

    python tools/make_golden_train.py [--reference /path/to/reference]      (default: GRL_REFERENCE_ROOT, as for oracle/refshim.py)
"""
import argparse
import importlib.util
import os
import warnings

import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.refshim import REFERENCE_ROOT  # noqa: E402  (where the reference tree is; nothing else is used)
CASE = dict(base_lr=2e-4, milestones=[30, 50, 65, 70, 75], gamma=0.5, warmup_iter=10, warmup_init_lr=1e-5, steps=80)


def reference_schedule(reference: str, base_lr, milestones, gamma, warmup_iter, warmup_init_lr, steps):
    """lr of optimizer steps 0 .. steps - 1 under the reference's scheduler class, loaded from its file."""
    spec = importlib.util.spec_from_file_location("ref_multi_steplr", os.path.join(reference, "optim", "multi_steplr.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    class Sched(mod.MultiStepLRWarmup):
        """The reference's get_lr under its own constructor's assignments; the constructor itself hands MultiStepLR a positional
        ``verbose`` that recent torch releases no longer take."""

        def __init__(self, optimizer):
            self.warmup_iter, self.warmup_init_lr = warmup_iter, warmup_init_lr
            torch.optim.lr_scheduler.MultiStepLR.__init__(self, optimizer, list(milestones), gamma)

    p = [torch.nn.Parameter(torch.zeros(1))]
    opt = torch.optim.AdamW(p, base_lr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = Sched(opt)
        lrs = []
        for _ in range(steps):
            lrs.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
    return lrs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=REFERENCE_ROOT, help="the reference tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "train", "lr_schedule.npz"))
    a = ap.parse_args()
    lrs = reference_schedule(a.reference, **CASE)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez(a.out, lr=np.asarray(lrs, dtype=np.float64), milestones=np.asarray(CASE["milestones"]), base_lr=CASE["base_lr"],
             gamma=CASE["gamma"], warmup_iter=CASE["warmup_iter"], warmup_init_lr=CASE["warmup_init_lr"])
    print(a.out, lrs[:3], lrs[9:12], lrs[-1])


if __name__ == "__main__":
    main()
