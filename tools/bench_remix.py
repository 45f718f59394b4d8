"""Times ``grl_batch_remix`` (csrc/remix.hip: mini-batch, mini-patch and MixUp of lq and gt in one launch) on the GPU against the
torch restatement it replaces.  One JSON line per workload, printed and written to --out:

  progressive+mixup   8 x 3 x 256 x 256 -> 4 x 3 x 128 x 128 at scale 1: selection, crop and blend
  mixup               8 x 3 x 64 x 64 LQ / x4 GT, full batch and patch: the blend alone (the training shape of bench.py)
  progressive         8 x 3 x 64 x 64 LQ / x4 GT -> 4 x 3 x 32 x 32 / x4: selection and crop alone (mix == 0: a gather)

Two pairs of figures per workload.  ``launch``: the kernel with its item table already on the device against the torch chain with
its index tensors and ``lam`` already on the device -- what the GPU and the launches cost.  ``step``: what a training step pays from
the host's plan on, ``remix.batch_remix(..., _table=table)`` (plan check, table upload, launch) against the chain with its uploads.
Every time is the median over --reps measurements, each the time between two device events around --inner back-to-back calls divided
by --inner; kernel and restatement alternate in the same loop, so both see the same machine.  ``algorithm_bytes`` counts every source
value the outputs need once (twice with MixUp: as itself and as a partner) and every output value once.  The kernel's outputs are
compared with the CPU restatement first (``torch.equal``).

    python tools/bench_remix.py [--reps 30] [--warmup 5] [--inner 20] [--out profiles/remix_bench_line.json]
"""
import argparse
import json
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import ops, remix as R  # noqa: E402


def torch_chain(lq, gt, src_a, src_b, lam, x0, y0, p, s):
    """The engine's own sequence on the device: index, slice, index again for the partner, blend (engines/base.py:144-169)."""
    out = []
    for x, k in ((lq, 1), (gt, s)):
        a = x[src_a][:, :, x0 * k : (x0 + p) * k, y0 * k : (y0 + p) * k]
        out.append(lam * a + (1 - lam) * a[src_b] if lam is not None else a.contiguous())
    return out


def _events_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _alternate(fns, a):
    for _ in range(a.warmup):
        for f in fns:
            _events_ms(f, a.inner)
    ts = [[] for _ in fns]
    for _ in range(a.reps):
        for t, f in zip(ts, fns):
            t.append(_events_ms(f, a.inner))
    return [(sorted(t)[len(t) // 2], min(t), max(t)) for t in ts]


def line(a, what, B, C, P, s, b, p, mixup, seed):
    g = torch.Generator().manual_seed(seed)
    lq, gt = torch.rand(B, C, P, P, generator=g), torch.rand(B, C, s * P, s * P, generator=g)
    plan = R.draw_remix(random.Random(seed), torch.Generator().manual_seed(seed), B, P, b, p, mixup)
    want = R.batch_remix(lq, gt, plan, s, patch=p)
    lq, gt = lq.cuda(), gt.cuda()
    table = torch.zeros((B, 5), dtype=torch.int32, device="cuda")
    outs = (torch.empty(b, C, p, p, device="cuda"), torch.empty(b, C, s * p, s * p, device="cuda"))
    got = R.batch_remix(lq, gt, plan, s, out=outs, patch=p, _table=table)
    exact = bool(torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1]))

    idx = list(plan.idx) if plan.idx is not None else list(range(B))

    def uploads():
        return (torch.tensor(idx).cuda(), plan.perm.cuda() if mixup else None, plan.lam.view(-1, 1, 1, 1).cuda() if mixup else None)

    src_a, perm, lam = uploads()
    chain = torch_chain(lq, gt, src_a, perm, lam, plan.x0, plan.y0, p, s)
    same = bool(torch.equal(chain[0], got[0]) and torch.equal(chain[1], got[1]))

    def chain_step():
        sa, pm, lm = uploads()
        return torch_chain(lq, gt, sa, pm, lm, plan.x0, plan.y0, p, s)

    (h, hmin, hmax), (c, cmin, cmax), (hs, _, _), (cs, _, _) = _alternate([
        lambda: ops.batch_remix(lq, gt, table, b, p, s, mixup, outs[0], outs[1]),
        lambda: torch_chain(lq, gt, src_a, perm, lam, plan.x0, plan.y0, p, s),
        lambda: R.batch_remix(lq, gt, plan, s, out=outs, patch=p, _table=table),
        chain_step], a)
    need = (outs[0].numel() + outs[1].numel()) * 4 * (3 if mixup else 2)
    return {"workload": f"{what}: {B}x{C}x{P}x{P} / x{s} -> {b}x{C}x{p}x{p} / x{s}, mixup {'on' if mixup else 'off'}",
            "device": torch.cuda.get_device_name(0),
            "hip_us_median": round(h * 1e3, 2), "hip_us_min": round(hmin * 1e3, 2), "hip_us_max": round(hmax * 1e3, 2),
            "torch_us_median": round(c * 1e3, 2), "torch_us_min": round(cmin * 1e3, 2), "torch_us_max": round(cmax * 1e3, 2),
            "torch_over_hip": round(c / h, 2), "hip_step_us_median": round(hs * 1e3, 2), "torch_step_us_median": round(cs * 1e3, 2),
            "algorithm_bytes": need, "algorithm_tbs": round(need / (h * 1e-3) / 1e12, 3), "hbm_peak_tbs": a.hbm_tbs,
            "hbm_floor_us": round(need / (a.hbm_tbs * 1e12) * 1e6, 2), "reps": a.reps, "inner": a.inner,
            "equals_cpu_restatement": exact, "equals_torch_chain": same}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM peak the floor is taken of")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remix_bench_line.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_remix needs the GPU")
    lines = []
    for args in (("progressive+mixup", 8, 3, 256, 1, 4, 128, True, 1), ("mixup", 8, 3, 64, 4, 8, 64, True, 2),
                 ("progressive", 8, 3, 64, 4, 4, 32, False, 3), ("one pixel", 1, 3, 1, 1, 1, 1, True, 4)):
        ln = line(a, *args)
        print(json.dumps(ln), flush=True)                             # each line is printed and kept as soon as it is measured
        lines.append(json.dumps(ln))
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
