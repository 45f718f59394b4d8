"""Times the fused optimizer step with gradient clipping and the weight average (csrc/grad.hip: grl_grad_sqnorm,
grl_grad_clip_finish, the (clip, ema) instance of the AdamW kernel) on the GPU, on the parameter list of ``GRL(**baseline_config(5))``
(GRL-Base: 1390 tensors) with random gradients and no forward.  Three forms alternate in one loop, so all see the same machine:

  (a) plain        FusedAdamW.step()
  (b) fused        FusedAdamW(max_grad_norm=, ema_decay=).step(): norm, finish and one AdamW launch that also moves the average
  (c) torch around clip_grad_norm_(foreach=True) + the plain fused step + torch._foreach_lerp_ on a separate list of averages

Every time is the median over --reps measurements, each the time between two device events around --inner back-to-back steps divided
by --inner (the host's launch work is inside: a form that the host issues slower than the GPU retires pays for it).  ``bytes`` counts
the streams the algorithm needs: 7 x 4 bytes per element for (a) (read g, read and write w, m, v), 3 more for (b) (the norm's read of
g, read and write of the average).  The acceptance condition is (b) faster than (c) in the same run; ``b_faster_than_c`` says it.

Then the captured training step (tools/train_steps.py --graph: GRL-Base, batch 8 x 64 x 64, L1) with both features off and on,
alternately, --graph-rounds times each in processes of their own; no bar is put on the difference, it is recorded.

    python tools/bench_optim.py [--reps 20] [--warmup 3] [--inner 5] [--graph-rounds 2] [--out profiles/optim_bench_line.json]
"""
import argparse
import datetime
import json
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import GRL, FusedAdamW, baseline_config  # noqa: E402

MAX_NORM, DECAY = 1.0, 0.999
KW = dict(lr=2e-4, weight_decay=1e-4)


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


def _params(shapes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ps = [torch.randn(s, device="cuda", generator=g).requires_grad_(True) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device="cuda", generator=g)
    return ps


def optimizer_forms(a):
    shapes = [tuple(p.shape) for p in GRL(**baseline_config(5)).parameters()]
    numel = sum(int(torch.Size(s).numel()) for s in shapes)
    pa, pb, pc = _params(shapes, 1), _params(shapes, 1), _params(shapes, 1)
    oa, ob, oc = FusedAdamW(pa, **KW), FusedAdamW(pb, max_grad_norm=MAX_NORM, ema_decay=DECAY, **KW), FusedAdamW(pc, **KW)
    ema_c = [p.detach().clone() for p in pc]
    weights_c = [p.detach() for p in pc]

    def torch_around():
        torch.nn.utils.clip_grad_norm_(pc, MAX_NORM, foreach=True)
        oc.step()
        torch._foreach_lerp_(ema_c, weights_c, 1.0 - DECAY)

    (ta, amin, amax), (tb, bmin, bmax), (tc, cmin, cmax) = _alternate([oa.step, ob.step, torch_around], a)
    tbs = lambda streams, ms: round(streams * 4 * numel / (ms * 1e-3) / 1e12, 3)
    return {"tensors": len(shapes), "elements": numel, "clip_coef": ob.last_clip_coef(),
            "a_plain_ms": round(ta, 4), "a_min_ms": round(amin, 4), "a_max_ms": round(amax, 4),
            "b_fused_clip_ema_ms": round(tb, 4), "b_min_ms": round(bmin, 4), "b_max_ms": round(bmax, 4),
            "c_torch_around_ms": round(tc, 4), "c_min_ms": round(cmin, 4), "c_max_ms": round(cmax, 4),
            "b_over_a": round(tb / ta, 3), "c_over_b": round(tc / tb, 3), "b_faster_than_c": bool(tb < tc),
            "a_bytes": 7 * 4 * numel, "b_bytes": 10 * 4 * numel, "a_tbs": tbs(7, ta), "b_tbs": tbs(10, tb), "hbm_peak_tbs": a.hbm_tbs}


def captured_step(a):
    """tools/train_steps.py --graph with both features off and on, alternately; a child that fails ends the measurement."""
    script = os.path.join(ROOT, "tools", "train_steps.py")
    times = {"off": [], "on": []}
    for _ in range(a.graph_rounds):
        for which, extra in (("off", []), ("on", ["--clip-grad-norm", str(MAX_NORM), "--ema-decay", str(DECAY)])):
            r = subprocess.run([sys.executable, script, "--graph", "--steps", str(a.graph_steps)] + extra, capture_output=True, text=True,
                               timeout=a.graph_timeout)
            m = re.search(r"([0-9.]+) ms per step", r.stdout)
            if r.returncode != 0 or m is None:
                raise SystemExit(f"train_steps.py ({which}) failed with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            times[which].append(float(m.group(1)))
    med = lambda t: sorted(t)[len(t) // 2]
    return {"graph_step_off_ms": times["off"], "graph_step_on_ms": times["on"],
            "graph_step_delta_ms": round(med(times["on"]) - med(times["off"]), 3), "graph_steps": a.graph_steps}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--graph-rounds", type=int, default=2, help="captured-step measurements per form (0: skip them)")
    ap.add_argument("--graph-steps", type=int, default=10)
    ap.add_argument("--graph-timeout", type=float, default=400.0, help="seconds a captured-step child may take")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM peak the achieved rates stand next to")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench_line.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim needs the GPU")
    line = {"workload": "optimizer step over GRL-Base's parameters (baseline_config(5)): plain / fused clip+EMA / torch around the plain step",
            "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(), "max_grad_norm": MAX_NORM,
            "ema_decay": DECAY, "reps": a.reps, "inner": a.inner}
    line.update(optimizer_forms(a))
    print(json.dumps(line), flush=True)
    with open(a.out, "w") as f:                              # (kept as soon as it is measured; completed below)
        f.write(json.dumps(line) + "\n")
    if a.graph_rounds > 0:
        torch.cuda.empty_cache()
        line.update(captured_step(a))
        print(json.dumps(line), flush=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
