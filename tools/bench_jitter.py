"""Times the colour jitter of the blind-SR data path on the GPU (csrc/jitter.hip): the ``grl_color_jitter`` entry alone -- its two
launches -- for the workload's 8 items of 3 x 400 x 400 in place with the item tables already on the device, and one
``PatchSampler.next()`` for batch 8, crop 400, scale 4 without and with ``jitter``, alternating in the same run.  First the entry
is checked against the float64 CPU composite of ``jitter.jitter_image`` on small items (all 24 orders) and on one 400 x 400 item.
Kernels: warm-up, then the median over --reps measurements, each the time between two device events around --inner back-to-back
calls, divided by --inner.  Bytes: what the two passes must move -- pass 1 reads the three planes (12 B per pixel), pass 2 reads
and writes them (24 B per pixel) -- over the call's time, against the measured HBM rate of 6.29 TB/s; the 15 MB of crops fit the
256 MB last-level cache, so a rate above HBM's is no error.  The other bound is the launches: the same call on 8 items of one
pixel, timed in the same run, is what two dependent launches cost with nothing to move; the line says which bound the call sits
nearest (the ratio of its time to each).  With --train-step, the captured training step of bench.py's training leg is timed in
the same process and the sampler's difference is given as a share of it.  One JSON line per measurement, printed and written to --out.

    python tools/bench_jitter.py [--reps 20] [--warmup 3] [--inner 10] [--train-step] [--out profiles/jitter_bench_line.json]
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import PatchSampler, PatchStore, jitter as J  # noqa: E402
from tools.bench_degrade import _train_step_ms  # noqa: E402
from tools.bench_metrics import _median_ms  # noqa: E402

N, CROP, SCALE, PATCH = 8, 400, 4, 64
BAR = 4 * 1.165e-6                                     # the kernels' bar of tests/test_gpu_jitter.py
HBM_TBPS = 6.29                                        # measured float4 copy rate of the MI355X (8.0 spec)
BYTES_PER_PIXEL = 12 + 24                              # pass 1 reads three planes, pass 2 reads and writes them


def _image(side_h, side_w, gen):
    y, x = torch.meshgrid(torch.arange(side_h) / side_h, torch.arange(side_w) / side_w, indexing="ij")
    im = torch.stack([x, y, (x + y) / 2]) * 0.8 + 0.1 + 0.1 * (torch.rand(3, side_h, side_w, generator=gen) - 0.5)
    return (im.clamp(0, 1) * 255).round().div(255)


def _check_items(gen):
    """24 small items, one per order, and one of the workload's size, with drawn factors; and their float64 composites."""
    orders = list(itertools.permutations(range(4)))
    imgs = [_image(19, 23, gen) for _ in orders] + [_image(CROP, CROP, gen)]
    params = [(o, *J.draw_jitter(gen)[1:]) for o in orders + [orders[9]]]
    want = [J.jitter_image(im.double(), p) for im, p in zip(imgs, params)]
    return imgs, params, want


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--train-step", action="store_true", help="also time the captured training step of bench.py's training leg")
    ap.add_argument("--train-steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jitter_bench_line.json"))
    a = ap.parse_args(argv)
    gen = torch.Generator().manual_seed(0)
    imgs, params, want = _check_items(gen)
    pixels = N * CROP * CROP
    print(f"bench_jitter: {len(imgs)} check items; the timed call moves {BYTES_PER_PIXEL * pixels / 1e6:.1f} MB over {pixels} pixels", flush=True)
    if not torch.cuda.is_available():
        raise SystemExit("bench_jitter needs the GPU")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    lines = []

    def emit(line):
        line = dict(line, device=name, reps=a.reps, inner=a.inner)
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))

    got = J.color_jitter([im.to(dev) for im in imgs], params)
    err = max(float((g.cpu().double() - w).abs().max()) for g, w in zip(got, want))

    def timed(side):
        """us (median, min, max) of one call on N items of 3 x side x side, in place, lists on the device."""
        crops = torch.stack([_image(side, side, gen) for _ in range(N)]).to(dev)
        lists = J.JitterLists(N, side, dev)
        ps = [J.draw_jitter(gen) for _ in range(N)]
        lists.run_(crops, ps)                          # writes the lists
        flat = crops.view(-1)

        def run():
            for _ in range(a.inner):
                J.hip_color_jitter(flat, flat, lists.rows, lists.factors, lists.partial, lists.means, side, side)

        return [t / a.inner * 1e3 for t in _median_ms(run, a.reps, a.warmup)]

    k, floor = timed(CROP), timed(1)
    hbm_us = BYTES_PER_PIXEL * pixels / (HBM_TBPS * 1e12) * 1e6
    nearest = "launches" if k[0] / floor[0] < k[0] / hbm_us else "HBM"
    emit({"workload": f"grl_color_jitter: {N} items of 3 x {CROP} x {CROP}, in place, one call (two launches)", "pixels": pixels,
          "hip_us_median": round(k[0], 2), "hip_us_min": round(k[1], 2), "hip_us_max": round(k[2], 2),
          "bytes_must_move": BYTES_PER_PIXEL * pixels, "GBps_must_move": round(BYTES_PER_PIXEL * pixels / (k[0] * 1e-6) / 1e9, 1),
          "hbm_floor_us": round(hbm_us, 2), "times_the_hbm_floor": round(k[0] / hbm_us, 2),
          "launch_floor_us_median": round(floor[0], 2), "launch_floor_us_min": round(floor[1], 2), "launch_floor_us_max": round(floor[2], 2),
          "times_the_launch_floor": round(k[0] / floor[0], 2), "nearest_bound": nearest,
          "max_error_vs_float64_cpu": float(f"{err:.3e}"), "error_bar": BAR})

    # the sampler without and with the option, alternating; same seed, so the same crops and plans
    g = np.random.RandomState(0)
    store = PatchStore([g.randint(0, 256, (480, 500, 3)).astype(np.uint8) for _ in range(4)], dev)
    samplers = {key: PatchSampler("sr", store, degrade=True, degrade_crop=CROP, patch=PATCH, scale=SCALE, batch=N, seed=0, jitter=key == "with")
                for key in ("without", "with")}
    ts = {"without": [], "with": []}
    for i in range(a.warmup + a.reps):
        for key, s in samplers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.next()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts[key].append((time.perf_counter() - t0) * 1e3)
    assert samplers["with"].rng.getstate() == samplers["without"].rng.getstate()
    line = {"workload": f"PatchSampler.next(): batch {N}, crop {CROP}, scale {SCALE}, patch {PATCH}, without / with jitter, host work included, "
                        "alternating"}
    for key, v in ts.items():
        v.sort()
        line.update({f"ms_median_{key}": round(v[len(v) // 2], 3), f"ms_min_{key}": round(v[0], 3), f"ms_max_{key}": round(v[-1], 3)})
    line["ms_jitter"] = round(line["ms_median_with"] - line["ms_median_without"], 3)
    if a.train_step:
        line["train_step_ms"] = round(_train_step_ms(a.train_steps), 2)
        line["jitter_share_of_train_step"] = round(line["ms_jitter"] / line["train_step_ms"], 4)
    emit(line)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if err > BAR:
        raise SystemExit(f"bench_jitter: the entry is outside its bar ({err:.3e} > {BAR:.3e})")


if __name__ == "__main__":
    main()
