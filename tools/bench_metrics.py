"""Times metrics.image_metrics(group="restorer_jpeg") on a 3 x 1356 x 2040 pair (DIV2K-val HR size) on the GPU: the HIP kernel
(grl_image_metrics: tile pass + per-image reduction) against the package's torch restatement of the same metrics run on the same
CUDA tensors (five 11x11 depthwise conv2d per plane and element-wise chains).  Warm-up, then the median of --reps runs, each timed
with device events around one call.  Prints one JSON line.

    python tools/bench_metrics.py [--reps 30] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import metrics as M  # noqa: E402


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=[1356, 2040])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics needs the GPU")
    H, W = a.size
    g = torch.Generator().manual_seed(0)
    t = torch.rand(1, 3, H, W, generator=g).cuda()
    r = (t + 0.05 * torch.randn(1, 3, H, W, generator=g).cuda()).contiguous()
    keys = M.GROUPS["restorer_jpeg"]
    hip = lambda: M.image_metrics(r, t, "restorer_jpeg")
    ref = lambda: M._torch_metrics(r, t, keys, 0)
    got, want = hip(), ref()
    err = {k: abs(float(got[k][0]) - float(want[k][0])) for k in keys}
    k_ms = _median_ms(hip, a.reps, a.warmup)
    t_ms = _median_ms(ref, max(5, a.reps // 3), 2)
    bytes_read = 2 * 3 * H * W * 4
    print(json.dumps({"workload": f"image_metrics restorer_jpeg 1x3x{H}x{W} fp32", "device": torch.cuda.get_device_name(0),
                      "hip_ms_median": round(k_ms[0], 4), "hip_ms_min": round(k_ms[1], 4), "hip_ms_max": round(k_ms[2], 4),
                      "torch_ms_median": round(t_ms[0], 3), "torch_ms_min": round(t_ms[1], 3),
                      "speedup": round(t_ms[0] / k_ms[0], 1), "hip_input_GBps": round(bytes_read / (k_ms[0] * 1e-3) / 1e9, 1),
                      "max_abs_diff_vs_torch": max(err.values()), "reps": a.reps}))


if __name__ == "__main__":
    main()
