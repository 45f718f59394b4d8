"""Times tasks.sr_lq on a 1 x 3 x 2160 x 3840 8-bit image at x4 and x2 on the GPU: the HIP kernel (grl_imresize, one launch, the 8-bit
quantisation fused) against the package's float64 torch restatement (gather by the tables, multiply, sum; then tensor_round) run on
the same CUDA tensor.  Warm-up, then the median of --reps runs, each timed with device events around one call.  The effective rate
counts the 4 H W C bytes read and the output bytes written over the kernel's time.  Prints one JSON line.

    python tools/bench_imresize.py [--reps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import tasks as T  # noqa: E402
from tools.bench_metrics import _median_ms  # noqa: E402


def _torch_sr_lq(gt, scale):
    H, W = gt.shape[-2:]
    rows, cols = T.resize_tables(H, H // scale, 1 / scale), T.resize_tables(W, W // scale, 1 / scale)
    return T._round8(T._torch_resize(gt, rows, cols).float())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, nargs=2, default=[2160, 3840])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_imresize needs the GPU")
    H, W = a.size
    gt = (torch.randint(0, 256, (1, 3, H, W), generator=torch.Generator().manual_seed(0)).float() / 255).cuda()
    line = {"workload": f"sr_lq 1x3x{H}x{W} fp32 (MATLAB bicubic, 8-bit quantised)", "device": torch.cuda.get_device_name(0), "reps": a.reps}
    for s in (4, 2):
        hip = lambda: T.sr_lq(gt, s)[0]
        ref = lambda: _torch_sr_lq(T.modcrop(gt, s), s)
        got, want = hip(), ref()
        k_ms = _median_ms(hip, a.reps, a.warmup)
        t_ms = _median_ms(ref, max(5, a.reps // 5), 2)
        moved = 4 * 3 * (H * W + got.shape[-2] * got.shape[-1])
        line[f"x{s}"] = {"hip_ms_median": round(k_ms[0], 4), "hip_ms_min": round(k_ms[1], 4), "hip_ms_max": round(k_ms[2], 4),
                        "torch_ms_median": round(t_ms[0], 3), "torch_ms_min": round(t_ms[1], 3), "speedup": round(t_ms[0] / k_ms[0], 1),
                        "hip_effective_TBps": round(moved / (k_ms[0] * 1e-3) / 1e12, 3),
                        "levels_differing_from_torch": int(((got - want).abs() > 0.5 / 255).sum())}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
