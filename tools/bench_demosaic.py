"""Times tasks.demosaic_gt on a 1 x 3 x 2160 x 3840 8-bit image on the GPU: the HIP kernel (grl_demosaic_matlab, one launch that reads
the RGB image on the RGGB lattice) against the package's float64 torch restatement of dm_matlab run on the same CUDA tensors (mosaic,
reflect pad, four 5x5 convolutions, channel fill).  Warm-up, then the median of --reps runs, each timed with device events around
one call.  The effective rate counts 16 B read and 48 B written per packed 2 x 2 cell.  Prints one JSON line.

    python tools/bench_demosaic.py [--reps 50] [--warmup 10]
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, nargs=2, default=[2160, 3840])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_demosaic needs the GPU")
    H, W = a.size
    g = torch.Generator().manual_seed(0)
    rgb = (torch.randint(0, 256, (1, 3, H, W), generator=g).float() / 255).cuda()
    hip = lambda: T.demosaic_gt(rgb)
    ref = lambda: T._torch_dm_matlab(T.mosaic_bayer(rgb))
    got, want = hip(), ref()
    bitwise = bool(torch.equal(got, want))
    k_ms = _median_ms(hip, a.reps, a.warmup)
    t_ms = _median_ms(ref, max(5, a.reps // 5), 2)
    cells = (H // 2) * (W // 2)
    print(json.dumps({"workload": f"demosaic_gt 1x3x{H}x{W} fp32 (dm_matlab)", "device": torch.cuda.get_device_name(0),
                      "hip_ms_median": round(k_ms[0], 4), "hip_ms_min": round(k_ms[1], 4), "hip_ms_max": round(k_ms[2], 4),
                      "torch_ms_median": round(t_ms[0], 3), "torch_ms_min": round(t_ms[1], 3),
                      "speedup": round(t_ms[0] / k_ms[0], 1), "hip_effective_TBps": round(64 * cells / (k_ms[0] * 1e-3) / 1e12, 3),
                      "bitwise_equal_to_torch": bitwise, "reps": a.reps}))


if __name__ == "__main__":
    main()
