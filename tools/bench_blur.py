"""Times tasks.blur (grl_blur_depthwise, one launch) on the GPU at the two shapes of the deblurring task -- a (1, 3, 720, 1280) image
with zero padding (validation) and an (8, 3, 64 + K - 1, 64 + K - 1) batch over the valid region with the centre crop (training) --
for K = 25 (the Gaussian) and K = 13 (the smallest Levin09 kernel), on random 8-bit data with a noise operand.  Next to each, what a
user would write without the kernel: ``torch.nn.functional.conv2d(x, taps repeated over the channels, groups=3)`` plus the noise
(and the two crops for training) on the same device.  Warm-up, then the median over --reps measurements, each the time between two
device events around --inner back-to-back calls, divided by --inner (a single small launch is shorter than the gap between two
host calls).  The share of the fp32 vector peak counts 2 K^2 FLOP per output value against --peak-tflops.  One JSON line per case.

    python tools/bench_blur.py [--reps 30] [--warmup 5] [--inner 20]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import tasks as T  # noqa: E402
from tools.bench_metrics import _median_ms  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--peak-tflops", type=float, default=157.3, help="fp32 vector peak of the device (MI355X: 157.3)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_blur needs the GPU")
    g = torch.Generator().manual_seed(0)
    for K in (25, 13):
        k = torch.rand(K, K, generator=g, dtype=torch.float64)
        taps = T.blur_taps(k / k.sum()).cuda()
        w3 = taps.view(1, 1, K, K).repeat(3, 1, 1, 1)
        for pad, shape in (("same", (1, 3, 720, 1280)), ("valid", (8, 3, 64 + K - 1, 64 + K - 1))):
            x = (torch.randint(0, 256, shape, generator=g).float() / 255).cuda()
            b = K // 2
            oshape = shape if pad == "same" else shape[:2] + (64, 64)
            noise = (torch.randn(oshape, generator=g) * (2 / 255)).cuda()
            if pad == "same":
                hip = lambda: T.blur(x, taps, "same", add=noise)
                ref = lambda: noise + F.conv2d(x, w3, groups=3, padding=b)
                got, want = hip(), ref()
            else:
                hip = lambda: T.blur(x, taps, "valid", add=noise, want_center=True)
                ref = lambda: (noise + F.conv2d(x, w3, groups=3), x[..., b:-b, b:-b].contiguous())
                got, want = hip()[0], ref()[0]
            err = float((got - want).abs().max())
            many = lambda fn: (lambda: [fn() for _ in range(a.inner)])
            k_ms = [t / a.inner for t in _median_ms(many(hip), a.reps, a.warmup)]
            t_ms = [t / a.inner for t in _median_ms(many(ref), a.reps, a.warmup)]
            flop = 2.0 * K * K * got.numel()
            print(json.dumps({"workload": f"blur {pad} {'x'.join(map(str, shape))} fp32, K {K}", "device": torch.cuda.get_device_name(0),
                              "hip_us_median": round(k_ms[0] * 1e3, 2), "hip_us_min": round(k_ms[1] * 1e3, 2),
                              "torch_us_median": round(t_ms[0] * 1e3, 2), "torch_us_min": round(t_ms[1] * 1e3, 2),
                              "speedup": round(t_ms[0] / k_ms[0], 2), "hip_tflops": round(flop / (k_ms[0] * 1e-3) / 1e12, 2),
                              "share_of_fp32_peak": round(flop / (k_ms[0] * 1e-3) / 1e12 / a.peak_tflops, 3),
                              "max_abs_diff_to_torch": err, "reps": a.reps, "inner": a.inner}), flush=True)


if __name__ == "__main__":
    main()
