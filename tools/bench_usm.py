"""Times tasks.usm_sharp (grl_usm_sharp: the blur / mask pass and the blend pass, 51 taps) on the GPU at a (1, 3, 1356, 2040)
validation image and a (1, 3, 512, 512) one, plain and with ``quantise``, on random 8-bit data.  Warm-up, then the median over --reps
measurements, each the time between two device events around --inner back-to-back calls, divided by --inner (a small launch pair is
shorter than the gap between two host calls).  ``gbs_algorithmic`` sets the time against the bytes the operation has to move: ``x``
read once and ``out`` written once (the kernels also write and re-read blur and mask and re-read ``x``; that traffic is theirs).  For
scale, the same image through ``scipy.ndimage.correlate1d`` in fp32 on the host (two separable blurs and the blend, what the
reference's ``cv2.GaussianBlur`` calls amount to), without the host-to-device copy that follows it there.  The GPU result is checked
first against the CPU path: blur within 2 gamma_51, and the result within 2 gamma_51 + 4 u wherever the two masks agree around a
pixel (tests/test_usm.py derives the bounds).  One JSON line per case, printed and written to --out.

    python tools/bench_usm.py [--reps 30] [--warmup 5] [--inner 20] [--out profiles/usm_bench_line.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import tasks as T  # noqa: E402
from tools.bench_metrics import _median_ms  # noqa: E402

U24 = 2.0 ** -24
GAMMA51 = 51 * U24 / (1 - 51 * U24)


def _scipy_ms(x, taps, reps):
    from scipy.ndimage import correlate1d

    G = lambda a: correlate1d(correlate1d(a, taps, axis=-1, mode="mirror"), taps, axis=-2, mode="mirror")
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = x - G(x)
        soft = G((np.abs(res) * 255 > 10).astype(np.float32))
        _ = soft * np.clip(x + 0.5 * res, 0, 1) + (1 - soft) * x
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def _check(x):
    """(max blur error, max result error over the pixels with no mask disagreement within the kernel's reach, mask disagreements)."""
    out, blur, mask = T.usm_sharp(x.cuda(), parts=True)
    wout, wblur, wmask = T.usm_sharp(x, parts=True)
    eb = float((blur.double().cpu() - wblur).abs().max())
    differ = (mask.cpu().double() != wmask).float()
    reach = torch.nn.functional.max_pool2d(differ, 51, 1, 25) > 0
    eo = float((out.double().cpu() - wout.double()).abs()[~reach].max())
    return eb, eo, int(differ.sum())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "usm_bench_line.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_usm needs the GPU")
    lines = []
    g = torch.Generator().manual_seed(0)
    taps = T.usm_taps().cuda()
    for shape in ((1, 3, 1356, 2040), (1, 3, 512, 512)):
        x = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).float().div(255)
        eb, eo, flips = _check(x)
        ok = eb <= 2 * GAMMA51 and eo <= 2 * GAMMA51 + 4.5 * U24
        xg = x.cuda()
        host_ms = _scipy_ms(x.numpy(), T.usm_taps().numpy(), max(3, a.reps // 10))
        for quantise in (False, True):
            out = torch.empty_like(xg)
            hip = lambda: [T.hip_usm(xg, taps, quantise=quantise, out=out) for _ in range(a.inner)]
            k_ms = [t / a.inner for t in _median_ms(hip, a.reps, a.warmup)]
            line = {"workload": f"usm_sharp {'x'.join(map(str, shape))} fp32, 51 taps" + (", quantise" if quantise else ""),
                    "device": torch.cuda.get_device_name(0), "hip_us_median": round(k_ms[0] * 1e3, 2),
                    "hip_us_min": round(k_ms[1] * 1e3, 2), "hip_us_max": round(k_ms[2] * 1e3, 2),
                    "gbs_algorithmic": round(2 * x.numel() * 4 / (k_ms[0] * 1e-3) / 1e9, 1),
                    "scipy_fp32_host_ms_median": round(host_ms, 1), "max_blur_error_vs_cpu": eb, "max_out_error_vs_cpu": eo,
                    "mask_disagreements": flips, "within_derived_tolerance": bool(ok), "reps": a.reps, "inner": a.inner}
            print(json.dumps(line), flush=True)
            lines.append(json.dumps(line))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not all(json.loads(l)["within_derived_tolerance"] for l in lines):
        raise SystemExit("bench_usm: the GPU result is outside the derived tolerance")


if __name__ == "__main__":
    main()
