"""Times tasks.jpeg_roundtrip (grl_jpeg_roundtrip: the block pass and the merge pass) on the GPU at the two shapes of the JPEG
artifact-removal task -- an (8, 3, 288, 288) batch of training patches with a quality per sample (jpeg/grl/grl_p288.yaml) and a
(1, 3, 1356, 2040) validation image at quality 10 -- on random 8-bit data.  Next to each, for scale, what the reference does instead:
the host library's encode + decode of the same images one after the other (Pillow's libjpeg-turbo here; the reference calls the
same library through OpenCV), without the host-to-device copy that follows it there.  Warm-up, then the median over --reps
measurements, each the time between two device events around --inner back-to-back calls, divided by --inner (a small launch pair is
shorter than the gap between two host calls).  The output is checked against the CPU restatement first.  One JSON line per case,
printed and written to --out; ``share_of_train_step`` sets the training-shape time against --train-step-ms (the captured training
step of DESIGN.md, 89.3 ms).

    python tools/bench_jpeg.py [--reps 30] [--warmup 5] [--inner 20] [--out profiles/jpeg_bench_line.json]
"""
import argparse
import io
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


def _pillow_ms(x8, quality, reps):
    """Median wall time of encoding and decoding the batch image by image on the host."""
    from PIL import Image

    imgs = [Image.fromarray(np.ascontiguousarray(im.transpose(1, 2, 0))) for im in x8]
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for im, q in zip(imgs, quality):
            buf = io.BytesIO()
            im.save(buf, format="JPEG", quality=int(q))
            buf.seek(0)
            np.asarray(Image.open(buf))
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--train-step-ms", type=float, default=89.3, help="the captured training step the patch batch feeds (DESIGN.md)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench_line.json"))
    a = ap.parse_args(argv)
    lines = []
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg needs the GPU")
    g = torch.Generator().manual_seed(0)
    for what, shape, quality in (("train", (8, 3, 288, 288), [10, 14, 19, 23, 27, 32, 36, 40]), ("val", (1, 3, 1356, 2040), [10])):
        x8 = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        x = (x8.float() / 255).cuda()
        q = torch.tensor(quality, dtype=torch.int32, device="cuda")
        exact = bool(torch.equal(T.jpeg_roundtrip(x, q).cpu(), T._torch_jpeg(x.cpu(), q.cpu())))
        hip = lambda: [T.hip_jpeg(x, q) for _ in range(a.inner)]
        k_ms = [t / a.inner for t in _median_ms(hip, a.reps, a.warmup)]
        p_ms = _pillow_ms(x8.numpy(), quality, max(3, a.reps // 6))
        line = {"workload": f"jpeg_roundtrip {what} {'x'.join(map(str, shape))} fp32, quality {quality[0]}..{quality[-1]}",
                "device": torch.cuda.get_device_name(0), "hip_us_median": round(k_ms[0] * 1e3, 2), "hip_us_min": round(k_ms[1] * 1e3, 2),
                "hip_us_max": round(k_ms[2] * 1e3, 2), "pillow_host_ms_median": round(p_ms, 3),
                "megapixels_per_s": round(shape[0] * shape[2] * shape[3] / (k_ms[0] * 1e-3) / 1e6, 1),
                "equals_cpu_restatement": exact, "reps": a.reps, "inner": a.inner}
        if what == "train":
            line["train_step_ms"] = a.train_step_ms
            line["share_of_train_step"] = round(k_ms[0] / a.train_step_ms, 5)
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
