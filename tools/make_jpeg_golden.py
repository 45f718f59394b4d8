"""Writes tests/golden/tasks/jpeg_roundtrip.npz: 8-bit inputs and what Pillow's bundled libjpeg-turbo decodes after
``Image.save(format="JPEG", quality=q)`` -- the library and the defaults (4:2:0, JDCT_ISLOW, baseline tables, fancy upsampling) that
OpenCV's ``cv2.imencode`` / ``cv2.imdecode`` of data/datasets/restoration_jpeg.py:62-79 run with.  ``tasks.jpeg_roundtrip`` has to
reproduce every byte (tests/test_jpeg.py on the CPU, tests/test_gpu_jpeg.py on the device).

Every case is a batch of three images of one size with three qualities, RGB (c3) or gray (c1), at the sizes that exercise the edge
rules: 1x1 (everything is padding), 8x8 (no padding), 9x17 and 37x53 (odd sides), 24x31 (H even, ceil(H/2) no multiple of 8),
50x16 (the same with two chroma block rows), 64x64 (several blocks per plane), and 20x4 (at most two chroma columns: libjpeg's plain
upsampler).  Batch "a" is uniform noise, a ramp and 0/255 binary noise at qualities 10, 40, 75; batch "b" is the 1-pixel 0/255
checkerboard at quality 100 and at quality 1 (the largest coefficients and the coarsest steps) and the 8-pixel one at quality 50.

    python tools/make_jpeg_golden.py

Refuses to run unless Pillow is built on libjpeg-turbo."""
import io
import json
import os

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tasks", "jpeg_roundtrip.npz")
SIZES = [(1, 1), (8, 8), (9, 17), (24, 31), (50, 16), (37, 53), (64, 64), (20, 4)]


def pillow_roundtrip(img: np.ndarray, quality: int) -> np.ndarray:
    """(H, W, C) uint8, C = 1 or 3 -> the decoded (H, W, C) uint8."""
    buf = io.BytesIO()
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img).save(buf, format="JPEG", quality=int(quality))
    buf.seek(0)
    out = np.asarray(Image.open(buf))
    return out[:, :, None] if out.ndim == 2 else out


def pattern(kind: str, H: int, W: int, C: int, rng) -> np.ndarray:
    """(H, W, C) uint8: noise, ramp, binary (0 / 255 noise), checker1 / checker8 (0 / 255 checkerboards of 1 and 8 pixels)."""
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":
        a = rng.randint(0, 256, (H, W, C))
    elif kind == "binary":
        a = rng.randint(0, 2, (H, W, C)) * 255
    elif kind == "ramp":
        a = np.stack([(3 * yy + 2 * xx + 40 * c) % 256 for c in range(C)], 2)
    elif kind in ("checker1", "checker8"):
        s = int(kind[-1])
        a = np.repeat((((yy // s + xx // s) % 2) * 255)[:, :, None], C, 2)
    else:
        raise ValueError(kind)
    return a.astype(np.uint8)


BATCHES = {"a": (("noise", "ramp", "binary"), (10, 40, 75)), "b": (("checker1", "checker1", "checker8"), (100, 1, 50))}


def main():
    if not features.check("libjpeg_turbo"):
        raise SystemExit("make_jpeg_golden: this Pillow is not built on libjpeg-turbo; the fixture must come from that library")
    rng = np.random.RandomState(20)
    arrays, cases = {}, []
    for H, W in SIZES:
        for C in (3, 1):
            for b, (kinds, quals) in BATCHES.items():
                name = f"{H}x{W}_c{C}_{b}"
                x = np.stack([pattern(k, H, W, C, rng) for k in kinds])
                y = np.stack([pillow_roundtrip(im, q) for im, q in zip(x, quals)])
                arrays[name + "__x"] = np.ascontiguousarray(x.transpose(0, 3, 1, 2))          # (3, C, H, W) uint8
                arrays[name + "__y"] = np.ascontiguousarray(y.transpose(0, 3, 1, 2))
                cases.append({"name": name, "size": [H, W], "channels": C, "kinds": list(kinds), "quality": list(quals)})
    meta = {"cases": cases, "libjpeg_turbo": features.version("libjpeg_turbo"), "pillow": features.version("pil")}
    np.savez_compressed(OUT, meta=json.dumps(meta), **arrays)
    print(f"wrote {OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
