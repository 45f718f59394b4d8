"""Writes tests/golden/tasks/usm.npz: the yardstick of ``tasks.usm_sharp`` / ``grl_usm_sharp``.

OpenCV is not available where this project is built and tested, so the file does not hold ``cv2.GaussianBlur`` results and bit
equality with OpenCV's summation order is not claimed anywhere.  The yardstick is a float64 restatement of
utils/utils_bsr/utils_usm.py:34-60 that shares no code with the package (this tool imports nothing of it):
``scipy.ndimage.correlate1d(mode="mirror")`` along both axes -- ``mirror`` is cv2's BORDER_REFLECT_101, repeated reflection
included -- with the taps of ``cv2.getGaussianKernel(51, 0)`` written out from their closed form (sigma = 0.3 ((51 - 1) / 2 - 1) + 0.8
= 8).  Both inputs are the float64 of the fp32 values a kernel sees: ``float64(float32(k / 255))`` for the 8-bit image and
``float64(float32(tap))``, so neither input rounding nor tap rounding is part of an error measured against the file.

Cases (images: a few smooth blobs plus two-sided noise, uint8):
  A  (1, 1, 130, 150)   crosses tile boundaries both ways
  B  (1, 3, 70, 90)     sides that are multiples of nothing
  C  (2, 1, 33, 64)     sides between K / 2 and K; batch indexing
  D  (1, 3, 20, 100)    H < 26: repeated reflection
  E1 (1, 1, 5, 3), E2 (1, 1, 1, 7)   degenerate sides

Per case the file holds
  <case>__x           uint8 (N, C, H, W)
  <case>__blur_q31, <case>__out_q31
                      the float64 blur and result at the DECIDED threshold as uint32 fixed point: ``rint(v * 2^31)``, i.e. the float64
                      value to within 2^-32 = 2.4e-10, four orders below the tightest tolerance taken against it.  (Full float64 of the
                      two arrays alone is 780 KB at these shapes; the fixture is kept under 512 KB.)
  <case>__mask        the float64 0 / 1 mask at the decided threshold, ``np.packbits`` of the flattened array
  <case>__out8        uint8: ``rint(clip(out, 0, 1) * 255)`` of the float64 result (half to even)
  <case>__undecided   ``np.packbits``: pixels whose ``|res| * 255`` lies within ``margin`` of the default threshold 10
and ``taps`` (fp32, 51) and a JSON ``meta``: per case the decided threshold (near 10, in the middle of the widest gap of
``|res| * 255`` between 9 and 11), the mask fraction, U = the number of undecided pixels, the share of pixels whose ``255 * out`` lies
within 1.8e-3 of a half-integer; ``margin`` = 255 * 2 gamma_51 + 1e-5 with gamma_n = n u / (1 - n u), u = 2^-24.

Asserted here: every decided threshold is at least 0.01 away from every value; the mask fraction of A - D is in 0.2 .. 0.8; at most
0.1 % of the pixels are undecided at threshold 10; at most 1 % are near a half-integer level.

    python tools/make_golden_usm.py [--out tests/golden/tasks]
"""
import argparse
import json
import os

import numpy as np
from scipy.ndimage import correlate1d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tasks")

K, SIGMA, WEIGHT, DEFAULT_THRESHOLD = 51, 8.0, 0.5, 10.0
U24 = 2.0 ** -24
GAMMA51 = 51 * U24 / (1 - 51 * U24)
MARGIN = 255 * 2 * GAMMA51 + 1e-5
HALF_BAND = 1.8e-3
NOISE = 0.4                       # share of the pixels that take a large step
CASES = [("A", (1, 1, 130, 150)), ("B", (1, 3, 70, 90)), ("C", (2, 1, 33, 64)), ("D", (1, 3, 20, 100)), ("E1", (1, 1, 5, 3)),
         ("E2", (1, 1, 1, 7))]


def taps32():
    i = np.arange(K, dtype=np.float64) - (K - 1) / 2
    k = np.exp(-(i * i) / (2 * SIGMA * SIGMA))
    return (k / k.sum()).astype(np.float32)


def image(g, shape):
    """Smooth blobs plus noise, uint8.  The noise is two-sided so that few residuals fall near the threshold: a share NOISE of the
    pixels steps by +-(18 .. 32) levels, the others move by a Gaussian of 1.5 levels."""
    N, C, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty(shape, dtype=np.float64)
    for n in range(N):
        for c in range(C):
            a = np.zeros((H, W))
            for _ in range(4):
                cy, cx, s = g.uniform(0, H), g.uniform(0, W), g.uniform(3, 12)
                a += g.uniform(0.4, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            a = a / max(a.max(), 1e-9)
            step = g.uniform(18, 32, (H, W)) * np.where(g.random_sample((H, W)) < 0.5, -1.0, 1.0)
            noise = np.where(g.random_sample((H, W)) < NOISE, step, 1.5 * g.standard_normal((H, W)))
            out[n, c] = (0.4 + 0.2 * a) * 255 + noise
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def G(a, t):
    return correlate1d(correlate1d(a, t, axis=-1, mode="mirror"), t, axis=-2, mode="mirror")


def usm64(x, t, threshold):
    blur = G(x, t)
    res = x - blur
    mask = (np.abs(res) * 255.0 > threshold).astype(np.float64)
    soft = G(mask, t)
    sharp = np.clip(x + WEIGHT * res, 0.0, 1.0)
    return blur, mask, soft * sharp + (1.0 - soft) * x


def decided_threshold(v):
    """The middle of the widest gap of the values between 9 and 11 (the two ends count as values)."""
    inside = np.sort(np.concatenate([[9.0, 11.0], v[(v > 9.0) & (v < 11.0)]]))
    i = int(np.argmax(np.diff(inside)))
    return float((inside[i] + inside[i + 1]) / 2)


def q31(a):
    assert a.min() >= 0.0 and a.max() <= 1.0
    return np.rint(a * 2.0 ** 31).astype(np.uint32)


def build():
    g = np.random.RandomState(51)
    t32 = taps32()
    t = t32.astype(np.float64)
    arrays, meta = {"taps": t32}, {"cases": {}, "margin": MARGIN, "half_band": HALF_BAND, "weight": WEIGHT, "K": K, "sigma": SIGMA,
                                   "default_threshold": DEFAULT_THRESHOLD, "noise": NOISE}
    for name, shape in CASES:
        x8 = image(g, shape)
        x = (x8.astype(np.float32) / np.float32(255)).astype(np.float64)
        v = np.abs(x - G(x, t)) * 255.0
        thr = decided_threshold(v.ravel())
        assert np.abs(v - thr).min() >= 0.01, (name, thr, np.abs(v - thr).min())
        blur, mask, out = usm64(x, t, thr)
        frac = float(mask.mean())
        if name in "ABCD":
            assert 0.2 <= frac <= 0.8, (name, frac)
        undecided = np.abs(v - DEFAULT_THRESHOLD) <= MARGIN
        U = int(undecided.sum())
        assert U <= 0.001 * v.size, (name, U)
        level = np.clip(out, 0.0, 1.0) * 255.0
        near_half = float((np.abs(level - np.floor(level) - 0.5) <= HALF_BAND).mean())
        assert near_half <= 0.01, (name, near_half)
        arrays[f"{name}__x"] = x8
        arrays[f"{name}__blur_q31"] = q31(blur)
        arrays[f"{name}__out_q31"] = q31(out)
        arrays[f"{name}__mask"] = np.packbits(mask.astype(np.uint8).ravel())
        arrays[f"{name}__out8"] = np.rint(level).astype(np.uint8)
        arrays[f"{name}__undecided"] = np.packbits(undecided.ravel())
        meta["cases"][name] = dict(shape=list(shape), threshold=thr, gap=float(np.abs(v - thr).min()), mask_fraction=frac, U=U,
                                   near_half=near_half)
        print(f"{name}: shape {shape} threshold {thr:.6f} (nearest value {np.abs(v - thr).min():.4f} away) mask {frac:.3f} "
              f"undecided at 10: {U} near a half level: {near_half:.4%}")
    return arrays, meta


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args(argv)
    arrays, meta = build()
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "usm.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    size = os.path.getsize(path)
    assert size < 512 * 1024, size
    print(f"wrote {path}: {len(arrays)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
