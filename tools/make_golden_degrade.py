"""Writes tests/golden/tasks/degrade.npz, the yardstick of the blind-SR degradation's blur (bsr_degrade.blur_items, csrc/blur_items.hip)
and of its anisotropic Gaussian kernel, from scipy alone: nothing of the package or of the reference is imported.

  blur cases   ``scipy.ndimage.convolve(x[c], k, mode="mirror")[::s, ::s]`` per channel in float64, on the fp32 values of a random
               image in [0, 1] and of a random NON-SYMMETRIC kernel ``k`` (positive, sum 1 before the fp32 rounding): a missing flip
               or a transposition of the taps shows.  The file holds ``k`` as ``ndimage.convolve`` takes it; the code under test gets
               it flipped over both axes (correlation taps).  Kernel sides 3, 7 and 25; an image smaller than the kernel, a
               one-row gray image, strides 2 and 4 (the pipeline's), and stride 5 (beyond the kernel's staged path).
  kernels      ``scipy.stats.multivariate_normal.pdf`` on the grid of the reference's ``gm_blur_kernel`` (utils_sisr.py:64-74),
               divided by its sum, for a few (ksize, theta, l1, l2).

    python tools/make_golden_degrade.py
"""
import json
import os

import numpy as np
from scipy import ndimage, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tasks", "degrade.npz")

# name: (shape, K, stride)
BLUR_CASES = {
    "k3": ((3, 40, 70), 3, 1),
    "k7": ((3, 40, 70), 7, 1),
    "k25": ((3, 40, 70), 25, 1),
    "tiny_k25": ((3, 5, 4), 25, 1),
    "row_k7": ((1, 1, 30), 7, 1),
    "s2_k7": ((3, 37, 53), 7, 2),
    "s4_k25": ((3, 37, 53), 25, 4),
    "s5_k3": ((3, 37, 53), 3, 5),
}
# (ksize, theta, l1, l2)
KERNELS = [(7, 0.3, 2.0, 0.7), (15, 2.5, 6.0, 1.5), (25, 1.0, 0.4, 7.5), (9, 0.0, 3.0, 3.0)]


def main():
    g = np.random.RandomState(20240)
    arrays, meta = {}, {"blur": {}, "kernels": []}
    for name, (shape, K, s) in BLUR_CASES.items():
        x = g.rand(*shape).astype(np.float32)
        k = g.rand(K, K) + 0.05
        k = (k / k.sum()).astype(np.float32)
        assert not np.array_equal(k, np.flip(k)) and not np.array_equal(k, k.T)
        out = np.stack([ndimage.convolve(x[c].astype(np.float64), k.astype(np.float64), mode="mirror") for c in range(shape[0])])
        arrays[f"{name}__x"], arrays[f"{name}__k"], arrays[f"{name}__out"] = x, k, out[:, ::s, ::s].copy()
        meta["blur"][name] = {"shape": list(shape), "K": K, "stride": s}
    for n, (ksize, theta, l1, l2) in enumerate(KERNELS):
        c, s = np.cos(theta), np.sin(theta)
        V = np.array([[c, s], [s, -c]])
        cov = V @ np.diag([l1, l2]) @ np.linalg.inv(V)
        center = ksize / 2.0 + 0.5
        k = np.zeros((ksize, ksize))
        for y in range(ksize):
            for x in range(ksize):
                k[y, x] = stats.multivariate_normal.pdf([x - center + 1, y - center + 1], mean=[0, 0], cov=cov)
        arrays[f"kernel_{n}"] = k / k.sum()
        meta["kernels"].append({"ksize": ksize, "theta": theta, "l1": l1, "l2": l2})
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
