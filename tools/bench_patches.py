"""Times grl_sample_patches at the two training shapes -- B 8, P 64, scale 4 (a 256 x 256 GT batch) and B 8, P 128, scale 1 -- from a
store of four synthetic 2K images (1080 x 2048 x 3, 8 bit) on the GPU, with all eight flag values in the work list: the HIP kernel
(one launch) against the torch restatement of the same work on the same GPU (per sample: index, flip, transpose, permute, contiguous,
float, div; then stack).  Warm-up, then the median of --reps runs, each timed with device events around one call.  The effective
rate counts the S S C bytes read and the 4 S S C bytes written per sample over the kernel's time.  Prints one JSON line.

    python tools/bench_patches.py [--reps 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import PatchStore  # noqa: E402
from tools.bench_metrics import _median_ms  # noqa: E402


def _torch_chain(store, work, S):
    """``work``: host list of (image, row, column, flags) in pixels of the store; crops lie inside the images."""
    out = []
    for n, r, c, f in work:
        x = store.image(n)[r : r + S, c : c + S]
        if f & 1:
            x = x.flip(0)
        if f & 2:
            x = x.flip(1)
        if f & 4:
            x = x.transpose(0, 1)
        out.append(x.permute(2, 0, 1).contiguous().to(torch.float32).div(255))
    return torch.stack(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_patches needs the GPU")
    g = np.random.RandomState(0)
    H, W, B = 1080, 2048, 8
    store = PatchStore([g.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(4)], "cuda:0")
    line = {"workload": f"grl_sample_patches, store of 4 x {H}x{W}x3 uint8, batch {B}, all 8 flag values",
            "device": torch.cuda.get_device_name(0), "reps": a.reps}
    for P, scale in ((64, 4), (128, 1)):
        S = P * scale
        rng = np.random.RandomState(P)
        work = [(b % 4, int(rng.randint(0, (H - S) // scale + 1)), int(rng.randint(0, (W - S) // scale + 1)), b % 8) for b in range(B)]
        wl = torch.tensor(work, dtype=torch.int32, device="cuda:0")
        pix = [(n, x * scale, y * scale, f) for n, x, y, f in work]
        out = torch.empty(B, 3, S, S, device="cuda:0")
        hip = lambda: store.sample(wl, P, scale, out=out)
        ref = lambda: _torch_chain(store, pix, S)
        equal = bool(torch.equal(hip().cpu(), ref().cpu()))           # (torch divides by a reciprocal on the GPU: may differ by 1 ulp)
        close = float((hip() - ref()).abs().max())
        k_ms = _median_ms(hip, a.reps, a.warmup)
        t_ms = _median_ms(ref, max(20, a.reps // 4), 5)
        moved = B * S * S * 3 * 5
        line[f"B{B}_P{P}_x{scale}"] = {"hip_ms_median": round(k_ms[0], 4), "hip_ms_min": round(k_ms[1], 4), "hip_ms_max": round(k_ms[2], 4),
                                       "torch_ms_median": round(t_ms[0], 4), "torch_ms_min": round(t_ms[1], 4),
                                       "speedup": round(t_ms[0] / k_ms[0], 1), "hip_effective_GBps": round(moved / (k_ms[0] * 1e-3) / 1e9, 1),
                                       "bitwise_equal_to_torch_on_gpu": equal, "max_abs_diff_to_torch_on_gpu": close}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
