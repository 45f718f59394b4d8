"""Times grl_sample_patches at the two training shapes -- B 8, P 64, scale 4 (a 256 x 256 GT batch) and B 8, P 128, scale 1 -- from a
store of four synthetic 2K images (1080 x 2048 x 3, 8 bit) on the GPU, with all eight flag values in the work list: the HIP kernel
(one launch) against the torch restatement of the same work on the same GPU (per sample: index, flip, transpose, permute, contiguous,
float, div; then stack).  Warm-up, then the median of --reps runs, each timed with device events around one call.  The effective
rate counts the S S C bytes read and the 4 S S C bytes written per sample over the kernel's time.  Prints one JSON line.

With --views also the dual-pixel batch (left view, right view, GT from three stores): ONE grl_sample_patch_views launch against the
three grl_sample_patches launches plus ``torch.cat`` it replaces, at batch 1 x patch 480 (the reference's per-GPU training shape,
db_defocus/grl_dual_p480) and batch 8 x patch 96.  Both run in the same process and alternate: --rounds rounds, in each the median of
--reps calls of one and then of the other; the line holds every round's medians, their median and their spread (min .. max over the
rounds).  Bytes moved: the one launch reads 9 S S and writes 36 S S per sample; the cat reads and writes the 24 S S of the
6-channel batch once more.

    python tools/bench_patches.py [--reps 200] [--warmup 20] [--views [--rounds 7]]
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


def _views(reps, warmup, rounds):
    """{shape: numbers} of the dual-pixel batch, one launch against three launches plus a cat, alternating."""
    from grl_image_restoration_amd.data import sample_views

    g = np.random.RandomState(1)
    H, W = 1120, 1680                                      # the size of a DPDD view
    left, right, gt = (PatchStore([g.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2)], "cuda:0") for _ in range(3))
    out = {}
    for B, P in ((1, 480), (8, 96)):
        rng = np.random.RandomState(P)
        wl = torch.tensor([(b % 2, int(rng.randint(0, H - P + 1)), int(rng.randint(0, W - P + 1)), b % 8) for b in range(B)],
                          dtype=torch.int32, device="cuda:0")
        lq, tg = torch.empty(B, 6, P, P, device="cuda:0"), torch.empty(B, 3, P, P, device="cuda:0")
        one = lambda: sample_views([(left, 1, lq, 0), (right, 1, lq, 3), (gt, 1, tg, 0)], wl, P)
        three = lambda: (torch.cat([left.sample(wl, P, 1), right.sample(wl, P, 1)], dim=1), gt.sample(wl, P, 1))
        one()
        equal = bool(torch.equal(lq, three()[0]) and torch.equal(tg, three()[1]))
        a, b = [], []
        for _ in range(rounds):
            a.append(_median_ms(one, reps, warmup)[0])
            b.append(_median_ms(three, reps, warmup)[0])
        med = lambda v: sorted(v)[len(v) // 2]
        S2 = B * P * P
        out[f"B{B}_P{P}"] = {"views_ms_rounds": [round(v, 4) for v in a], "three_plus_cat_ms_rounds": [round(v, 4) for v in b],
                             "views_ms": round(med(a), 4), "views_ms_spread": [round(min(a), 4), round(max(a), 4)],
                             "three_plus_cat_ms": round(med(b), 4), "three_plus_cat_ms_spread": [round(min(b), 4), round(max(b), 4)],
                             "views_bytes": 45 * S2, "three_plus_cat_bytes": (45 + 48) * S2, "bitwise_equal": equal}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--views", action="store_true", help="also time grl_sample_patch_views against three launches plus torch.cat")
    ap.add_argument("--rounds", type=int, default=7, help="--views: alternations of the two")
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
    if a.views:
        line["views"] = dict(_views(a.reps, a.warmup, a.rounds), rounds=a.rounds,
                             workload="dual-pixel batch from three stores of 2 x 1120x1680x3 uint8, all flag values")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
