"""NIQE of one 3 x 2040 x 2720 image (a x4 output) on the GPU: the HIP path (metrics.niqe: grl_image_niqe_features + the 36 x 36
tail) next to the float64 torch restatement on the same GPU; median of 30 after warm-up, events on the stream.

    python tools/bench_niqe.py --params niqe_pris_params.npz [--out profiles/niqe_bench_line.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grl_image_restoration_amd import metrics as M  # noqa: E402

LAUNCHES = 5            # Y plane, sums at scale 1, grl_imresize, sums at scale 2, finalize


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--params", default=os.environ.get(M.NIQE_ENV))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    params = M.load_niqe_params(a.params)
    B, C, H, W = 1, 3, 2040, 2720
    g = torch.Generator().manual_seed(0)
    lo = torch.nn.functional.interpolate(torch.rand(B, C, H // 8, W // 8, generator=g), size=(H, W), mode="bicubic", align_corners=False)
    x = (0.1 + 0.6 * lo + 0.2 * torch.rand(B, C, H, W, generator=g)).clamp(0, 1).to("cuda:0")
    feat = M.hip_niqe_features(x)
    ref = M.niqe_features_torch(x)
    score, score_t = float(M.niqe(x, params)), float(M._niqe_tail(ref, *(p.to(x.device) for p in params)))
    hip_feat_ms = timed(lambda: M.hip_niqe_features(x), a.steps, a.warmup)
    hip_ms = timed(lambda: M.niqe(x, params), a.steps, a.warmup)
    torch_ms = timed(lambda: M._niqe_tail(M.niqe_features_torch(x), *(p.to(x.device) for p in params)), a.torch_steps, 1)
    nbh, nbw = H // 96, W // 96
    read = B * C * H * W * 4                                       # the image, once; everything after it stays in the workspace
    line = dict(workload=f"NIQE, {C} x {H} x {W} fp32 ({nbh * nbw} blocks)", niqe=score, niqe_torch=score_t,
                hip_ms=hip_ms, hip_features_ms=hip_feat_ms, torch_float64_ms=torch_ms, speedup=torch_ms / hip_ms, launches=LAUNCHES,
                bytes_read=read, gb_per_s=read / hip_feat_ms / 1e6, steps=a.steps,
                max_feature_diff=float((feat - ref).abs().nan_to_num(0).max()))
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    assert hip_ms < torch_ms, (hip_ms, torch_ms)


if __name__ == "__main__":
    main()
