"""Times LPIPS (csrc/lpips.hip, lpips.py) on the GPU, at 1 x 3 x 512 x 512 and at a full validation image, 1 x 3 x 1356 x 2040:

  grl_lpips_tap alone (with its finishing launch) at the five tap shapes of each image size, on random fp32 features;
  the whole metric -- prep, thirteen convolutions, five taps -- on a random image pair with seeded weights.

Warm-up, then the median (min, max) over --reps measurements, each the time between two device events around ``inner`` back-to-back
calls, divided by ``inner`` (``inner`` is chosen per shape so that a window is about 3 ms or one call, whichever is longer).
``bytes_algorithmic``: what the tap kernel has to move -- the fp32 features of both images read once, the fp16 pooled outputs written
-- and ``gbs_achieved`` = those bytes over the median.  The features of the first two taps of the large image are over 1 GB each,
past the 256 MiB Infinity Cache; the small shapes fit in it and say nothing about HBM.  One JSON line per measurement, printed and
written to --out.  No time is fixed in advance.

    python tools/bench_lpips.py [--reps 20] [--warmup 3] [--sizes 512x512,1356x2040] [--out profiles/lpips_bench_line.json]

``--loss`` times LPIPS as a training loss instead (``lpips.LPIPSLoss``), at 8 x 3 x 256 x 256 and 1 x 3 x 512 x 512 (``--loss-shapes``):

  grl_lpips_tap_bwd alone at the five tap shapes, against the bytes it must move: both halves of the fp32 pre-activation read, the
  fp32 gradient written, the fp32 pool gradient read;
  forward + backward of ``LPIPSLoss`` (13 convolutions each way) and of ``perceptual.PerceptualLoss`` (VGG19: 16), one call of each
  in turn inside the same run, so that both see the same clocks;
  fp32 torch autograd of the same LPIPS expressions on the GPU (``F.conv2d`` / ``relu`` / ``max_pool2d`` / ``lpips_term``).

    python tools/bench_lpips.py --loss [--reps 20] [--warmup 3] [--out profiles/lpips_loss_bench_line.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.bench_metrics import _median_ms  # noqa: E402


def _alternate_ms(fns, reps, warmup):
    """Per function the sorted times of ``reps`` single calls, the functions taking turns within every repetition."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [sorted(t) for t in ts]


def _torch_lpips(model, x, gt):
    """fp32 torch on the tensors' device: the expressions of ``LPIPS.composite`` with autograd on, the mean over the batch."""
    import torch.nn.functional as F

    from grl_image_restoration_amd import lpips as LP

    B = x.shape[0]
    z = torch.cat([x, gt])
    z = ((2 * z - 1) - model.shift) / model.scale
    total, ci, tap = 0, 0, 0
    for pos, name in enumerate(LP.NAMES[: LP.TAP_INDEX[-1] + 1]):
        if name.startswith("conv"):
            z = F.conv2d(z, model.weights[ci], model.biases[ci], padding=1)
            ci += 1
        elif name.startswith("relu"):
            z = F.relu(z)
        else:
            z = F.max_pool2d(z, 2, 2)
        if pos == LP.TAP_INDEX[tap]:
            total = total + LP.lpips_term(z[:B], z[B:], model.lins[tap])
            tap += 1
    return total.mean()


def bench_loss(a, emit, timed):
    from grl_image_restoration_amd import lpips as LP
    from grl_image_restoration_amd import ops
    from grl_image_restoration_amd import perceptual as P

    g = torch.Generator(device="cuda").manual_seed(0)
    model = LP.LPIPS(*LP.seeded_weights(0)).cuda()
    loss = LP.LPIPSLoss(model)
    percep = P.PerceptualLoss(P.GAN_LAYER_WEIGHTS, P.seeded_state_dict(0)).cuda()
    for shape in a.loss_shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        h, w, total_us, total_bytes = H, W, 0.0, 0
        for l, (name, C_) in enumerate(zip(LP.TAPS, LP.WIDTHS)):
            pool = l < 4
            n = B * h * w
            f = torch.randn(2 * n, C_, device="cuda", generator=g)
            wl = torch.rand(C_, device="cuda", generator=g) / C_
            dpool = torch.randn(B * (h // 2) * (w // 2), C_, device="cuda", generator=g) if pool else None
            nbytes = 2 * n * C_ * 4 + n * C_ * 4 + (dpool.numel() * 4 if pool else 0)
            inner = max(1, min(200, int(3e-3 / (nbytes / 4e12 + 8e-6))))
            t = timed(lambda: ops.lpips_tap_bwd(f, wl, B, h, w, 1.0 / n, dpool), inner)
            emit(workload=f"lpips_tap_bwd {name} C{C_} {B}x{h}x{w} of {B}x3x{H}x{W}" + ("" if pool else " (no dpool)"), **t,
                 bytes_algorithmic=nbytes, gbs_achieved=round(nbytes / (t["us_median"] * 1e-6) / 1e9, 1))
            total_us, total_bytes = total_us + t["us_median"], total_bytes + nbytes
            del f, dpool
            h, w = h // 2, w // 2
        emit(workload=f"lpips_tap_bwd, the five taps of {B}x3x{H}x{W}", us_median=round(total_us, 2), bytes_algorithmic=total_bytes,
             gbs_achieved=round(total_bytes / (total_us * 1e-6) / 1e9, 1))
        gt = torch.rand(B, 3, H, W, device="cuda", generator=g)
        x = (gt + 0.05 * torch.randn(B, 3, H, W, device="cuda", generator=g)).clamp(0, 1).requires_grad_(True)

        def step(fn):
            x.grad = None
            fn().backward()

        names = ["LPIPSLoss forward + backward (HIP chain, VGG16: 13 convolutions)",
                 "PerceptualLoss forward + backward (HIP chain, VGG19: 16 convolutions)",
                 "LPIPS forward + backward, fp32 torch autograd on the GPU"]
        fns = [lambda: step(lambda: loss(x, gt)), lambda: step(lambda: percep(x, gt)[0]), lambda: step(lambda: _torch_lpips(model, x, gt))]
        for name, ts in zip(names, _alternate_ms(fns, a.reps, a.warmup)):
            emit(workload=f"{name} {B}x3x{H}x{W}", ms_median=round(ts[len(ts) // 2], 3), ms_min=round(ts[0], 3), ms_max=round(ts[-1], 3), inner=1,
                 alternating=True, **(dict(scale_log2=int(torch.log2(torch.tensor(loss.last_scale)))) if name.startswith("LPIPSLoss") else {}))
        del x, gt
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="512x512,1356x2040")
    ap.add_argument("--loss", action="store_true", help="time LPIPS as a training loss (lpips.LPIPSLoss) instead of the metric")
    ap.add_argument("--loss-shapes", default="8x256x256,1x512x512", help="--loss: BxHxW of the image batches")
    ap.add_argument("--out", default=None, help="default: profiles/lpips_bench_line.json, or profiles/lpips_loss_bench_line.json with --loss")
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "lpips_loss_bench_line.json" if a.loss else "lpips_bench_line.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips needs the GPU")
    from grl_image_restoration_amd import lpips as LP
    from grl_image_restoration_amd import ops

    dev = torch.cuda.get_device_name(0)
    lines = []

    def emit(**kw):
        line = dict(dict(device=dev, reps=a.reps), **kw)
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))

    def timed(fn, inner):
        med, lo, hi = _median_ms(lambda: [fn() for _ in range(inner)], a.reps, a.warmup)
        return dict(us_median=round(med / inner * 1e3, 2), us_min=round(lo / inner * 1e3, 2), us_max=round(hi / inner * 1e3, 2), inner=inner)

    if a.loss:
        bench_loss(a, emit, timed)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    g = torch.Generator(device="cuda").manual_seed(0)
    model = LP.LPIPS(*LP.seeded_weights(0)).cuda()
    B = 1
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        h, w, total_us, total_bytes = H, W, 0.0, 0
        for l, (name, C_) in enumerate(zip(LP.TAPS, LP.WIDTHS)):
            pool = l < 4
            n = B * h * w
            f = torch.randn(2 * n, C_, device="cuda", generator=g)
            wl = torch.rand(C_, device="cuda", generator=g) / C_
            out = torch.zeros(B, dtype=torch.float64, device="cuda")
            pooled = torch.empty(2 * B * (h // 2) * (w // 2), C_, dtype=ops.GEMM_DTYPE, device="cuda") if pool else None
            nbytes = 2 * n * C_ * 4 + (2 * B * (h // 2) * (w // 2) * C_ * 2 if pool else 0)
            inner = max(1, min(200, int(3e-3 / (nbytes / 4e12 + 8e-6))))
            t = timed(lambda: ops.lpips_tap(f, wl, B, h, w, out, accumulate=False, pool=pool, pool_out=pooled), inner)
            emit(workload=f"lpips_tap (+ finish) {name} C{C_} {h}x{w} of {H}x{W}" + ("" if pool else " (no pool)"), **t,
                 bytes_algorithmic=nbytes, gbs_achieved=round(nbytes / (t["us_median"] * 1e-6) / 1e9, 1))
            total_us, total_bytes = total_us + t["us_median"], total_bytes + nbytes
            del f, pooled
            h, w = h // 2, w // 2
        emit(workload=f"lpips_tap, the five taps of {H}x{W}", us_median=round(total_us, 2), bytes_algorithmic=total_bytes,
             gbs_achieved=round(total_bytes / (total_us * 1e-6) / 1e9, 1))
        gt = torch.rand(B, 3, H, W, device="cuda", generator=g)
        x = (gt + 0.05 * torch.randn(B, 3, H, W, device="cuda", generator=g)).clamp(0, 1)
        gmac = 2 * B * sum(cin * cout * 9 * (H >> (int(n_[4]) - 1)) * (W >> (int(n_[4]) - 1)) for n_, _, cin, cout in model.convs) / 1e9
        inner = 10 if H * W <= 512 * 512 else 1
        t = timed(lambda: model(x, gt), inner)
        emit(workload=f"LPIPS forward {B}x3x{H}x{W} (restored + target)", ms_median=round(t["us_median"] / 1e3, 3),
             ms_min=round(t["us_min"] / 1e3, 3), ms_max=round(t["us_max"] / 1e3, 3), inner=inner, gmac=round(gmac, 1),
             tflops=round(2 * gmac / t["us_median"] * 1e3, 1), value=float(model(x, gt)[0]))
        del x, gt
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
