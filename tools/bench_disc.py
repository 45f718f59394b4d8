"""Times the discriminator's kernels (csrc/disc.hip, grl_gemm_tn taps = 16) on the GPU at the layer shapes of
``UNetDiscriminatorSN(3, 64)`` for a 1 x 3 x 512 x 512 input (patch 128 at scale 4, batch 1):

  the three directions of the 4x4 stride-2 convolutions (conv1 .. conv3) and the x2 bilinear upsampling pair (the three decoder steps);
  for the 4x4 forward also the construction available before the direct kernel, in the same process, alternating with it: a
    materialised space-to-depth copy of the 1-padded input ([Ho + 1, Wo + 1, 4 Cin]) and grl_conv3x3_fwd over 4 Cin channels with
    the five dead taps zero (timed with the copy, and the convolution alone); its result is compared with the direct kernel's;
  the whole discriminator forward, and forward + backward of the D loss;
  one ``GanStep`` at GRL-Base ``bsr_psnr`` geometry (nearest+conv tail) next to the eager PSNR-stage step (forward, L1, backward,
    FusedAdamW) of the same run (--no-step skips both).

Warm-up, then the median (min, max) over --reps measurements, each the time between two device events around --inner back-to-back
calls, divided by --inner.  ``tflops`` = 2 * pixels * 16 * Cin * Cout over the median (the algorithm's operations, not the padded
ones).  One JSON line per measurement, printed and written to --out.

    python tools/bench_disc.py [--reps 20] [--warmup 3] [--inner 10] [--out profiles/disc_bench_line.json]

``--sn`` measures the spectral normalisation instead (csrc/spectral_norm.hip): the discriminator at 1 x 3 x 512 x 512 (the
reference's per-GPU GAN batch, bsr/grl.yaml) and at 8 x 3 x 256 x 256, forward and forward + backward, once on the kernels and once
on the torch chain they replaced -- ``UNetDiscriminatorSN._weights(chain=True)``, bound over the instance's method; the two forms
alternate in one process, each is timed twice and reports the run with the lower median, both medians beside it -- then the two
entry points alone on the eight layers of num_feat 64, and (unless --no-step) one ``GanStep`` on a single GPU in both forms.
Device-event medians as above, and beside them ``host_us``: the wall-clock time of the same calls up to a final synchronize,
which is where launch-bound glue shows.  ONE JSON line, printed and written to profiles/sn_bench_line.json.

    python tools/bench_disc.py --sn [--no-step]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.bench_metrics import _median_ms  # noqa: E402


def s2d_operands(x, w, B, H, W):
    """(copy(), weights, bias) of the parent-commit construction: x tokens [B*H*W, Cin] -> space-to-depth of the padded image as
    tokens [B*(Ho+1)*(Wo+1), 4 Cin]; w [Cout, Cin, 4, 4] -> a 3x3 weight over 4 Cin channels, live taps (1..2, 1..2)."""
    from grl_image_restoration_amd import ops

    Cout, Cin = w.shape[:2]
    Ho, Wo = H // 2, W // 2

    def copy():
        p = F.pad(x.view(B, H, W, Cin), (0, 0, 1, 1, 1, 1))                               # [B, H+2, W+2, Cin]
        p = p.view(B, Ho + 1, 2, Wo + 1, 2, Cin).permute(0, 1, 3, 2, 4, 5)                # [B, Y, X, py, px, ci]
        return p.reshape(B * (Ho + 1) * (Wo + 1), 4 * Cin)

    w3 = torch.zeros(Cout, 2, 2, Cin, 3, 3, device=w.device)
    for i in range(2):
        for j in range(2):
            for py in range(2):
                for px in range(2):
                    w3[:, py, px, :, 1 + i, 1 + j] = w[:, :, 2 * i + py, 2 * j + px]
    w3 = w3.view(Cout, 4 * Cin, 3, 3)
    return copy, ops.pack_conv_weight(w3, 4 * Cin, Cout), torch.zeros(Cout, device=w.device)


def sn_bench(a, timed, dev):
    """--sn (module docstring): returns the one result line."""
    import functools

    from grl_image_restoration_amd import ops
    from grl_image_restoration_amd.discriminator import UNetDiscriminatorSN
    from grl_image_restoration_amd.gan import GanStep, gan_loss

    def both(fn, **kw):
        """Device-event statistics of ``fn`` and the host's wall-clock median for the same call (synchronised)."""
        t = timed(fn, **kw)
        walls = []
        for _ in range(max(5, a.reps // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e6)
        return dict(t, host_us=round(sorted(walls)[len(walls) // 2], 2))

    def ab(d, fn, **kw):
        """kernels / chain / kernels / chain; per form the run with the lower median, both medians beside it."""
        chain = functools.partial(UNetDiscriminatorSN._weights, d, chain=True)
        runs = {"kernels": [], "chain": []}
        for form in ("kernels", "chain", "kernels", "chain"):
            if form == "chain":
                d._weights = chain                   # (an instance attribute over the class's method)
            else:
                d.__dict__.pop("_weights", None)
            runs[form].append(both(fn, **kw))
        d.__dict__.pop("_weights", None)
        out = {}
        for form, (r1, r2) in runs.items():
            best = r1 if r1["us_median"] <= r2["us_median"] else r2
            out[form] = dict(best, us_median_first=r1["us_median"], us_median_second=r2["us_median"])
        out["chain_over_kernels"] = round(out["chain"]["us_median"] / out["kernels"]["us_median"], 3)
        out["host_us_saved"] = round(out["chain"]["host_us"] - out["kernels"]["host_us"], 1)
        return out

    res = dict(workload="spectral normalisation of UNetDiscriminatorSN(3, 64): HIP kernels vs the torch chain", device=dev,
               date=time.strftime("%Y-%m-%d"), reps=a.reps, inner=2)
    g = torch.Generator(device="cuda").manual_seed(0)
    torch.manual_seed(0)
    d = UNetDiscriminatorSN(3, 64, True).cuda().train()
    for B, H in ((1, 512), (8, 256)):
        img = torch.rand(B, 3, H, H, device="cuda", generator=g)
        with torch.no_grad():
            for _ in range(5):
                d(img)

        def fwd():
            with torch.no_grad():
                d(img)

        def fwd_bwd():
            for p in d.parameters():
                p.grad = None
            gan_loss(d(img), True, is_disc=True).backward()

        res[f"forward {B}x3x{H}x{H}"] = ab(d, fwd, inner=2)
        res[f"forward+backward {B}x3x{H}x{H}"] = ab(d, fwd_bwd, inner=2)
    convs = [getattr(d, f"conv{i}") for i in range(1, 9)]
    ws, us, vs = [c.weight_orig.detach() for c in convs], [c.weight_u.clone() for c in convs], [c.weight_v.clone() for c in convs]
    _, kept = ops.spectral_norm(ws, us, vs, True)
    gs = [torch.randn_like(w) for w in ws]
    res["grl_spectral_norm_fwd, 8 layers (3 launches)"] = both(lambda: ops.spectral_norm(ws, us, vs, True))
    res["grl_spectral_norm_fwd eval, 8 layers (2 launches)"] = both(lambda: ops.spectral_norm(ws, us, vs, False))
    res["grl_spectral_norm_bwd, 8 layers (2 launches)"] = both(lambda: ops.spectral_norm_bwd(gs, ws, kept))
    res["weight_megabytes"] = round(sum(w.numel() for w in ws) * 4 / 1e6, 2)
    if not a.no_step:
        from grl_image_restoration_amd import GRL, FusedAdamW, make_config

        torch.manual_seed(0)
        net = GRL(**make_config("base", "bsr_psnr", upscale=4, img_size=128, upsampler="nearest+conv")).cuda().train()
        opt_g, opt_d = FusedAdamW(net.parameters(), lr=1e-4, weight_decay=0), FusedAdamW(d.parameters(), lr=1e-4, weight_decay=0)
        lq, gt = torch.rand(1, 3, 128, 128, device="cuda", generator=g), torch.rand(1, 3, 512, 512, device="cuda", generator=g)
        step = GanStep(net, d, opt_g, opt_d, lambda y, t_: (y - t_).abs().mean(), usm_pixel=True, usm_gan=False)
        res["GanStep (eager), GRL-Base bsr_psnr x4, LQ 128, batch 1, one GPU"] = ab(d, lambda: step(lq, gt, gt), inner=1,
                                                                                     reps=max(3, a.reps // 4), warmup=2)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--sn", action="store_true", help="measure the spectral normalisation: kernels against the torch chain")
    ap.add_argument("--out", default=None, help="default: profiles/disc_bench_line.json (--sn: profiles/sn_bench_line.json)")
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "sn_bench_line.json" if a.sn else "disc_bench_line.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_disc needs the GPU")
    from grl_image_restoration_amd import autograd as AG
    from grl_image_restoration_amd import ops
    from grl_image_restoration_amd.discriminator import UNetDiscriminatorSN
    from grl_image_restoration_amd.gan import GanStep, gan_loss

    dev = torch.cuda.get_device_name(0)
    lines = []

    def emit(**kw):
        line = dict(dict(device=dev, reps=a.reps, inner=a.inner), **kw)
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))

    def timed(fn, inner=None, reps=None, warmup=None):
        inner = inner or a.inner
        med, lo, hi = _median_ms(lambda: [fn() for _ in range(inner)], reps or a.reps, warmup or a.warmup)
        return dict(us_median=round(med / inner * 1e3, 2), us_min=round(lo / inner * 1e3, 2), us_max=round(hi / inner * 1e3, 2))

    if a.sn:
        line = json.dumps(sn_bench(a, timed, dev))
        print(line, flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return

    g = torch.Generator(device="cuda").manual_seed(0)
    B = 1
    for name, Cin, Cout, H in (("conv1", 64, 128, 512), ("conv2", 128, 256, 256), ("conv3", 256, 512, 128)):
        W = H
        Ho, Wo = H // 2, W // 2
        x = torch.randn(B * H * W, Cin, device="cuda", generator=g)
        w = torch.randn(Cout, Cin, 4, 4, device="cuda", generator=g) / (16 * Cin) ** 0.5
        dy = torch.randn(B * Ho * Wo, Cout, device="cuda", generator=g)
        wp = ops.pack_conv4x4(w, Cout, Cin)
        wt = ops.pack_conv4x4(w, Cin, Cout, transpose=True)
        flop = 2.0 * B * Ho * Wo * 16 * Cin * Cout
        direct = lambda: ops.conv4x4s2(x, wp, B, H, W, x_cols=Cin, n_store=Cout, act=2, slope=0.2)
        copy, w3, b3 = s2d_operands(x, w, B, H, W)
        xs = copy()
        via3 = lambda: ops.conv3x3(xs, w3, b3, B, Ho + 1, Wo + 1, act=2, slope=0.2)
        both = lambda: ops.conv3x3(copy(), w3, b3, B, Ho + 1, Wo + 1, act=2, slope=0.2)
        diff = float((via3().view(B, Ho + 1, Wo + 1, Cout)[:, :Ho, :Wo] - direct().view(B, Ho, Wo, Cout)).abs().max())
        # alternate the two constructions (measuring guide: compare two versions in the same call); each side is timed twice and
        # reports the run with the lower median, both medians beside it
        t_d1, t_s1, t_c, t_d2, t_s2 = timed(direct), timed(both), timed(via3), timed(direct), timed(both)
        t_d = t_d1 if t_d1["us_median"] <= t_d2["us_median"] else t_d2
        t_s = t_s1 if t_s1["us_median"] <= t_s2["us_median"] else t_s2
        tag = f"{name} {Cin}->{Cout} {H}x{W}"
        emit(workload=f"conv4x4s2 fwd {tag}", **t_d, tflops=round(flop / (t_d["us_median"] * 1e-6) / 1e12, 1),
             us_median_first=t_d1["us_median"], us_median_second=t_d2["us_median"])
        emit(workload=f"space-to-depth copy + conv3x3 over 4 Cin {tag}", **t_s, us_median_first=t_s1["us_median"],
             us_median_second=t_s2["us_median"], conv_alone_us_median=t_c["us_median"], max_abs_diff_to_direct=diff)
        t = timed(lambda: ops.conv4x4s2(dy, wt, B, H, W, x_cols=Cout, n_store=Cin, transposed=True))
        emit(workload=f"conv4x4s2 bwd_data {tag}", **t, tflops=round(flop / (t["us_median"] * 1e-6) / 1e12, 1))
        t = timed(lambda: ops.gemm_tn(dy, x, Cout, Cin, taps=16, hw=(Ho, Wo)))
        emit(workload=f"gemm_tn taps=16 (dW) {tag}", **t, tflops=round(flop / (t["us_median"] * 1e-6) / 1e12, 1))
        del x, dy, xs
    for C_, H in ((512, 64), (256, 128), (128, 256)):
        x = torch.randn(B * H * H, C_, device="cuda", generator=g)
        dy = torch.randn(B * 4 * H * H, C_, device="cuda", generator=g)
        nbytes = 5 * x.numel() * 4
        t = timed(lambda: ops.upsample2x(x, B, H, H))
        emit(workload=f"upsample2x fwd C{C_} {H}x{H}", **t, gbs_algorithmic=round(nbytes / (t["us_median"] * 1e-6) / 1e9, 1))
        t = timed(lambda: ops.upsample2x(dy, B, H, H, backward=True))
        emit(workload=f"upsample2x bwd C{C_} {H}x{H}", **t, gbs_algorithmic=round(nbytes / (t["us_median"] * 1e-6) / 1e9, 1))
        del x, dy

    torch.manual_seed(0)
    d = UNetDiscriminatorSN(3, 64, True).cuda().train()
    img = torch.rand(1, 3, 512, 512, device="cuda", generator=g)
    with torch.no_grad():
        for _ in range(5):
            d(img)

    def fwd():
        with torch.no_grad():
            d(img)

    def fwd_bwd():
        for p in d.parameters():
            p.grad = None
        gan_loss(d(img), True, is_disc=True).backward()

    emit(workload="UNetDiscriminatorSN(3, 64) forward 1x3x512x512 (train mode, eager)", **timed(fwd, inner=2), inner=2)
    emit(workload="UNetDiscriminatorSN(3, 64) forward + backward 1x3x512x512 (eager)", **timed(fwd_bwd, inner=2), inner=2)

    if not a.no_step:
        from grl_image_restoration_amd import GRL, FusedAdamW, make_config

        torch.manual_seed(0)
        net = GRL(**make_config("base", "bsr_psnr", upscale=4, img_size=128, upsampler="nearest+conv")).cuda().train()
        opt_g, opt_d = FusedAdamW(net.parameters(), lr=1e-4, weight_decay=0), FusedAdamW(d.parameters(), lr=1e-4, weight_decay=0)
        l1 = lambda y, t_: (y - t_).abs().mean()
        lq, gt = torch.rand(1, 3, 128, 128, device="cuda", generator=g), torch.rand(1, 3, 512, 512, device="cuda", generator=g)
        step = GanStep(net, d, opt_g, opt_d, l1, usm_pixel=True, usm_gan=False)

        def psnr_step():
            opt_g.zero_grad(set_to_none=True)
            l1(net(lq), gt).backward()
            opt_g.step()

        r = dict(inner=1, reps=max(3, a.reps // 4), warmup=2)
        gan_step = lambda: step(lq, gt, gt)
        t_p1, t_g1, t_p2, t_g2 = timed(psnr_step, **r), timed(gan_step, **r), timed(psnr_step, **r), timed(gan_step, **r)
        t_g = t_g1 if t_g1["us_median"] <= t_g2["us_median"] else t_g2
        emit(workload="eager PSNR-stage step, GRL-Base bsr_psnr x4, LQ 128, batch 1", ms_median=round(min(t_p1["us_median"], t_p2["us_median"]) / 1e3, 2),
             ms_median_first=round(t_p1["us_median"] / 1e3, 2), ms_median_second=round(t_p2["us_median"] / 1e3, 2), reps=r["reps"], inner=1)
        emit(workload="GanStep (eager), same generator + UNetDiscriminatorSN(3, 64)", ms_median=round(t_g["us_median"] / 1e3, 2),
             ms_median_first=round(t_g1["us_median"] / 1e3, 2), ms_median_second=round(t_g2["us_median"] / 1e3, 2),
             ms_min=round(t_g["us_min"] / 1e3, 2), ms_max=round(t_g["us_max"] / 1e3, 2), reps=r["reps"], inner=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
