"""Times the perceptual loss (csrc/vgg.hip, perceptual.py) on the GPU:

  the tap kernels (grl_vgg_tap_fwd with its finishing launch, grl_vgg_tap_bwd) at the five tap shapes of a 1 x 3 x 256 x 256 input,
    each next to the unfused torch construction on the same channels-last layout -- ``l1_loss`` on the two feature matrices and
    ``max_pool2d(relu(.))`` of both, and autograd through ``coef * |fx - fg|.sum() + <max_pool2d(relu(fx)), dpool>`` -- the two
    alternating in one process (each side is timed twice and reports the run with the lower median, both medians beside it);
  the whole perceptual forward, and forward + backward (dL/dx), at 1 and at --batch images of 3 x 256 x 256 with the yaml's five taps;
  one eager ``GanStep`` at GRL-Base ``bsr_psnr`` geometry (nearest+conv tail, LQ 64 -> GT 256, batch 1) with and without the term
    (--no-step skips both).

Warm-up, then the median (min, max) over --reps measurements, each the time between two device events around --inner back-to-back
calls, divided by --inner.  ``gbs_algorithmic``: the bytes the fused kernel has to move (both feature matrices read once, fp16 pooled
outputs written; backward: both read, dpool read, dfx written) over the median.  One JSON line per measurement, printed and written
to --out.

    python tools/bench_vgg.py [--reps 20] [--warmup 3] [--inner 200] [--batch 8] [--out profiles/vgg_bench_line.json]

``--style`` times the style loss instead (csrc/gram.hip, perceptual.PerceptualStyleLoss) at --batch images of 3 x 256 x 256 and writes
profiles/style_bench_line.json:
  ``PerceptualLoss`` and ``PerceptualStyleLoss`` (style weight 400), forward and forward + backward, the two classes alternating in one
    process (a, b, a, b; the lower-median run of each, both medians beside it);
  each Gram launch alone at the five tap shapes -- ``grl_vgg_gram_fwd`` on the 2 x batch images, ``grl_vgg_gram_loss``, and
    ``grl_vgg_gram_bwd`` on the batch restored images -- with ``gbs_algorithmic``, the bytes the launch must move over the median
    (forward: the features read once, G written; loss: G read, D written; backward: the features and D read, the gradient matrix
    read and written), and for the two contractions ``tflops`` (forward: the upper triangle's 64 x 64 blocks that are computed).

    python tools/bench_vgg.py --style [--batch 8] [--out profiles/style_bench_line.json]
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.bench_metrics import _median_ms  # noqa: E402

TAP_SHAPES = (("conv1_2", 64, 256), ("conv2_2", 128, 128), ("conv3_4", 256, 64), ("conv4_4", 512, 32), ("conv5_4", 512, 16))


def style_bench(a, g, emit, timed, ab):
    """--style: the two loss classes alternating, then each Gram launch alone at the five tap shapes."""
    from grl_image_restoration_amd import ops
    from grl_image_restoration_amd import perceptual as P

    B = a.batch
    sd = P.seeded_state_dict(0)
    pl = P.PerceptualLoss(P.GAN_LAYER_WEIGHTS, sd).cuda()
    ps = P.PerceptualStyleLoss(P.GAN_LAYER_WEIGHTS, sd, style_weight=400.0).cuda()
    gt = torch.rand(B, 3, 256, 256, device="cuda", generator=g)
    x = (gt + 0.1 * torch.randn(B, 3, 256, 256, device="cuda", generator=g)).clamp(0, 1)

    def fwd(mod):
        def run():
            with torch.no_grad():
                return mod(x, gt)
        return run

    def fwd_bwd(mod):
        def run():
            leaf = x.detach().requires_grad_(True)
            percep, style = mod(leaf, gt)
            (percep if style is None else percep + style).backward()
            return leaf.grad
        return run

    r = dict(inner=10, reps=max(5, a.reps // 2))
    for what, make in (("forward", fwd), ("forward + backward", fwd_bwd)):
        t = [timed(make(pl), **r), timed(make(ps), **r), timed(make(pl), **r), timed(make(ps), **r)]
        for label, u, v in ((f"PerceptualLoss {what} {B}x3x256x256", t[0], t[2]), (f"PerceptualStyleLoss {what} {B}x3x256x256 (style weight 400)", t[1], t[3])):
            best = u if u["us_median"] <= v["us_median"] else v
            emit(workload=label, ms_median=round(best["us_median"] / 1e3, 3), ms_min=round(best["us_min"] / 1e3, 3), ms_max=round(best["us_max"] / 1e3, 3),
                 ms_medians=[round(u["us_median"] / 1e3, 3), round(v["us_median"] / 1e3, 3)], **r)
    emit(workload="operand scale of the last backward", perceptual_log2=int(math.log2(pl.last_scale)), perceptual_style_log2=int(math.log2(ps.last_scale)))
    del x, gt
    nb = 2 * B
    for name, C_, H in TAP_SHAPES:
        hw = H * H
        f = torch.randn(nb * hw, C_, device="cuda", generator=g)
        d = torch.randn(B * hw, C_, device="cuda", generator=g)
        loss = torch.zeros(1, device="cuda")
        gram = ops.vgg_gram(f, nb, hw)
        diff = ops.vgg_gram_loss(gram, loss, 1.0, accumulate=False)
        tag = f"{name} C{C_} {H}x{H}"
        inner = max(10, a.inner // 10)
        nT = C_ // 64
        for label, fn, nbytes, flop in (
                (f"vgg_gram fwd {nb} images {tag}", lambda: ops.vgg_gram(f, nb, hw), nb * hw * C_ * 4 + nb * C_ * C_ * 4, 2.0 * nb * hw * 64 * 64 * (nT * (nT + 1) / 2 - nT / 4)),
                (f"vgg_gram_loss {B}+{B} images {tag}", lambda: ops.vgg_gram_loss(gram, loss, 1.0, accumulate=False), 3 * B * C_ * C_ * 4, None),
                (f"vgg_gram_bwd {B} images {tag}", lambda: ops.vgg_gram_bwd(f, diff, hw, 1e-9, d), 3 * B * hw * C_ * 4 + B * C_ * C_ * 4, 2.0 * B * hw * C_ * C_)):
            t = timed(fn, inner=inner)
            extra = dict(tflops=round(flop / (t["us_median"] * 1e-6) / 1e12, 1)) if flop else {}
            emit(workload=label, **t, mbytes=round(nbytes / 1e6, 1), gbs_algorithmic=round(nbytes / (t["us_median"] * 1e-6) / 1e9, 1), **extra)
        del f, d, gram, diff


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=200, help="back-to-back calls per timed window of the tap kernels (200 x ~15 us = ~3 ms)")
    ap.add_argument("--batch", type=int, default=8, help="the whole loss is timed at batch 1 and at this batch")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--style", action="store_true", help="time the style loss (csrc/gram.hip) instead; writes profiles/style_bench_line.json")
    ap.add_argument("--out", default=None, help="default: profiles/vgg_bench_line.json (--style: profiles/style_bench_line.json)")
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "style_bench_line.json" if a.style else "vgg_bench_line.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench_vgg needs the GPU")
    from grl_image_restoration_amd import ops
    from grl_image_restoration_amd import perceptual as P
    from grl_image_restoration_amd.gan import GanStep

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

    def ab(f_a, f_b):
        """a, b, a, b: (the lower-median run of each, [first, second] medians of each)."""
        t = [timed(f_a), timed(f_b), timed(f_a), timed(f_b)]
        pick = lambda u, v: u if u["us_median"] <= v["us_median"] else v
        return pick(t[0], t[2]), pick(t[1], t[3]), [t[0]["us_median"], t[2]["us_median"]], [t[1]["us_median"], t[3]["us_median"]]

    g = torch.Generator(device="cuda").manual_seed(0)
    if a.style:
        style_bench(a, g, emit, timed, ab)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    B = 1
    for name, C_, H in TAP_SHAPES:
        W = H
        pool = name != "conv5_4"
        n = B * H * W
        both = torch.randn(2 * n, C_, device="cuda", generator=g)          # the two halves of one matrix, as the chain has them
        fx, fg = both[:n], both[n:]
        dpool = torch.randn(B * (H // 2) * (W // 2), C_, device="cuda", generator=g) if pool else None
        loss = torch.zeros(1, device="cuda")
        coef = 1.0 / (n * C_)
        # NCHW views in channels_last memory format of the same storage: what eager torch would be handed on this layout
        ix, ig = (t.view(B, H, W, C_).permute(0, 3, 1, 2) for t in (fx, fg))
        idp = dpool.view(B, H // 2, W // 2, C_).permute(0, 3, 1, 2) if pool else None

        def fused_fwd():
            return ops.vgg_tap(fx, fg, B, H, W, loss, coef, accumulate=False, pool=pool)

        def torch_fwd():
            out = F.l1_loss(ix, ig)
            if pool:
                return out, F.max_pool2d(F.relu(ix), 2, 2).half(), F.max_pool2d(F.relu(ig), 2, 2).half()
            return out

        def fused_bwd():
            return ops.vgg_tap_bwd(fx, fg, B, H, W, coef, dpool)

        def torch_bwd():
            leaf = ix.detach().requires_grad_(True)
            out = coef * (leaf - ig).abs().sum()
            if pool:
                out = out + (F.max_pool2d(F.relu(leaf), 2, 2) * idp).sum()
            return torch.autograd.grad(out, leaf)[0]

        diff = float((fused_bwd().view(B, H, W, C_).permute(0, 3, 1, 2) - torch_bwd()).abs().max())
        tag = f"{name} C{C_} {H}x{W}" + ("" if pool else " (no pool)")
        bytes_f = 2 * n * C_ * 4 + (2 * (n // 4) * C_ * 2 if pool else 0)
        bytes_b = 3 * n * C_ * 4 + ((n // 4) * C_ * 4 if pool else 0)
        t_f, t_t, m_f, m_t = ab(fused_fwd, torch_fwd)
        emit(workload=f"vgg_tap fwd (+ finish) {tag}", **t_f, gbs_algorithmic=round(bytes_f / (t_f["us_median"] * 1e-6) / 1e9, 1), us_medians=m_f)
        emit(workload=f"torch l1_loss + relu + max_pool2d (+ .half()) x2 {tag}", **t_t, us_medians=m_t,
             fused_over_torch=round(t_f["us_median"] / t_t["us_median"], 3))
        t_f, t_t, m_f, m_t = ab(fused_bwd, torch_bwd)
        emit(workload=f"vgg_tap bwd {tag}", **t_f, gbs_algorithmic=round(bytes_b / (t_f["us_median"] * 1e-6) / 1e9, 1), us_medians=m_f,
             max_abs_diff_to_torch=diff)
        emit(workload=f"torch autograd of l1 + relu + max_pool2d {tag}", **t_t, us_medians=m_t,
             fused_over_torch=round(t_f["us_median"] / t_t["us_median"], 3))
        del both, fx, fg, dpool

    pl = P.PerceptualLoss(P.GAN_LAYER_WEIGHTS, P.seeded_state_dict(0)).cuda()
    for nb in sorted({1, a.batch}):
        gt = torch.rand(nb, 3, 256, 256, device="cuda", generator=g)
        x = (gt + 0.1 * torch.randn(nb, 3, 256, 256, device="cuda", generator=g)).clamp(0, 1)

        def fwd():
            with torch.no_grad():
                return pl(x, gt)[0]

        def fwd_bwd():
            leaf = x.detach().requires_grad_(True)
            pl(leaf, gt)[0].backward()
            return leaf.grad

        r = dict(inner=10, reps=max(5, a.reps // 2))
        # multiply-adds of the sixteen convolutions for the restored image and the target; the backward adds the restored image's data gradients
        gmac = 2 * nb * sum(cin * cout * 9 * (256 >> (int(n[4]) - 1)) ** 2 for n, _, cin, cout in pl.vgg.convs) / 1e9
        t = timed(fwd, **r)
        emit(workload=f"PerceptualLoss forward {nb}x3x256x256 (restored + target)", ms_median=round(t["us_median"] / 1e3, 3),
             ms_min=round(t["us_min"] / 1e3, 3), ms_max=round(t["us_max"] / 1e3, 3), gmac=round(gmac, 1),
             tflops=round(2 * gmac / t["us_median"] * 1e3, 1), **r)
        t = timed(fwd_bwd, **r)
        emit(workload=f"PerceptualLoss forward + backward {nb}x3x256x256", ms_median=round(t["us_median"] / 1e3, 3),
             ms_min=round(t["us_min"] / 1e3, 3), ms_max=round(t["us_max"] / 1e3, 3), gmac=round(1.5 * gmac, 1),
             tflops=round(2 * 1.5 * gmac / t["us_median"] * 1e3, 1), operand_scale_log2=int(math.log2(pl.last_scale)), **r)
        del x, gt

    if not a.no_step:
        from grl_image_restoration_amd import GRL, FusedAdamW, make_config
        from grl_image_restoration_amd.discriminator import UNetDiscriminatorSN

        torch.manual_seed(0)
        net = GRL(**make_config("base", "bsr_psnr", upscale=4, img_size=64, upsampler="nearest+conv")).cuda().train()
        d = UNetDiscriminatorSN(3, 64, True).cuda().train()
        opt_g, opt_d = FusedAdamW(net.parameters(), lr=1e-4, weight_decay=0), FusedAdamW(d.parameters(), lr=1e-4, weight_decay=0)
        l1 = lambda y, t_: (y - t_).abs().mean()
        lq, gt1 = torch.rand(1, 3, 64, 64, device="cuda", generator=g), torch.rand(1, 3, 256, 256, device="cuda", generator=g)
        plain = GanStep(net, d, opt_g, opt_d, l1, usm_pixel=True, usm_gan=False)
        with_p = GanStep(net, d, opt_g, opt_d, l1, usm_pixel=True, usm_gan=False, perceptual=pl, usm_percep=True)
        r = dict(inner=1, reps=max(3, a.reps // 4), warmup=2)
        f_a, f_b = (lambda: plain(lq, gt1, gt1)), (lambda: with_p(lq, gt1, gt1))
        t = [timed(f_a, **r), timed(f_b, **r), timed(f_a, **r), timed(f_b, **r)]
        for label, u, v in (("GanStep (eager), GRL-Base bsr_psnr x4, LQ 64, batch 1, no perceptual term", t[0], t[2]),
                            ("GanStep (eager), same, with the VGG19 perceptual term", t[1], t[3])):
            best = u if u["us_median"] <= v["us_median"] else v
            emit(workload=label, ms_median=round(best["us_median"] / 1e3, 2), ms_min=round(best["us_min"] / 1e3, 2),
                 ms_max=round(best["us_max"] / 1e3, 2), ms_medians=[round(u["us_median"] / 1e3, 2), round(v["us_median"] / 1e3, 2)], inner=r["inner"], reps=r["reps"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
