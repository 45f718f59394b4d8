"""Times image8.pack8 (grl_image_pack8, one launch) on the GPU and what it replaces, at the two shapes of a saved x4 validation image:
the (1, 3, 1356, 2040) output at rep 1 and the (1, 3, 339, 510) input at rep 4 (the reference's ``F.interpolate(input,
scale_factor=4)`` before saving, engines/base.py:529-530).  Three measurements, one JSON line each, printed and written to --out:

  kernel     the median over --reps measurements, each the time between two device events around --inner back-to-back calls divided
             by --inner, for ``pack8`` and, alternating with it in the same loop, for the torch chain on the same device (``clamp ->
             mul -> round -> to(uint8) -> permute -> contiguous``, after ``F.interpolate`` at rep 4).  ``algorithm_bytes`` is what the
             conversion has to move (4 bytes read per SOURCE value, 1 byte written per output value); ``hbm_share`` sets that against
             --hbm-tbs (the 8.0 TB/s peak of the MI355X).  The output is checked against the CPU restatement first
  host       the host alternative: a device-to-host copy of the fp32 image and the numpy conversion (clip, multiply, rint, cast,
             transpose) on one thread, against ``pack8`` plus the copy of its bytes into pinned memory; host clock around a synchronise
  end2end    ``evaluate_folder`` over --images seeded 339 x 510 images at x4 (GRL-Base, random weights) with and without ``save_dir``
             (4 writer threads, LQ and HQ saved), alternating, wall clock from the call to its return (the writer is closed and the
             device idle by then); recorded, not gated: PNG compression on a shared host is the noisy part

    python tools/bench_image8.py [--reps 30] [--warmup 5] [--inner 20] [--images 16] [--out profiles/image8_bench_line.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import GRL, evaluate as EV, image8 as I, make_config  # noqa: E402

SHAPES = (("hq", (1, 3, 1356, 2040), 1), ("lq_x4", (1, 3, 339, 510), 4))


def torch_chain(x, rep):
    if rep > 1:
        x = F.interpolate(x, scale_factor=rep)
    return x.clamp(0.0, 1.0).mul(255.0).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _events_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def kernel_lines(a):
    g = torch.Generator().manual_seed(0)
    for what, shape, rep in SHAPES:
        x = (torch.rand(shape, generator=g) * 1.2 - 0.1).cuda()
        exact = bool(torch.equal(I.pack8(x, rep).cpu(), I._torch_pack8(x.cpu(), rep)))
        chain_equal = bool(torch.equal(torch_chain(x, rep), I.pack8(x, rep)))
        hip, chain = (lambda: I.pack8(x, rep)), (lambda: torch_chain(x, rep))
        for _ in range(a.warmup):
            _events_ms(hip, a.inner), _events_ms(chain, a.inner)
        th, tc = [], []
        for _ in range(a.reps):                                       # alternating: both see the same machine
            th.append(_events_ms(hip, a.inner))
            tc.append(_events_ms(chain, a.inner))
        (h, hmin, hmax), (c, cmin, cmax) = _stats(th), _stats(tc)
        out_bytes = x.numel() * rep * rep
        need = 4 * x.numel() + out_bytes
        yield {"workload": f"pack8 {what} {'x'.join(map(str, shape))} fp32, rep {rep}", "device": torch.cuda.get_device_name(0),
               "hip_us_median": round(h * 1e3, 2), "hip_us_min": round(hmin * 1e3, 2), "hip_us_max": round(hmax * 1e3, 2),
               "torch_chain_us_median": round(c * 1e3, 2), "torch_chain_us_min": round(cmin * 1e3, 2),
               "torch_chain_us_max": round(cmax * 1e3, 2), "chain_over_hip": round(c / h, 2), "algorithm_bytes": need,
               "algorithm_tbs": round(need / (h * 1e-3) / 1e12, 3), "hbm_peak_tbs": a.hbm_tbs,
               "hbm_share": round(need / (h * 1e-3) / 1e12 / a.hbm_tbs, 3), "equals_cpu_restatement": exact,
               "equals_torch_chain": chain_equal, "reps": a.reps, "inner": a.inner}


def host_line(a):
    """fp32 copy + numpy on one thread against pack8 + the copy of its bytes; each the median of ``reps // 3`` host-clock times."""
    g = torch.Generator().manual_seed(1)
    _, shape, _ = SHAPES[0]
    x = (torch.rand(shape, generator=g) * 1.2 - 0.1).cuda()
    pin32 = torch.empty(shape, dtype=torch.float32, pin_memory=True)
    pin8 = torch.empty((shape[0], shape[2], shape[3], shape[1]), dtype=torch.uint8, pin_memory=True)

    def host():
        pin32.copy_(x, non_blocking=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        v = pin32.numpy()[0]
        u8 = np.ascontiguousarray(np.rint(np.clip(v, 0.0, 1.0) * np.float32(255.0)).astype(np.uint8).transpose(1, 2, 0))
        return u8, time.perf_counter() - t

    def device():
        pin8.copy_(I.pack8(x), non_blocking=True)
        torch.cuda.synchronize()
        return pin8.numpy()[0]

    same = bool(np.array_equal(host()[0], device()))
    n = max(3, a.reps // 3)
    th, tn, td = [], [], []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, conv = host()
        th.append((time.perf_counter() - t0) * 1e3)
        tn.append(conv * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device()
        td.append((time.perf_counter() - t0) * 1e3)
    return {"workload": f"host alternative {'x'.join(map(str, shape))}: fp32 D2H + numpy on one thread vs pack8 + 8-bit D2H",
            "device": torch.cuda.get_device_name(0), "host_fp32_copy_and_numpy_ms_median": round(_stats(th)[0], 3),
            "of_which_numpy_ms_median": round(_stats(tn)[0], 3), "pack8_and_u8_copy_ms_median": round(_stats(td)[0], 3),
            "fp32_bytes": x.numel() * 4, "u8_bytes": x.numel(), "same_bytes": same, "reps": n}


def end2end_line(a):
    from PIL import Image

    tmp = tempfile.mkdtemp(prefix="grl_image8_bench_")
    try:
        rng = np.random.RandomState(0)
        lq_dir, gt_dir = os.path.join(tmp, "lq"), os.path.join(tmp, "gt")
        os.makedirs(lq_dir), os.makedirs(gt_dir)
        for i in range(a.images):
            # a smooth seeded image with some grain: compresses like a photograph rather than like noise
            small = torch.from_numpy(rng.rand(1, 3, 43, 64).astype(np.float32))
            gt = F.interpolate(small, size=(1356, 2040), mode="bicubic", align_corners=False).clamp(0, 1)
            gt = (gt + torch.from_numpy(rng.randn(1, 3, 1356, 2040).astype(np.float32)) * 0.01).clamp(0, 1)
            lq = F.interpolate(gt, size=(339, 510), mode="area")
            Image.fromarray(I.pack8(gt)[0].numpy()).save(os.path.join(gt_dir, f"im{i:02d}.png"), compress_level=1)
            Image.fromarray(I.pack8(lq)[0].numpy()).save(os.path.join(lq_dir, f"im{i:02d}.png"), compress_level=1)
        torch.manual_seed(0)
        model = GRL(**make_config("base", "sr_ckpt_df2", upscale=4)).eval().cuda()

        def run(save_dir):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                v = EV.evaluate_folder(model, lq_dir, gt_dir, 4, verbose=False, save_dir=save_dir)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, v

        run(None)                                                     # warm-up: plans, the library, the file cache
        plain, saving, same = [], [], True
        for r in range(a.rounds):
            tp, vp = run(None)
            ts, vs = run(os.path.join(tmp, f"save{r}"))
            plain.append(tp), saving.append(ts)
            same = same and vp == vs
        files = sum(len(f) for _, _, f in os.walk(os.path.join(tmp, "save0")))
        p, s = _stats(plain)[0], _stats(saving)[0]
        return {"workload": f"evaluate_folder x4, {a.images} images 339x510 -> 1356x2040, GRL-Base, with / without save_dir (LQ + HQ, 4 workers)",
                "device": torch.cuda.get_device_name(0), "plain_ms_per_image": round(p / a.images, 2),
                "saving_ms_per_image": round(s / a.images, 2), "saving_costs_ms_per_image": round((s - p) / a.images, 2),
                "plain_ms_all": [round(t, 1) for t in plain], "saving_ms_all": [round(t, 1) for t in saving], "files_written": files,
                "same_metrics": same, "rounds": a.rounds, "host_cpus": len(os.sched_getaffinity(0))}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3, help="end to end: alternating pairs of runs")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM peak the share is taken of")
    ap.add_argument("--skip-end2end", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image8_bench_line.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_image8 needs the GPU")
    def measured():
        yield from kernel_lines(a)
        yield host_line(a)
        if not a.skip_end2end:
            yield end2end_line(a)

    lines = []
    for line in measured():                                           # each line is printed and kept as soon as it is measured
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
