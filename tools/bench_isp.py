"""Times the camera-noise stage of the blind-SR degradation on the GPU (csrc/isp.hip): each of the three entries alone, eight items per
launch at the workload's sizes -- ``grl_isp_roundtrip`` on the HR crops (3 x 400 x 400), ``grl_isp_unprocess`` / ``grl_isp_process`` on
LQ images with sides 50 .. 400 -- with the item tables already on the device, and ``bsr_degrade.apply_plans`` for a batch of 8 crops of
400 at scale 4 with the plans of ``random.Random(0)``, without and with a bank (and its HR pass), alternating in the same run.
Every item uses its own tone curve (16 of the 22 tables, 64 MB, are read).  Two kinds of image: "smooth" (a colour ramp with mild
texture: neighbouring pixels index neighbouring table entries, as natural images do) and "uniform" (independent uniform values: the
gathers are scattered over the whole table).  Kernels: warm-up, then the median over --reps measurements, each the time between two
device events around --inner back-to-back launches, divided by --inner.  Bytes: what the entry must move per pixel -- the images, the
raw plane and the normals, 20 / 16 / 24 B for unprocess / process / roundtrip -- and next to it the 4-byte table gathers (3 / 3 / 6
per pixel), over the kernel time.  The tables are analytic (y = t^0.8 and its inverse): the access pattern does not depend on the
curve.  First the whole stage is checked against the float64 CPU restatement (SHADOW_STEP below says how).  With --train-step, the captured training step of bench.py's training leg is timed in the same process for scale.  One JSON
line per measurement, printed and written to --out.

    python tools/bench_isp.py [--reps 20] [--warmup 3] [--inner 10] [--train-step] [--out profiles/isp_bench_line.json]
"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import _lib, bsr_degrade as B, isp, item_lists  # noqa: E402
from tools.bench_degrade import _train_step_ms  # noqa: E402
from tools.bench_metrics import _median_ms  # noqa: E402

N, CROP, SCALE = 8, 400, 4
LQ_SIDES = [50, 100, 150, 200, 250, 300, 350, 400]
BAR = 4 * 1.002e-5                                     # the kernels' bar of tests/test_gpu_isp.py
# The check below runs the whole stage, and on images with shadows.  Where the linear value is below 1.1e-3, a step of the t^0.8 table
# times the 12.92 of the sRGB curve's linear segment exceeds the bar, so a table index one off (the reference's fp32 arithmetic has
# them against float64 as well) shows; the largest such step is the table's first, 1.58e-5 * 12.92.
SHADOW_STEP = 1.58e-5 * 12.92


def _bank():
    g = np.load(os.path.join(ROOT, "tests", "golden", "tasks", "isp.npz"))
    t = torch.linspace(0, 1, isp.TABLE_N, dtype=torch.float64)
    table = torch.stack([t ** 0.8, t ** 1.25]).float()
    return isp.CameraBank.from_arrays(g["forward1"], g["forward2"], g["curve_x"], g["curve_y"], tables={c: table for c in range(11)})


def _images(kind, sides, gen):
    out = []
    for s in sides:
        if kind == "uniform":
            out.append(torch.rand(3, s, s, generator=gen))
        else:
            y, x = torch.meshgrid(torch.arange(s) / s, torch.arange(s) / s, indexing="ij")
            out.append((torch.stack([x, y, (x + y) / 2]) * 0.8 + 0.1 + 0.02 * torch.rand(3, s, s, generator=gen)).clamp(0, 1))
    return out


def _params(bank):
    r = random.Random(1)
    ps = []
    for b in range(N):
        log_shot = r.uniform(-4, np.log10(0.006))
        ps.append(bank.params(dict(camera=b, curve=b, fw=r.random(), d_r=1.2 + 1.2 * r.random(), d_b=1.2 + 1.2 * r.random(),
                                   e=0.2 * r.random() - 0.1, shot=10 ** log_shot, read=10 ** (2.275 * log_shot + 1.47))))
    return ps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--train-step", action="store_true", help="also time the captured training step of bench.py's training leg")
    ap.add_argument("--train-steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isp_bench_line.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_isp needs the GPU")
    dev = torch.device("cuda:0")
    L = _lib.lib()
    name = torch.cuda.get_device_name(0)
    bank = _bank()
    params = _params(bank)
    tables = bank.tables(dev)
    recs = torch.stack([p.rec for p in params]).to(dev)
    gen = torch.Generator().manual_seed(0)
    lines = []

    def emit(line):
        line = dict(line, device=name, reps=a.reps, inner=a.inner)
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))

    # the whole stage (all three entries) against the float64 CPU restatement on two small items
    small = _images("smooth", [37, 64], gen)
    z = [torch.randn(s, s, generator=gen) for s in (37, 64)]
    got = isp.camera_noise([i.to(dev) for i in small], [i.to(dev) for i in small], params[:2], [n.to(dev) for n in z])
    want = isp.camera_noise([i.double() for i in small], [i.double() for i in small], params[:2], z)
    errs = torch.cat([(g.cpu().double() - w).abs().reshape(-1) for gs, ws in zip(got, want) for g, w in zip(gs, ws)])
    err, over = float(errs.max()), int((errs > BAR).sum())

    for kind in ("smooth", "uniform"):
        for entry, sides, src_planes, dst_planes, must, gathers in (("grl_isp_unprocess", LQ_SIDES, 3, 1, 20, 3), ("grl_isp_process", LQ_SIDES, 1, 3, 16, 3),
                                                                    ("grl_isp_roundtrip", [CROP] * N, 3, 3, 24, 6)):
            imgs = _images(kind, sides, gen)
            if src_planes == 1:
                imgs = [i[0] for i in imgs]
            src, so = item_lists.pack(imgs)
            src = src.to(dev)
            pixels = sum(s * s for s in sides)
            dst, do = item_lists.empty([(dst_planes, s, s) for s in sides], dev)
            normals = torch.randn(pixels, generator=gen).to(dev)
            zo = [sum(s * s for s in sides[:b]) for b in range(N)]
            table = item_lists.table([(so[b], do[b], s, s, 2 * b * isp.TABLE_N, (2 * b + 1) * isp.TABLE_N, zo[b], 0) for b, s in enumerate(sides)], dev)
            args = item_lists.args(entry, src, dst, table, params=recs.data_ptr(), tables=tables.data_ptr(), tables_elems=tables.numel(),
                                   normals=normals.data_ptr(), normals_elems=normals.numel(), C=3, max_h=max(sides), max_w=max(sides))
            fn = getattr(L, entry)

            def run():
                for _ in range(a.inner):
                    _lib.check(fn(_lib.stream_ptr(), C.byref(args)), entry)

            k = [t / a.inner for t in _median_ms(run, a.reps, a.warmup)]
            emit({"workload": f"{entry}: 8 items, sides {sides[0]} .. {sides[-1]}, {kind} images, one launch", "pixels": pixels,
                  "hip_us_median": round(k[0] * 1e3, 2), "hip_us_min": round(k[1] * 1e3, 2), "hip_us_max": round(k[2] * 1e3, 2),
                  "bytes_must_move": must * pixels, "gather_bytes": 4 * gathers * pixels,
                  "GBps_must_move": round(must * pixels / (k[0] * 1e-3) / 1e9, 1),
                  "GBps_with_gathers": round((must + 4 * gathers) * pixels / (k[0] * 1e-3) / 1e9, 1),
                  "stage_max_error_vs_float64_cpu": float(f"{err:.3e}"), "stage_values_over_bar": f"{over} of {errs.numel()}", "error_bar": BAR})

    # the pipeline without and with the stage, alternating
    x = torch.stack(_images("smooth", [CROP] * N, gen)).to(dev)
    rng = random.Random(0)
    plans0 = [B.draw_plan(rng, SCALE, CROP) for _ in range(N)]
    rng = random.Random(0)
    plans1 = [B.draw_plan(rng, SCALE, CROP, camera=bank) for _ in range(N)]
    g = torch.Generator(device=dev).manual_seed(0)
    ts = {"without": [], "with": []}
    for i in range(a.warmup + a.reps):
        for key, plans in (("without", plans0), ("with", plans1)):
            hr = x.clone() if key == "with" else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            B.apply_plans(x, plans, g, hr=hr)
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts[key].append((time.perf_counter() - t0) * 1e3)
    line = {"workload": f"apply_plans: batch {N}, crop {CROP}, scale {SCALE}, plans of random.Random(0) without / with a bank (HR pass included), "
                        "host work included, alternating",
            "camera_ops": sum(op["op"] == "camera" for p in plans1 for op in p),
            "camera_sides": [op["size"] for p in plans1 for op in p if op["op"] == "camera"]}
    for key, v in ts.items():
        v.sort()
        line.update({f"ms_median_{key}": round(v[len(v) // 2], 3), f"ms_min_{key}": round(v[0], 3), f"ms_max_{key}": round(v[-1], 3)})
    if a.train_step:
        line["train_step_ms"] = round(_train_step_ms(a.train_steps), 2)
        for key in ts:
            line[f"share_of_train_step_{key}"] = round(line[f"ms_median_{key}"] / line["train_step_ms"], 4)
    emit(line)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if over > errs.numel() / 1000 or err > BAR + SHADOW_STEP:
        raise SystemExit("bench_isp: the stage is outside its bar")


if __name__ == "__main__":
    main()
