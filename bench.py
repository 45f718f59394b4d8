#!/usr/bin/env python3
"""Throughput benchmark of the GRL hot path on MI355X (contract in the task statement).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
        N > 1 and no torchrun environment: bench.py spawns the N ranks itself (one process per GPU, RCCL);
        under `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` it uses the launcher's ranks.

A plain run sets up, warms up, times the K steps and prints the headline line (metric, value, unit, ms_per_step, dtype, the
workload's configuration); nothing else runs on the GPU.  `--full` adds the untimed passes listed below to the line.
`--dump-outputs DIR` writes what the timed path returned in its last step (rank 0) as DIR/output.npy (float32), or, above 64 MB,
DIR/output_sample.npy: the same 2^23 elements of the flattened output every run (seeded draw of indices, in ascending order).

Workload (BASELINE.json configs[2], the configuration the metric is quoted on): GRL-Base x4 SR,
released-checkpoint geometry (window 32, stripes 64x64, anchor /2), batches of 256x256 LQ tiles,
synthetic uniform-random pixels, random-init weights WITH CHECKPOINT-LIKE LOGIT SCALES (round 5: the released checkpoints
sit at / around the clamp exp(ln 100), where this implementation takes its split-operand projection and the attention
offsets move more often -- the regime a user of the reference's checkpoints sees; `--random-init-scales` times the
constructor's scales instead).  One step = one forward of `--tiles` tiles per GPU with the tiles already resident in HBM.  Tiles are independent units: ranks shard them
with no data-path collective (weak scaling); the only collectives are the timing barrier/max.

The timed region contains no probes.  With --full, separate untimed passes after it collect
  roofline       : the dominant kernel (cosine window / stripe attention, MFMA-bound): algorithmic FLOPs per launch /
                   its mean launch duration from HIP events on the launching stream, against the 2.5 PFLOP/s fp16/bf16 dense peak.
                   `frac` = the kernel alone on the GPU (overlap off, `exclusive_*`); `concurrent_frac` = its residency inside the timed
                   schedule (two tile groups on two streams share the chip); `whole_network_frac` = the step's FLOPs / time / peak
  random_init_scales : the same K steps with the logit scales the reference constructor sets (10 for every head; the headline of
                   rounds 1-4) -- `trained_scales` when --random-init-scales swaps the legs
  tiled          : (N > 1) strong-scaling leg: tiling.forward_tiled of a fixed 8 x N-tile list, sharded over the ranks
                   with its RCCL all-gather
  training       : BASELINE configs[4] in short: GRL-Base x4 SR training steps on 64x64 LQ patches, batch 8 per GPU, L1 loss,
                   autograd over the HIP kernels + FusedAdamW (one launch for the 1390 tensors); N > 1: DistributedDataParallel
                   over RCCL (bucketed gradient all-reduce overlapped with the backward pass)
  cpu_baseline   : the CPU oracle (a torch-fp32 port of the reference forward) on this box's host cores: ONE FULL tile of the
                   workload (256x256 LQ for config 3: 60-120 s), thread count picked by a warm-up sweep on 64x64 tiles.
--config 2 / --config 4 measure BASELINE configs[1] / configs[3] (Small denoise 128x128; Base deblur 384x384 tiles) with
the same harness (their lines are kept under profiles/).
"""
import argparse
import json
import math
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_F16_TFLOPS = 2500.0  # MI355X dense fp16 / bf16 MFMA (MI355X_MICROARCH.md)

WORKLOADS = {
    # config id -> (baseline_config index, tile side, label, GFLOP per tile or None)
    3: (3, 256, "BASELINE configs[2]: GRL-Base x4 SR, 256x256 LQ tiles, ckpt geometry (window 32, stripe 64x64, anchor /2)", 5468.5),
    2: (2, 128, "BASELINE configs[1]: GRL-Small denoise sigma 25, 128x128 tiles, dn geometry (window 16, stripe 64x128, anchor /4)", 181.0),
    4: (4, 384, "BASELINE configs[3]: GRL-Base motion deblur, 384x384 tiles of a 1280x720 frame (window 12, stripe 48x96, anchor /4)", None),
}


def attention_launches(prof):
    """durations of the forward attention launches of an ops.profile_end() record (labelled per geometry: 'attention q.. k..')"""
    return [t for k, v in prof.items() if k.startswith("attention ") or k == "attention" for t in v]


def attention_flops_per_launch(cfg, tiles, hw):
    """each of the three attention launches of a block (window, anchors->
    stripe, stripe->anchors) does 2 * L * N_keys * C FLOPs per tile (QK^T + PV over C/2 channels)."""
    L = hw[0] * hw[1]
    C = cfg["embed_dim"]
    ws = cfg["window_size"]
    df = cfg["anchor_window_down_factor"]
    n_w = ws * ws
    n_anchor = (cfg["stripe_size"][0] // df) * (cfg["stripe_size"][1] // df)
    win = 2 * L * n_w * C
    a2w = 2 * L * n_anchor * C
    return tiles * (win + 2 * a2w) / 3.0  # mean over the three launches of a block


def cpu_baseline(cfg, side):
    """Reference algorithm on the host cores: oracle/grl_oracle.py (kind 'port': a torch-fp32 restatement pinned against the
    unmodified reference; the reference sources themselves do not travel to the GPU box).  One full tile of the metric's own
    configuration (256x256 LQ for config 3): nothing is extrapolated.  Thread count from a sweep on a 64x64 tile."""
    from oracle import grl_oracle as O

    from grl_image_restoration_amd import GRL

    torch.manual_seed(0)

    def make(sd_side):
        c = dict(cfg)
        c["img_size"] = sd_side
        m = GRL(**c)
        return c, {k: v.detach().clone() for k, v in m.state_dict().items()}

    def run(c, sd, sd_side):
        x = torch.rand(1, 3, sd_side, sd_side, generator=torch.Generator().manual_seed(1))
        t0 = time.time()
        with torch.no_grad():
            O.grl_forward(x, c, sd)
        return time.time() - t0

    ncpu = os.cpu_count() or 1
    c64, sd = make(64)
    sweep = {}
    for th in sorted({min(ncpu, t) for t in (8, 16, 32, 64)}):
        torch.set_num_threads(th)
        run(c64, sd, 64) if not sweep else None   # first call: page-in / allocator warm-up
        sweep[th] = run(c64, sd, 64)
    best = min(sweep, key=sweep.get)
    torch.set_num_threads(best)
    cfull, _ = make(side)
    dt = run(cfull, sd, side)     # (the thread sweep above has paged everything in; one forward: 60 .. 120 s for a 256x256 Base tile)
    return {
        "value": round(side * side / dt / 1e6, 6),
        "unit": "LQ megapixels/s",
        "cores": best,
        "host_cpus": ncpu,
        "kind": "port",
        "thread_sweep_s_per_64x64_tile": {str(k): round(v, 2) for k, v in sweep.items()},
        "sample": f"one full {side}x{side} LQ tile of the benchmark configuration (same network / window / stripe geometry, fp32 torch CPU, "
                  f"{best} threads after a warm-up + thread sweep on 64x64 tiles): {dt:.1f} s per forward; nothing extrapolated",
    }


def measure_attention_traffic(tiles):
    """HBM bytes per attention launch from the PMC counters, measured in THIS run: two rocprofv3 passes
    (--pmc FETCH_SIZE, --pmc WRITE_SIZE: separate passes, --kernel-trace only, as the MI355X guide's HBM section prescribes) over the
    per-kernel micro-benchmark (tools/bench_kernels.py: the three attention launches of one block on `tiles` tiles of the bench's
    shape).  Units: KiB; FETCH_SIZE doubled on gfx950 (the guide's correction for 16-B-per-lane streaming loads).  None when
    rocprofv3 is not on the box or a pass fails -- the caller then quotes the stored figure of profiles/attention_traffic.json."""
    import shutil
    import sqlite3
    import subprocess
    import tempfile

    if shutil.which("rocprofv3") is None:
        return None
    got = {}
    try:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = tempfile.mkdtemp(prefix="grl_pmc_", dir="/tmp")
            cmd = ["rocprofv3", "--kernel-trace", "--pmc", counter, "-d", d, "-o", "r", "--", sys.executable,
                   os.path.join(ROOT, "tools", "bench_kernels.py"), "--tiles", str(tiles), "--iters", "2", "--only", "attn_window,attn_a2w,attn_w2a"]
            subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           timeout=240, check=True)
            dbs = [os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs if f.endswith(".db")]
            cur = sqlite3.connect(dbs[0]).cursor()
            tabs = [r[0] for r in cur.execute("select name from sqlite_master where type='table'")]
            pick = lambda pre: [t for t in tabs if t.startswith(pre)][0]
            ev, info, kd, ks = pick("rocpd_pmc_event"), pick("rocpd_info_pmc"), pick("rocpd_kernel_dispatch"), pick("rocpd_info_kernel_symbol")
            cols = [r[1] for r in cur.execute(f"pragma table_info({kd})")]
            key = "event_id" if "event_id" in cols else "id"
            rows = cur.execute(
                f"select s.kernel_name, count(*), avg(v) from (select e.event_id as eid, e.pmc_id as pid, sum(e.value) as v from {ev} e "
                f"group by e.event_id, e.pmc_id) x join {info} i on x.pid = i.id join {kd} d on d.{key} = x.eid join {ks} s on d.kernel_id = s.id "
                f"where i.name = '{counter}' and s.kernel_name like '%attn_rows_kernel%' group by s.kernel_name").fetchall()
            n = sum(r[1] for r in rows)
            got[counter] = sum(r[1] * r[2] for r in rows) / n
            shutil.rmtree(d, ignore_errors=True)
        return {"bytes_per_launch": int((2.0 * got["FETCH_SIZE"] + got["WRITE_SIZE"]) * 1024), "FETCH_SIZE_KiB_mean": round(got["FETCH_SIZE"], 1),
                "WRITE_SIZE_KiB_mean": round(got["WRITE_SIZE"], 1), "tiles_per_launch": tiles}
    except Exception as e:      # noqa: BLE001 -- a missing counter, a changed schema, a timeout: report the stored figure instead
        return {"error": f"{type(e).__name__}: {e}"[:200]}


def timed_steps(model, x, steps, world):
    with torch.no_grad():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            y = model(x)
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=x.device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt, y


DUMP_MAX_BYTES = 64 << 20
DUMP_SAMPLE = 1 << 23


def dump_outputs(out_dir, y):
    """The timed path's output as float32 .npy: whole when it fits DUMP_MAX_BYTES, else a fixed seeded sample of it."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    y = y.detach().float()
    if y.numel() * 4 <= DUMP_MAX_BYTES:
        np.save(os.path.join(out_dir, "output.npy"), y.cpu().numpy())
        return
    idx = torch.randint(y.numel(), (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
    np.save(os.path.join(out_dir, "output_sample.npy"), y.reshape(-1)[idx.to(y.device)].cpu().numpy())


def training_leg(args, dev, rank, world):
    """A few optimizer steps of BASELINE configs[4] (reference: engines/base.py:221-236, tools/trainer.py:135-142,
    config/optimizer/adamw.yaml, config/loss/l1.yaml) on synthetic pairs."""
    from grl_image_restoration_amd import GRL, FusedAdamW, baseline_config, ddp, ops

    cfg = baseline_config(5)
    bsz, side, sc = args.train_batch, 64, cfg["upscale"]
    g = torch.Generator().manual_seed(100 + rank)
    lq = torch.rand(bsz, 3, side, side, generator=g).to(dev)
    gt = torch.rand(bsz, 3, side * sc, side * sc, generator=g).to(dev)

    def fresh():
        torch.manual_seed(0)
        m = GRL(**cfg).to(dev).train()
        return m, FusedAdamW(m.parameters(), lr=2e-4, weight_decay=1e-4)

    def eager_stepper(net, opt):
        def step():
            opt.zero_grad(set_to_none=True)
            loss = (net(lq) - gt).abs().mean()
            loss.backward()
            opt.step()
            return loss
        return step

    # The whole step replayed from captured HIP graphs -- eager, the ~19 k launches of a step are host-bound (train_graph.py).  One
    # GPU: ONE graph (forward, L1, backward, FusedAdamW), the eager time of the same step reported next to it.  Replicas: graph A
    # (forward .. flat gradient buffer), one RCCL all-reduce, graph B (FusedAdamW); if that path fails on this node the leg falls
    # back to the eager DistributedDataParallel step and says so.
    graphed, eager_ms, graph_error = None, None, None
    model, opt = fresh()
    if not args.no_train_graph:
        from grl_image_restoration_amd import GraphedTrainStep

        try:
            if world == 1:
                step = eager_stepper(model, opt)
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(2):
                    step()
                torch.cuda.synchronize()
                eager_ms = (time.perf_counter() - t0) / 2 * 1e3
            graphed = GraphedTrainStep(model, opt, lambda y, t: (y - t).abs().mean(), lq, gt, warmup=1 if world == 1 else 3)
            for _ in range(2):
                graphed(lq, gt)
            run = lambda: graphed(lq, gt)
        except Exception as e:          # noqa: BLE001 -- (only the multi-GPU path is allowed to fall back: it has never met N > 1 ranks)
            if world == 1:
                raise
            graphed, graph_error = None, f"{type(e).__name__}: {e}"[:300]
            torch.cuda.synchronize()
            model, opt = fresh()
    if world > 1 and not args.no_train_graph:      # the ranks fall back together or not at all
        bad = torch.tensor([0.0 if graphed is not None else 1.0], device=dev)
        dist.all_reduce(bad, op=dist.ReduceOp.MAX)
        if bad.item() > 0 and graphed is not None:
            graphed, graph_error = None, "another rank could not capture the step"
            model, opt = fresh()
    if graphed is None:
        net = ddp.wrap(model, device=dev, bucket_mb=32) if world > 1 else model
        step = run = eager_stepper(net, opt)
        for _ in range(2):
            step()
    else:
        step = eager_stepper(model, opt) if world == 1 else None
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.train_steps):
        loss = run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    assert math.isfinite(float(loss.detach()))
    if graphed is not None:
        graphed.finish()
    ops.profile_begin()
    if step is not None:
        step()
    else:                       # replicas on the graphed path: the per-kernel probe step is an eager one of the same class
        graphed._eager_step()
    prof = ops.profile_end()
    kern = {k: round(sum(v), 3) for k, v in sorted(prof.items(), key=lambda kv: -sum(kv[1]))}
    # dominant kernel pair of the step: attention backward (attn_dq_kernel + attn_dkv_kernel, one "attention_bwd" probe each).
    # Algorithmic work = 5 contractions (S recomputed, dP, dV, dK, dQ) against the forward's 2 (QK^T, PV).
    bwd = prof.get("attention_bwd", [])
    bwd_ms = sum(bwd) / max(len(bwd), 1)
    fl_bwd = 2.5 * attention_flops_per_launch(cfg, bsz, (side, side))
    ach = fl_bwd / (bwd_ms * 1e-3) / 1e12 if bwd_ms > 0 else 0.0
    roof = {"kernel": "attn_dq_kernel + attn_dkv_kernel (attention backward, recompute-S)", "bound": "mfma", "achieved": round(ach, 2),
            "peak": PEAK_F16_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_F16_TFLOPS, 4), "traffic": None,
            "launches_timed": len(bwd), "mean_launch_ms": round(bwd_ms, 4), "flops_per_launch": fl_bwd,
            "share_of_hip_kernel_time": round(sum(bwd) / max(sum(sum(v) for v in prof.values()), 1e-9), 3)}
    return {
        "workload": "BASELINE configs[4]: GRL-Base x4 SR training, 64x64 LQ synthetic pairs, L1 loss, FusedAdamW(lr 2e-4, wd 1e-4)",
        "batch_per_gpu": bsz, "steps": args.train_steps, "ms_per_step": round(dt / args.train_steps * 1e3, 2),
        "step_mode": ("eager" if graphed is None else "one captured HIP graph per step (forward + L1 + backward + FusedAdamW), replayed"
                      if world == 1 else "two captured HIP graphs per step (forward + L1 + backward + flat gradients | FusedAdamW) around "
                      "one RCCL all-reduce of the flat fp32 gradient buffer"),
        "graph_fallback": graph_error,
        "eager_ms_per_step": round(eager_ms, 2) if eager_ms is not None else None,
        "samples_per_s": round(world * bsz * args.train_steps / dt, 2),
        "value": round(world * bsz * side * side * args.train_steps / dt / 1e6, 4), "unit": "LQ megapixels/s (training)",
        "parallelism": ("single GPU" if world == 1 else f"data-parallel replicas x{world}, one flat gradient all-reduce per step over RCCL"
                        if graphed is not None else f"DDP x{world} over RCCL, 32 MB gradient buckets"),
        "hip_kernel_ms_per_step": kern, "roofline": roof, "final_loss": round(float(loss.detach()), 5),
    }


def run(args, rank, world, local_rank):
    if world > 1:
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    dev = torch.device("cuda", local_rank if world > 1 else 0)
    torch.cuda.set_device(dev)

    from grl_image_restoration_amd import GRL, baseline_config, ops, tiling

    ci, side, label, gflop_tile = WORKLOADS[args.config]
    cfg = baseline_config(ci)
    cfg["img_size"] = side
    torch.manual_seed(0)
    model = GRL(**cfg).eval().to(dev)
    g = torch.Generator(device="cpu").manual_seed(1 + rank)
    x = torch.rand(args.tiles, 3, side, side, generator=g).to(dev)
    scale = cfg["upscale"]

    # The timed leg runs on CHECKPOINT-LIKE logit scales (round 5): every released checkpoint of the reference has its
    # logit scales at / around the clamp exp(min(., ln 100)) (efficient.py:39), where the q / k / anchor projection runs on split operands
    # and the lazy softmax offsets of the attention kernel move more often.  Same seeded draw as the *_hiscale parity fixtures.  The
    # random-init scales (10 for every head) are the secondary leg `random_init_scales`.
    scale_params = [(n, p_) for n, p_ in model.named_parameters() if n.endswith("logit_scale")]
    init_scales = [p_.detach().clone() for _, p_ in scale_params]
    trained_regime = not args.random_init_scales
    if trained_regime:
        gs = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for _, p_ in scale_params:
                p_.copy_((math.log(100.0) + 0.3 * torch.randn(p_.shape, generator=gs)).to(dev))
    with torch.no_grad():
        for _ in range(args.warmup):
            y = model(x)
    dt, y = timed_steps(model, x, args.steps, world)
    assert torch.isfinite(y).all()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, y)
    precision_mode = model.precision   # (of the timed leg: `auto` is resolved per weight set, the other leg may differ)
    cal = getattr(model, "calibration", None)
    calibration = None
    if cal:     # precision `auto` on the wide SR models: per-block choice by measurement (GRL._calibrated_plan)
        calibration = {k: (float(f"{v:.3g}") if isinstance(v, float) else v) for k, v in cal.items() if k != "split_blocks"}
        calibration["rule"] = ("a fixed smooth probe image through the all-split network and through the fp16-operand one; blocks move to split "
                               "operands, costliest first, until max <= bar_max and rms <= bar_rms on the probe (tests: five weight draws of "
                               "this configuration + one at this tile size hold 1e-3 against the float64 reference in this mode)")

    # ---- untimed passes of --full (rank 0 measures; every rank runs the same launches so that the barriers match) ----
    groups = model.stream_groups(args.tiles)   # tile groups advancing on separate HIP streams (one launch = one group)
    excl = {}
    if args.full:
        with torch.no_grad():
            ops.profile_begin()
            dt_probe, _ = timed_steps(model, x, args.steps, world)
            prof = ops.profile_end()
            if groups > 1:
                os.environ["GRL_SPLIT_STREAMS"] = "1"
                model(x)
                torch.cuda.synchronize()
                ops.profile_begin()
                model(x)
                p1 = ops.profile_end()
                del os.environ["GRL_SPLIT_STREAMS"]
                a1 = attention_launches(p1)
                if a1:
                    ms1 = sum(a1) / len(a1)
                    fl1 = attention_flops_per_launch(cfg, args.tiles, (side, side))
                    excl = {"exclusive_mean_launch_ms": round(ms1, 4), "exclusive_tiles_per_launch": args.tiles,
                            "exclusive_achieved": round(fl1 / (ms1 * 1e-3) / 1e12, 2),
                            "exclusive_frac": round(fl1 / (ms1 * 1e-3) / 1e12 / PEAK_F16_TFLOPS, 4)}

    # the other logit-scale regime, same K steps
    other = None
    if args.full and not args.no_other_scales:
        with torch.no_grad():
            if trained_regime:
                for (_, p_), v in zip(scale_params, init_scales):
                    p_.copy_(v)
            else:
                gs = torch.Generator().manual_seed(7)
                for _, p_ in scale_params:
                    p_.copy_((math.log(100.0) + 0.3 * torch.randn(p_.shape, generator=gs)).to(dev))
            for _ in range(max(1, args.warmup)):
                yt = model(x)
        dt_t, yt = timed_steps(model, x, args.steps, world)
        assert torch.isfinite(yt).all()
        other = {"ms_per_step": round(dt_t / args.steps * 1e3, 3), "value": round(world * args.tiles * side * side * args.steps / dt_t / 1e6, 4),
                 "unit": "LQ megapixels/s", "ratio_to_timed_leg": round(dt_t / dt, 4), "precision_mode": model.precision,
                 "logit_scales": "as initialised by the reference constructor (10 for every head)" if trained_regime else
                                 "exp(min(ln 100 + 0.3 N(0,1), ln 100)): about half of the heads at the clamp"}

    # what the other precision modes cost on the timed leg's weights (same tiles, fewer steps): every contraction on split operands
    # (`high`: 5e-6 from the float64 reference) and, when the calibration moved blocks, plain fp16 operands everywhere
    precision_legs = None
    if args.full and not args.no_precision_legs and args.config == 3 and world == 1:
        with torch.no_grad():                      # the timed leg's logit scales again (the leg above swapped them)
            gs = torch.Generator().manual_seed(7)
            for (_, p_), v in zip(scale_params, init_scales):
                p_.copy_((math.log(100.0) + 0.3 * torch.randn(p_.shape, generator=gs)).to(dev) if trained_regime else v)
        precision_legs = {}
        n_leg = max(2, min(args.steps, 6))
        for name, env, arg in (("high", {}, "high"), ("fp16_operands_uncalibrated", {"GRL_CALIBRATE": "0"}, "auto")):
            if name != "high" and not (cal and cal.get("split", 0) > 0):
                continue
            os.environ.update(env)
            m2 = GRL(**cfg, precision=arg).eval().to(dev)
            m2.load_state_dict(model.state_dict(), strict=True)
            with torch.no_grad():
                m2(x)
            dt2, _ = timed_steps(m2, x, n_leg, 1)
            precision_legs[name] = {"ms_per_step": round(dt2 / n_leg * 1e3, 3), "ratio_to_timed_leg": round(dt2 / n_leg / (dt / args.steps), 3),
                                    "precision_mode": m2.precision, "steps": n_leg}
            for k_ in env:
                os.environ.pop(k_, None)
            del m2
        torch.cuda.empty_cache()

    # strong-scaling leg: one fixed tile list sharded over the ranks, stitched through the RCCL all-gather
    tiled = None
    if args.full and world > 1 and not args.no_tiled:
        n_t = 8 * world
        cols = 8
        rows = n_t // cols
        frame = torch.rand(1, 3, rows * side, cols * side, generator=torch.Generator().manual_seed(3)).to(dev)   # same on every rank
        with torch.no_grad():
            tiling.forward_tiled(model, frame, side, 0, scale, tile_batch=args.tiles)
            dt_s, _ = timed_steps(lambda f: tiling.forward_tiled(model, f, side, 0, scale, tile_batch=args.tiles), frame, 3, world)
        tiled = {"tiles": n_t, "ms_per_frame": round(dt_s / 3 * 1e3, 3),
                 "value": round(n_t * side * side * 3 / dt_s / 1e6, 4), "unit": "LQ megapixels/s", "scaling": "strong",
                 "collective": f"all_gather_into_tensor of {n_t // world} x (3, {side * scale}, {side * scale}) fp32 tiles per rank (RCCL)"}

    training = None
    if args.full and not args.no_train and args.config == 3:
        del model, x, y
        torch.cuda.empty_cache()
        try:      # a secondary leg: its failure is reported in the line, it does not take the headline measurement down with it
            training = training_leg(args, dev, rank, world)
        except Exception as e:      # noqa: BLE001
            training = {"error": f"{type(e).__name__}: {e}"[:400]}

    if rank == 0:
        mp = world * args.tiles * side * side * args.steps / dt / 1e6
        conf = {
            "workload": label + (", random-init weights with checkpoint-like logit scales exp(min(ln 100 + 0.3 N(0,1), ln 100)): about half of the heads at "
                                 "the clamp, the regime of every released checkpoint" if trained_regime else ", random-init weights and logit scales (10)"),
            "logit_scale_regime": "checkpoint-like" if trained_regime else "random-init",
            "tiles_per_gpu_per_step": args.tiles,
            "hr_megapixels_per_s": round(mp * scale * scale, 2),
            "parallelism": f"tile-sharded x{world}, no data-path collective",
            "precision_mode": precision_mode,
            "precision_calibration": calibration,
        }
        if gflop_tile:
            conf.update(gflop_per_tile=gflop_tile, model_tflops=round(gflop_tile * 1e9 * world * args.tiles * args.steps / dt / 1e12, 2))
        roofline = None
        if args.full:
            att = attention_launches(prof)
            att_ms = sum(att) / max(len(att), 1)
            fl = attention_flops_per_launch(cfg, args.tiles // groups, (side, side))
            ach = fl / (att_ms * 1e-3) / 1e12 if att_ms > 0 else 0.0
            traffic, traffic_source = None, None
            tpath = os.path.join(ROOT, "profiles", "attention_traffic.json")
            live = measure_attention_traffic(args.tiles // groups) if (args.config == 3 and world == 1 and not args.no_traffic) else None
            if live and "bytes_per_launch" in live:
                traffic = live["bytes_per_launch"]
                traffic_source = (f"measured in this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (separate passes) over tools/bench_kernels.py, "
                                  f"{live['tiles_per_launch']} tiles per launch, mean of the three attention launches of a block; KiB units, FETCH_SIZE x2 (gfx950): "
                                  f"FETCH {live['FETCH_SIZE_KiB_mean']} KiB, WRITE {live['WRITE_SIZE_KiB_mean']} KiB")
            elif args.config == 3 and os.path.isfile(tpath):
                traffic = json.load(open(tpath)).get("hbm_bytes_per_tile")  # PMC pass (profiles/), per tile
                traffic = traffic * (args.tiles // groups) if traffic else None
                traffic_source = ("profiles/attention_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of an earlier profile run, not measured in "
                                  "this run" + (f": {live['error']}" if live and "error" in live else ": rocprofv3 not available or --no-traffic") + ")")
            # Roofline of the dominant kernel.  `frac` is the kernel alone on the GPU (the `exclusive` pass: overlap off, one launch per
            # attention call over all tiles) -- what the kernel is capable of; `concurrent_frac` is its per-launch residency inside the timed
            # schedule, where a launch shares the GPU with the other tile group's kernels and therefore understates it; `whole_network_frac`
            # prices the whole step's algorithmic FLOPs (5468.5 GFLOP per tile) against the same peak.
            roofline = {
                # the row-streaming kernel serves the 32-aligned geometry of config 3; the window-12 / -16 geometries of configs 2 and 4
                # run the generic kernel (grl_attention_fwd's dispatch, csrc/attention.hip)
                "kernel": "attn_rows_kernel (cosine window / anchored-stripe attention, csrc/attention_rows.hip)" if args.config == 3 else
                          "attn_kernel (generic cosine window / anchored-stripe attention, csrc/attention.hip)",
                "bound": "mfma",
                # `achieved` / `frac`: the kernel's mean launch duration measured live in the step's own schedule (HIP events on the
                # launching streams of a repeat of the timed region) -- with two tile groups on two streams a launch shares the GPU with
                # the other group's kernels; `exclusive_*` below: the kernel alone on the GPU; `whole_network_frac`: the step's FLOPs
                "whole_network_frac": round(gflop_tile * 1e9 * world * args.tiles * args.steps / dt / 1e12 / PEAK_F16_TFLOPS, 4) if gflop_tile else None,
                "achieved": round(ach, 2),
                "peak": PEAK_F16_TFLOPS,
                "unit": "TFLOP/s",
                "frac": round(ach / PEAK_F16_TFLOPS, 4),
                "frac_is": "in the timed schedule (two tile groups on two HIP streams share the GPU)" if groups > 1 else "in the timed schedule (one stream)",
                "concurrent_achieved": round(ach, 2),
                "concurrent_frac": round(ach / PEAK_F16_TFLOPS, 4),
                "logit_scale_regime": "checkpoint-like" if trained_regime else "random-init",
                "traffic": traffic,
                "traffic_source": traffic_source,
                "algorithmic_bytes_per_launch": int(37.65e6 * (args.tiles // groups)) if args.config == 3 else None,
                "launches_timed": len(att),
                "mean_launch_ms": round(att_ms, 4),
                "flops_per_launch": fl,
                "probe_pass_ms_per_step": round(dt_probe / args.steps * 1e3, 3),
                "time_share_of_step": round(sum(att) / (dt_probe * 1e3), 3) if att else None,
                "time_share_note": "sum of the launches' own durations / step time; the tile groups run on concurrent streams, so launches overlap "
                                   "and the shares of all kernels add up to more than 1" if groups > 1 else None,
                "concurrent_streams": groups,
                "tiles_per_launch": args.tiles // groups,
                **excl,
            }
        line = {
            "metric": "LQ megapixels/s, " + label.split(":")[1].split(",")[0].strip() + f", {side}x{side} LQ tiles",
            "value": round(mp, 4),
            "unit": "LQ megapixels/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f16 MFMA operands (attention, linear, conv), f32 accumulate + residual stream",
            "data": "synthetic",
            "config": conf,
        }
        if roofline:
            line["roofline"] = roofline
        if other:
            line["random_init_scales" if trained_regime else "trained_scales"] = other
        if precision_legs:
            line["precision_legs"] = precision_legs
        if tiled:
            line["tiled"] = tiled
        if training:
            line["training"] = training
        if args.full and not args.no_cpu_baseline and world == 1:      # rank 0 at N = 1 only: the other ranks would sit in the barrier
            line["cpu_baseline"] = cpu_baseline(cfg, side if not args.cpu_baseline_side else args.cpu_baseline_side)
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _spawned(local_rank, args, world, port):
    os.environ.update(RANK=str(local_rank), LOCAL_RANK=str(local_rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    run(args, local_rank, world, local_rank)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tiles", type=int, default=8, help="LQ tiles per GPU per step")
    ap.add_argument("--config", type=int, default=3, choices=sorted(WORKLOADS), help="BASELINE config (3 = the metric's)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-side", type=int, default=0, help="tile side of the CPU baseline leg (default: the workload's own tile)")
    ap.add_argument("--random-init-scales", action="store_true", help="time the random-init logit scales (the pre-round-5 headline) instead of checkpoint-like ones")
    ap.add_argument("--no-other-scales", "--no-trained-scales", dest="no_other_scales", action="store_true", help="skip the leg on the other logit-scale regime")
    ap.add_argument("--no-train-graph", action="store_true", help="training leg: eager steps instead of the captured HIP graph")
    ap.add_argument("--no-tiled", action="store_true")
    ap.add_argument("--no-precision-legs", action="store_true", help="skip timing the other precision modes on the timed leg's weights")
    ap.add_argument("--no-traffic", action="store_true", help="do not run the two rocprofv3 --pmc passes that measure roofline.traffic")
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--train-steps", type=int, default=3)
    ap.add_argument("--train-batch", type=int, default=8, help="64x64 LQ patches per GPU per training step")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the untimed passes (roofline, other logit scales, precision legs, tiled, training, "
                         "CPU baseline); the --no-* options above select among them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the timed path's output of its last step (rank 0) as float32 .npy under DIR (a fixed seeded sample above 64 MB)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    env_world = os.environ.get("WORLD_SIZE")
    if env_world is not None:                       # launched by torch.distributed.run
        world = int(env_world)
        if world != args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        run(args, int(os.environ.get("RANK", "0")), world, int(os.environ.get("LOCAL_RANK", "0")))
    elif args.gpus > 1:                             # plain `python bench.py --gpus N`: spawn the ranks here
        n_dev = torch.cuda.device_count()
        if n_dev < args.gpus:
            raise SystemExit(f"bench.py: --gpus {args.gpus} but only {n_dev} GPU(s) visible")
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        import torch.multiprocessing as mp

        mp.spawn(_spawned, args=(args, args.gpus, port), nprocs=args.gpus, join=True)
    else:
        run(args, 0, 1, 0)


if __name__ == "__main__":
    main()
