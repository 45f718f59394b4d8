"""Times the two kernels of the x8 self-ensemble (csrc/ensemble.hip: ``grl_dihedral_pack``, ``grl_dihedral_merge``, one launch each)
on the GPU against the torch restatement they replace, and the whole wrapper against a plain forward.  One JSON line per
measurement, printed and written to --out:

  pack       ``ensemble.dihedral_pack`` of one 1 x 3 x 256 x 256 tile (the eight transformed tiles are bench.py's batch of 8) against
             ``flip`` / ``transpose`` copies of the eight transforms and a ``cat``.  ``algorithm_bytes``: 9 x the image (read once,
             written eight times)
  merge      ``ensemble.dihedral_merge`` of eight 1 x 3 x 1024 x 1024 members -- the headline tile at x4; the members are the eight
             images of ONE real GRL-Base x4 forward of batch 8, taken before the model's final ``contiguous()``: channels-last views
             with padded channels, as ``forward_infer._image`` returns them -- and of eight 1 x 3 x 1356 x 2040 members, a whole
             image at scale 1 (seeded values in views of the same pitch; the network is not run at that size here).  Against eight
             inverse copies, a ``stack`` and a ``mean`` on the same views.  ``algorithm_bytes``: 8 x the output read, 1 x written;
             ``touched_bytes`` counts whole pixels of the padded views, which is what the lines fetched hold
  wrapper    ``SelfEnsemble(GRL-Base x4)`` on one 256 x 256 tile against one plain forward of batch 8 of the same shape (bench.py's
             workload and weights regime apart): the difference is the feature's whole overhead -- two launches, and the batch made
             of one tile's transforms instead of eight tiles
  one_pixel  both kernels on a 1 x 3 x 1 x 1 image: the cost of a launch, what a small shape cannot go below

Every kernel time is the median over --reps measurements, each the time between two device events around --inner back-to-back
calls divided by --inner; kernel and restatement alternate in the same loop, so both see the same machine.  ``hbm_share`` sets
``algorithm_bytes`` against --hbm-tbs (the 8.0 TB/s peak of the MI355X; about 6.3 TB/s is achievable).  The kernels' outputs are
compared with the CPU restatement first (``torch.equal``).

    python tools/bench_ensemble.py [--reps 30] [--warmup 5] [--inner 20] [--out profiles/ensemble_bench_line.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from grl_image_restoration_amd import GRL, baseline_config, ensemble as E, forward_infer  # noqa: E402


def torch_pack(x):
    """What the kernel replaces around the model: eight copies and a cat per group."""
    a = torch.cat([E.transform(x, k).contiguous() for k in E.GROUP_A], dim=0)
    b = torch.cat([E.transform(x, k).contiguous() for k in E.GROUP_B], dim=0)
    return a, b


def torch_merge(members):
    """What the kernel replaces after the model: eight inverse copies, a stack and a mean."""
    return torch.stack([E.transform(m.float(), E.INVERSE[k]).contiguous() for k, m in enumerate(members)], dim=0).mean(dim=0)


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


def _alternate(hip, chain, a, inner=None):
    inner = inner or a.inner
    for _ in range(a.warmup):
        _events_ms(hip, inner), _events_ms(chain, inner)
    th, tc = [], []
    for _ in range(a.reps):
        th.append(_events_ms(hip, inner))
        tc.append(_events_ms(chain, inner))
    return _stats(th), _stats(tc)


def _line(workload, a, hip, chain, need, inner=None, **more):
    (h, hmin, hmax), (c, cmin, cmax) = _alternate(hip, chain, a, inner)
    line = {"workload": workload, "device": torch.cuda.get_device_name(0),
            "hip_us_median": round(h * 1e3, 2), "hip_us_min": round(hmin * 1e3, 2), "hip_us_max": round(hmax * 1e3, 2),
            "torch_us_median": round(c * 1e3, 2), "torch_us_min": round(cmin * 1e3, 2), "torch_us_max": round(cmax * 1e3, 2),
            "torch_over_hip": round(c / h, 2), "reps": a.reps, "inner": inner or a.inner}
    if need:
        line.update(algorithm_bytes=need, algorithm_tbs=round(need / (h * 1e-3) / 1e12, 3), hbm_peak_tbs=a.hbm_tbs,
                    hbm_floor_us=round(need / (a.hbm_tbs * 1e12) * 1e6, 2), hbm_share=round(need / (h * 1e-3) / 1e12 / a.hbm_tbs, 3))
    line.update(more)
    return line


def pack_line(a, shape=(1, 3, 256, 256), what="pack"):
    x = torch.rand(shape, generator=torch.Generator().manual_seed(0)).cuda()
    wa, wb = E.dihedral_pack(x.cpu())
    ga, gb = E.dihedral_pack(x)
    exact = bool(torch.equal(ga.cpu(), wa) and torch.equal(gb.cpu(), wb))
    ta, tb = torch_pack(x)
    same = bool(torch.equal(ta, ga) and torch.equal(tb, gb))
    return _line(f"{what} {'x'.join(map(str, shape))} fp32 -> 8 transforms", a, lambda: E.dihedral_pack(x), lambda: torch_pack(x),
                 9 * x.numel() * 4, equals_cpu_restatement=exact, equals_torch_chain=same)


def _padded_views(shape, pitch, seed):
    """Eight channels-last views of ``pitch`` columns per pixel holding seeded values: the layout of ``forward_infer._image``."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(8):
        h, w = (W, H) if k % 2 else (H, W)
        t = torch.zeros(B * h * w, pitch, device="cuda")
        t[:, :C] = torch.rand(B * h * w, C, generator=g).cuda()
        out.append(forward_infer._image(t, B, h, w, C))
    return out


def merge_line(a, members, what, inner=None):
    B, C, Ho, Wo = members[0].shape
    got = E.dihedral_merge(members)
    exact = bool(torch.equal(got.cpu(), E.dihedral_merge([m.cpu() for m in members])))
    close = float((torch_merge(members) - got).abs().max())
    out_bytes = got.numel() * 4
    pitch = members[0].stride(3)
    return _line(f"merge {what}: 8 x {B}x{C}x{Ho}x{Wo} {str(members[0].dtype).replace('torch.', '')} views, {pitch} columns per pixel", a,
                 lambda: E.dihedral_merge(members), lambda: torch_merge(members), 9 * out_bytes, inner,
                 touched_bytes=8 * B * Ho * Wo * pitch * members[0].element_size() + out_bytes, equals_cpu_restatement=exact,
                 max_abs_diff_to_stack_mean=close)


def grl_members(model, x):
    """The eight images of one forward of batch 8 as ``forward_infer.forward`` leaves them: views of one channels-last matrix with
    padded channels (``GRL._forward_eager`` goes on to rescale and copy them)."""
    with torch.no_grad():
        xp = model.check_image_size(x.float())
        mean = model._mean.to(xp.device, xp.dtype)
        plan = model._plan(tuple(xp.shape[2:]), xp.device)
        y = forward_infer.forward(model, (xp - mean) * model.img_range, plan)      # still in the network's range: only the layout matters
    assert not y.is_contiguous() and y.stride(1) == 1, (y.shape, y.stride())
    return [y[k : k + 1] for k in range(8)]


def wrapper_line(a, model, tile):
    x8 = torch.rand(8, *tile.shape[1:], generator=torch.Generator().manual_seed(2)).cuda()
    se = E.SelfEnsemble(model)
    with torch.no_grad():
        for _ in range(2):
            se(tile), model(x8)
        inner = 2
        (h, hmin, hmax), (c, cmin, cmax) = _alternate(lambda: se(tile), lambda: model(x8), argparse.Namespace(
            warmup=1, reps=max(5, a.reps // 3), inner=inner))
    return {"workload": f"SelfEnsemble(GRL-Base x4) on one {'x'.join(map(str, tile.shape))} tile vs one plain forward of batch 8",
            "device": torch.cuda.get_device_name(0), "self_ensemble_ms_median": round(h, 3), "self_ensemble_ms_min": round(hmin, 3),
            "self_ensemble_ms_max": round(hmax, 3), "plain_batch8_ms_median": round(c, 3), "plain_batch8_ms_min": round(cmin, 3),
            "plain_batch8_ms_max": round(cmax, 3), "overhead_ms": round(h - c, 3), "overhead_share": round((h - c) / c, 4),
            "reps": max(5, a.reps // 3), "inner": inner}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM peak the share is taken of")
    ap.add_argument("--skip-model", action="store_true", help="no GRL forward: the x4 members are seeded views, the wrapper is not timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench_line.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble needs the GPU")

    def measured():
        yield pack_line(a)
        model, pitch = None, 32
        if not a.skip_model:
            cfg = baseline_config(3)
            cfg["img_size"] = 256
            torch.manual_seed(0)
            model = GRL(**cfg).eval().cuda()
            tile = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(1)).cuda()
            members = grl_members(model, torch.cat(E.dihedral_pack(tile), dim=0))    # the eight transforms of one tile
            pitch = members[0].stride(3)
            yield merge_line(a, members, "x4 tile, real GRL-Base output")
            del members
        else:
            yield merge_line(a, _padded_views((1, 3, 1024, 1024), pitch, 3), "x4 tile, seeded")
        yield merge_line(a, _padded_views((1, 3, 1356, 2040), pitch, 4), "whole image at scale 1, seeded", inner=max(2, a.inner // 4))
        yield merge_line(a, [m.contiguous() for m in _padded_views((1, 3, 1024, 1024), pitch, 5)], "x4 tile, contiguous NCHW")
        one = torch.rand(1, 3, 1, 1).cuda()
        yield _line("one_pixel pack 1x3x1x1", a, lambda: E.dihedral_pack(one), lambda: torch_pack(one), 0)
        yield _line("one_pixel merge 8 x 1x3x1x1", a, lambda: E.dihedral_merge([one] * 8), lambda: torch_merge([one] * 8), 0)
        if model is not None:
            yield wrapper_line(a, model, tile)

    lines = []
    for line in measured():                                           # each line is printed and kept as soon as it is measured
        print(json.dumps(line), flush=True)
        lines.append(json.dumps(line))
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
