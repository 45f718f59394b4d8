"""GPU tests of ``grl_batch_remix`` (csrc/remix.hip) against the torch restatement on the CPU, bit for bit; the argument errors;
a captured launch that follows its table; and ``train`` across a stage boundary, captured and eager."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import _lib as L
from grl_image_restoration_amd import ops
from grl_image_restoration_amd import remix as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def pair(shape_lq, scale, cg=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    B, Cl, P, _ = shape_lq
    return torch.randn(shape_lq, generator=g), torch.randn((B, cg or Cl, P * scale, P * scale), generator=g)


def mix_plan(idx, x0, y0, b, seed=0):
    gen = torch.Generator().manual_seed(seed)
    drawn = R.draw_remix(random.Random(seed), gen, b, 1, b, 1, True)        # no progressive draw: only perm and lam
    return R.RemixPlan(idx, x0, y0, drawn.perm, drawn.lam)


def both(lq, gt, plan, scale, patch, to_dev=lambda t: t.to(DEV)):
    want = R.batch_remix(lq, gt, plan, scale, patch=patch)
    got = R.batch_remix(to_dev(lq), to_dev(gt), plan, scale, patch=patch)
    assert all(t.is_cuda and t.is_contiguous() for t in got)
    return [t.cpu() for t in got], want


CASES = {
    # every row misaligned against its output, odd widths, 2 of 3 selected
    "odd_crop": (pair((3, 3, 8, 8), 2), 2, 5, lambda: mix_plan((2, 0), 1, 2, 2)),
    "dual_pixel": (pair((2, 6, 7, 7), 1, cg=3), 1, 7, lambda: mix_plan(None, 0, 0, 2, seed=1)),
    "one_channel_x3": (pair((2, 1, 5, 5), 3), 3, 3, lambda: mix_plan((1, 0), 2, 1, 2, seed=2)),
    "one_channel_x4": (pair((2, 1, 5, 5), 4), 4, 3, lambda: mix_plan((1,), 1, 2, 1, seed=3)),
    # p a multiple of 4 at y0 = 0 in 16-byte aligned rows: the all-vector path
    "all_vector": (pair((3, 3, 16, 16), 2), 2, 8, lambda: mix_plan((0, 2), 3, 0, 2, seed=4)),
    # aligned source rows against a window four columns in: vector rows with a shifted source
    "vector_shifted": (pair((2, 3, 16, 16), 1), 1, 12, lambda: mix_plan(None, 1, 4, 2, seed=5)),
    "mixup_only_64_x4": (pair((8, 3, 64, 64), 4), 4, 64, lambda: mix_plan(None, 0, 0, 8, seed=6)),
    "select_and_crop_only": (pair((4, 3, 12, 12), 2), 2, 7, lambda: R.RemixPlan((3, 1, 0), 5, 2, None, None)),
    "more_than_one_block": (pair((2, 3, 40, 40), 1), 1, 33, lambda: mix_plan((1, 0), 7, 3, 2, seed=7)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_the_cpu_restatement(name):
    (lq, gt), scale, p, plan = CASES[name]
    got, want = both(lq, gt, plan(), scale, p)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_channels_last_and_sliced_sources():
    (lq, gt), plan = pair((3, 3, 8, 8), 2), mix_plan((2, 0), 1, 2, 2)
    want = R.batch_remix(lq, gt, plan, 2, patch=5)

    def channels_last(t):
        return t.to(DEV).contiguous(memory_format=torch.channels_last)

    def sliced(t):      # the batch sits inside a larger tensor: every stride differs from the contiguous one
        B, C_, H, W = t.shape
        big = torch.full((B + 1, C_ + 2, H + 3, W + 5), float("nan"), device=DEV)
        view = big[1:, 1 : 1 + C_, 2 : 2 + H, 3 : 3 + W]
        view.copy_(t)
        return view

    for to_dev in (channels_last, sliced):
        a, b = to_dev(lq), to_dev(gt)
        assert not a.is_contiguous() and not b.is_contiguous()
        got = R.batch_remix(a, b, plan, 2, patch=5)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


def test_copy_mode_reads_neither_lam_nor_the_partner():
    lq, gt = pair((3, 3, 8, 8), 2)
    table = torch.tensor([[2, 1 << 30, 1, 2, 0], [0, -7, 1, 2, 0]], dtype=torch.int32)      # src_b far outside the batch
    table[:, 4] = torch.tensor([float("nan")] * 2).view(torch.int32)                        # lam poisoned
    a, b = torch.empty(2, 3, 5, 5, device=DEV), torch.empty(2, 3, 10, 10, device=DEV)
    ops.batch_remix(lq.to(DEV), gt.to(DEV), table.to(DEV), 2, 5, 2, False, a, b)
    want = R.batch_remix(lq, gt, R.RemixPlan((2, 0), 1, 2, None, None), 2, patch=5)
    assert torch.equal(a.cpu(), want[0]) and torch.equal(b.cpu(), want[1])


def test_nan_inf_and_denormals_propagate_as_on_the_cpu():
    lq, gt = pair((4, 3, 8, 8), 2, seed=3)
    special = torch.tensor([float("nan"), float("inf"), float("-inf"), 1e-40, -3e-42, 1.1754944e-38, 3.4e38, -0.0])
    lq.view(-1)[:: 7][: 8 * 13] = special.repeat(13)
    gt.view(-1)[:: 11][: 8 * 20] = special.flip(0).repeat(20)
    for plan, p in ((mix_plan((3, 1, 0), 0, 0, 3, seed=8), 8), (mix_plan(None, 2, 1, 4, seed=9), 6)):
        got, want = both(lq, gt, plan, 2, p)
        assert any(bool(w.isnan().any()) for w in want) and all(bool(w.isinf().any()) for w in want)
        assert any(bool(((w.abs() < 1.1754944e-38) & (w != 0)).any()) for w in want)        # denormal results
        for g, w in zip(got, want):
            nan = w.isnan()
            assert torch.equal(g.isnan(), nan)
            # bit for bit outside the NaNs (torch.equal would also pass -0.0 for 0.0)
            assert torch.equal(g[~nan].view(torch.int32), w[~nan].view(torch.int32))


@pytest.mark.parametrize("pad", [1, 3, 4])
def test_out_views_inside_larger_buffers_keep_their_border(pad):
    (lq, gt), scale, p = pair((3, 3, 9, 9), 3), 3, 5
    plan = mix_plan((1, 2), 3, 4, 2, seed=pad)
    want = R.batch_remix(lq, gt, plan, scale, patch=p)
    outs, bufs = [], []
    for shape in ((2, 3, p, p), (2, 3, scale * p, scale * p)):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * pad + 1,), -12345.0, device=DEV)
        bufs.append(buf)
        outs.append(buf[pad : pad + n].view(shape))                 # contiguous, `pad` floats off its 16-byte line
    got = R.batch_remix(lq.to(DEV), gt.to(DEV), plan, scale, out=tuple(outs))
    assert got[0].data_ptr() == outs[0].data_ptr() and got[1].data_ptr() == outs[1].data_ptr()
    for buf, o, w in zip(bufs, outs, want):
        assert torch.equal(o.cpu(), w)
        assert bool((buf[:pad] == -12345.0).all()) and bool((buf[pad + w.numel():] == -12345.0).all())


def test_a_captured_launch_follows_the_rewritten_table():
    lq, gt = pair((4, 3, 8, 8), 2, seed=5)
    dlq, dgt = lq.to(DEV), gt.to(DEV)
    plans = [mix_plan((0, 1), 0, 0, 2, seed=1), mix_plan((3, 2), 3, 1, 2, seed=2), mix_plan((1, 1), 2, 3, 2, seed=3)]
    table = torch.zeros((4, 5), dtype=torch.int32, device=DEV)
    a, b = torch.zeros(2, 3, 5, 5, device=DEV), torch.zeros(2, 3, 10, 10, device=DEV)
    table[:2].copy_(R.plan_table(plans[0], 4, 8, 5))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.batch_remix(dlq, dgt, table, 2, 5, 2, True, a, b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.batch_remix(dlq, dgt, table, 2, 5, 2, True, a, b)
    for plan in plans[1:]:
        table[:2].copy_(R.plan_table(plan, 4, 8, 5))
        graph.replay()
        want = R.batch_remix(lq, gt, plan, 2, patch=5)
        assert torch.equal(a.cpu(), want[0]) and torch.equal(b.cpu(), want[1])


def test_bad_arguments_return_their_codes_without_a_launch():
    lq, gt = (t.to(DEV) for t in pair((2, 3, 8, 8), 2))
    table = torch.zeros((2, 5), dtype=torch.int32, device=DEV)
    a, b = torch.full((2, 3, 8, 8), 7.0, device=DEV), torch.full((2, 3, 16, 16), 7.0, device=DEV)
    fn = L.lib().grl_batch_remix
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def code(**over):
        kw = dict(lq=lq.data_ptr(), lq_stride=(C.c_int64 * 4)(*lq.stride()), gt=gt.data_ptr(), gt_stride=(C.c_int64 * 4)(*gt.stride()),
                  B=2, P=8, Cl=3, Cg=3, b=2, p=8, s=2, mix=1, items=table.data_ptr(), lq_out=a.data_ptr(), gt_out=b.data_ptr())
        kw.update(over)
        return fn(stream, C.byref(L.GrlBatchRemixArgs(**kw)))

    assert fn(stream, None) == -1
    for name in ("lq", "gt", "items", "lq_out", "gt_out"):
        assert code(**{name: None}) == -1, name
    for name in ("B", "P", "Cl", "Cg", "b", "p", "s"):
        assert code(**{name: 0}) == -1 and code(**{name: -3}) == -1, name
    assert code(p=9) == -1                                          # p > P
    for name in ("lq", "gt", "items", "lq_out", "gt_out"):
        assert code(**{name: lq.data_ptr() + 2}) == -2, name     # not aligned to an element
    assert code(B=1 << 15, P=256, p=8, Cl=1) == -2                  # 2^31 source elements
    assert code(P=1 << 14, p=1 << 14, b=8, Cl=1, Cg=1, s=1) == -2   # 2^31 output elements
    assert code(P=1 << 14, p=8, s=4, B=1, Cg=1) == -2               # ... of the target's source, through the scale
    assert code(b=65536, p=1, P=8) == -2
    torch.cuda.synchronize()
    assert bool((a == 7.0).all()) and bool((b == 7.0).all())        # nothing ran
    assert code() == 0
    torch.cuda.synchronize()
    assert not bool((a == 7.0).any())


def test_train_across_a_stage_boundary_captured_and_eager(tmp_path, capsys):
    """A two-stage run on dual-pixel folders (6 channels in, 3 out): stage 0 is steps 0 .. 2 on 1 x 48 x 48, stage 1 is step 3 on
    2 x 96 x 96, MixUp comes on at step 1, inside stage 0.  The captured run builds a second captured step at the boundary; the
    eager run is the comparison, and a second eager run the yardstick for how far two runs of the same step drift apart (the
    bound of test_gpu_train_graph.py::test_graphed_train_step_matches_eager_steps)."""
    from PIL import Image

    from grl_image_restoration_amd import evaluate, train

    g = np.random.RandomState(4)
    for name in ("left", "right", "target"):
        (tmp_path / name).mkdir()
        for i, (h, w) in enumerate([(120, 112), (96, 100)]):
            smooth = np.kron(g.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)), np.ones((8, 8, 1)))[:h, :w].astype(np.uint8)
            Image.fromarray(smooth).save(tmp_path / name / f"im{i}.png")
    L_, R_, G = (str(tmp_path / n) for n in ("left", "right", "target"))
    model = ["--task", "sr", "--scale", "1", "--model", "tiny", "--geometry", "defocus"]
    args = model + ["--gt", G, "--lq", L_, "--lq-r", R_, "--patch", "96", "--batch", "2", "--steps", "4", "--lr", "2e-4",
                    "--stage-steps", "2+2", "--batch-sizes", "1+2", "--patch-sizes", "48+96", "--mixup", "--mixup-after", "1"]
    runs = []
    for extra in (["--out", str(tmp_path / "run")], ["--eager"], ["--eager"]):
        torch.manual_seed(0)
        runs.append(train.main(args + extra))
    captured, ea, eb = runs
    for r in runs:
        assert r["steps"] == [0, 1, 2, 3] and all(np.isfinite(r["losses"])) and r["stages"] == [(0, 1, 48), (3, 2, 96)]
        assert r["work"] == captured["work"]
    l_ee = max(abs(a - b) for a, b in zip(ea["losses"], eb["losses"]))
    print(f"losses captured {captured['losses']} | eager {ea['losses']} | eager {eb['losses']}; max |dloss| eager-eager {l_ee:.3e}")
    assert all(abs(a - b) <= max(2e-4 * abs(a), 4 * l_ee + 5e-5) for a, b in zip(ea["losses"], captured["losses"]))
    obj = torch.load(captured["checkpoint"], map_location="cpu", weights_only=False)
    assert {int(s["step"]) for s in obj["optimizer"]["state"].values()} == {4}          # the host's count: every step was one step
    assert obj["step"] == 4 and set(obj["remix_rng"]) == {"draws", "mixup"}
    v = evaluate.main(model + ["--lq", L_, "--lq-r", R_, "--gt", G, "--tile", "96", "--overlap", "16", "--ckpt", captured["checkpoint"],
                               "--metric", "restorer"])
    assert all(np.isfinite(x) for x in v.values())
    capsys.readouterr()
