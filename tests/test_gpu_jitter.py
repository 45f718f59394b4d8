"""``grl_color_jitter`` (csrc/jitter.hip) against the float64 evaluation of the statement in include/grl_hip.h
(``jitter.jitter_image`` on float64 CPU tensors), and ``PatchSampler(jitter=True)`` on the device.  torchvision is not installed:
no test here is a run of it.

The bar is 4 E, E = tests/test_jitter.py's ``E_FP32`` = 1.165e-6: the worst deviation of torch's fp32 CPU evaluation of the same
statement from float64 on these very items (the reference's own arithmetic, measured on the CPU, frozen).  The factor covers
multiply-add contraction and the different summation of the mean; it is the factor csrc/isp.hip is held to.  The map is
continuous, so nothing is left out: no tie exclusion, no outlier allowance.  The contrast means are held to E.
"""
import ctypes as C

import pytest
import torch

from grl_image_restoration_amd import PatchSampler, PatchStore, _lib, bsr_degrade as B, jitter as J
from tests.test_degrade import U24, resize_bound
from tests.test_jitter import E_FP32, ORDERS, image8, kernel_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 4 * E_FP32
FILL = -7.0


@pytest.fixture(scope="module")
def cases():
    """The items, their place in the arenas and the float64 yardstick, computed once.  Items follow each other without padding (so
    the 19 x 23 ones start at odd offsets), except that the 64 x 64 one is moved to a multiple of 4: it takes the float4 path."""
    cs, at = kernel_cases(), 0
    for c in cs:
        h, w = c["x"].shape[1:]
        if (h, w) == (64, 64):
            at = (at + 3) // 4 * 4
        c["off"], c["h"], c["w"] = at, h, w
        c["want"], mean = J.jitter_image(c["x"].double(), c["params"], with_mean=True)
        c["want_mean"] = float(mean)
        at += 3 * h * w
    return cs, at


def _launch(cs, total, pick=None, in_place=False):
    """One call over the items ``pick`` (all of them) at their places.  Returns ({item: result}, {item: mean}, the destination)."""
    pick = list(range(len(cs))) if pick is None else pick
    src = torch.zeros(total, device=DEV)
    for c in cs:
        src[c["off"] : c["off"] + c["x"].numel()] = c["x"].to(DEV).reshape(-1)
    dst = src if in_place else torch.full((total,), FILL, device=DEV)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    rows, factors = J.item_rows([(cs[i]["off"], cs[i]["off"], cs[i]["h"], cs[i]["w"]) for i in pick], [cs[i]["params"] for i in pick])
    max_h, max_w = max(cs[i]["h"] for i in pick), max(cs[i]["w"] for i in pick)
    nwg = J.num_workgroups(max_h, max_w)
    partial = torch.full((len(pick) * nwg,), float("nan"), dtype=torch.float64, device=DEV)
    means = torch.full((len(pick),), float("nan"), dtype=torch.float64, device=DEV)
    J.hip_color_jitter(src, dst, rows.to(DEV), factors.to(DEV), partial, means, max_h, max_w)
    torch.cuda.synchronize()
    out = dst.cpu()
    res = {i: out[cs[i]["off"] : cs[i]["off"] + 3 * cs[i]["h"] * cs[i]["w"]].view(3, cs[i]["h"], cs[i]["w"]) for i in pick}
    if not in_place:
        touched = torch.zeros(total, dtype=torch.bool)
        for i in pick:
            touched[cs[i]["off"] : cs[i]["off"] + 3 * cs[i]["h"] * cs[i]["w"]] = True
        assert bool((out[~touched] == FILL).all()), "nothing outside the items' destinations is written"
    return res, dict(zip(pick, means.cpu().tolist())), out


@pytest.fixture(scope="module")
def full(cases):
    return _launch(*cases)


def test_all_orders_in_one_launch_against_float64(cases, full):
    cs, _ = cases
    assert [c["params"][0] for c in cs[:24]] == ORDERS
    shapes = [(c["h"], c["w"]) for c in cs]
    assert shapes[:24] == [(19, 23)] * 24 and {(1, 1), (1, 70), (64, 64), (33, 130)} <= set(shapes[24:])
    vec = cs[shapes.index((64, 64))]
    assert vec["off"] % 4 == 0 and cs[3]["off"] % 4, "the float4 path and the scalar path both run"
    assert J.num_workgroups(33, 130) > 1 and J.num_workgroups(19, 23) == 1 and J.num_workgroups(400, 400) == 40
    res, means, _ = full
    worst = worst_mean = 0.0
    for i, c in enumerate(cs):
        got = res[i].double()
        assert bool(torch.isfinite(got).all()) and 0 <= float(got.min()) and float(got.max()) <= 1
        err, merr = float((got - c["want"]).abs().max()), abs(means[i] - c["want_mean"])
        print(f"item {i} {c['h']} x {c['w']} order {c['params'][0]}: max|hip - float64| = {err:.3e} ({err / BAR:.2f} of the bar), "
              f"mean off by {merr:.3e}")
        worst, worst_mean = max(worst, err), max(worst_mean, merr)
    print(f"worst {worst:.3e}, bar {BAR:.3e}; worst mean {worst_mean:.3e}, bar {E_FP32:.3e}")
    assert worst <= BAR and worst_mean <= E_FP32


def test_two_calls_give_the_same_bits(cases, full):
    res, means, out = full
    res2, means2, out2 = _launch(*cases)
    assert torch.equal(out, out2) and means == means2


def test_an_items_result_does_not_depend_on_the_list(cases, full):
    cs, total = cases
    multi = next(i for i, c in enumerate(cs) if (c["h"], c["w"]) == (33, 130))
    for i in (0, 5, multi):
        res, means, _ = _launch(cs, total, pick=[i])
        assert torch.equal(res[i], full[0][i]) and means[i] == full[1][i], i


def test_in_place(cases, full):
    res, means, _ = _launch(*cases, in_place=True)
    for i in full[0]:
        assert torch.equal(res[i], full[0][i]), i
    assert means == full[1]


def _args(**kw):
    h = w = 8
    src = torch.rand(3 * h * w, device=DEV)
    dst = torch.full((3 * h * w,), FILL, device=DEV)
    rows, factors = J.item_rows([(0, 0, h, w)], [((0, 1, 2, 3), 0.9, 1.1, 0.9, 0.02)])
    rows, factors = rows.to(DEV), factors.to(DEV)
    partial, means = torch.zeros(4, dtype=torch.float64, device=DEV), torch.full((1,), FILL, dtype=torch.float64, device=DEV)
    good = dict(src=src.data_ptr(), dst=dst.data_ptr(), src_elems=src.numel(), dst_elems=dst.numel(), items=rows.data_ptr(),
                params=factors.data_ptr(), partial=partial.data_ptr(), n_partial=partial.numel(), means=means.data_ptr(), n_items=1,
                C=3, max_h=h, max_w=w)
    return dict(good, **kw), dst, means, (src, rows, factors, partial)


def test_bad_arguments_launch_nothing():
    fn = _lib.lib().grl_color_jitter
    good, dst, means, keep = _args()
    for bad in (dict(src=None), dict(dst=None), dict(items=None), dict(params=None), dict(partial=None), dict(means=None), dict(C=1),
                dict(C=4), dict(n_items=0), dict(n_items=65536), dict(src_elems=0), dict(dst_elems=0), dict(max_h=0), dict(max_w=0),
                dict(max_h=(1 << 20) + 1), dict(n_partial=0), dict(src=good["src"] + 2), dict(dst=good["dst"] + 1),
                dict(params=good["params"] + 2), dict(items=good["items"] + 4), dict(partial=good["partial"] + 4), dict(means=good["means"] + 4)):
        assert fn(_lib.stream_ptr(), C.byref(_lib.GrlColorJitterArgs(**dict(good, **bad)))) == -1, bad
    assert fn(_lib.stream_ptr(), None) == -1
    assert _lib.lib().grl_color_jitter_num_workgroups(0, 8) == -1 and _lib.lib().grl_color_jitter_num_workgroups(8, (1 << 20) + 1) == -1
    torch.cuda.synchronize()
    assert bool((dst == FILL).all()) and float(means[0]) == FILL
    assert fn(_lib.stream_ptr(), C.byref(_lib.GrlColorJitterArgs(**good))) == 0          # and the good one runs
    torch.cuda.synchronize()
    assert not bool((dst == FILL).any()) and float(means[0]) != FILL


def test_an_item_outside_the_arena_is_skipped_and_its_neighbours_stay():
    """Three 8 x 8 items; the middle one reaches past the destination or the source, starts before them, has h = 0, a side beyond
    2^20, more pixels than the host vouched for, or an order that is no permutation: it is skipped whole -- its destination and its
    mean keep the fill -- and the two others come out as they do alone."""
    h = w = 8
    n = 3 * h * w
    params = [((3, 1, 0, 2), 0.85, 1.15, 0.9, -0.03), ((1, 0, 2, 3), 1.1, 0.9, 1.2, 0.04), ((2, 3, 1, 0), 0.95, 0.8, 1.05, 0.05)]
    src = torch.cat([image8(80 + i, h, w).reshape(-1) for i in range(3)]).to(DEV)
    good, factors = J.item_rows([(i * n, i * n, h, w) for i in range(3)], params)
    factors = factors.to(DEV)

    def run(rows):
        dst = torch.full((3 * n,), FILL, device=DEV)
        partial = torch.zeros(3, dtype=torch.float64, device=DEV)
        means = torch.full((3,), FILL, dtype=torch.float64, device=DEV)
        J.hip_color_jitter(src, dst, rows.to(DEV), factors, partial, means, h, w)
        torch.cuda.synchronize()
        return dst.cpu(), means.cpu()

    ref, ref_means = run(good)
    assert not bool((ref == FILL).any()) and not bool((ref_means == FILL).any())
    for col, val in ((1, 2 * n + 1), (1, 3 * n), (0, 2 * n + 1), (1, -1), (0, -1), (2, 0), (3, 0), (2, (1 << 20) + 1), (7, 1), (4, 4), (5, -1)):
        rows = good.clone()
        rows[1, col] = val
        got, means = run(rows)
        assert bool((got[n : 2 * n] == FILL).all()) and float(means[1]) == FILL, (col, val)
        assert torch.equal(got[:n], ref[:n]) and torch.equal(got[2 * n :], ref[2 * n :]), (col, val)
        assert means[0] == ref_means[0] and means[2] == ref_means[2], (col, val)
    # an item of two workgroups that fits the arenas, in a call whose host vouched for one workgroup per item
    big = image8(90, 65, 65).reshape(-1).to(DEV)
    dst = torch.full_like(big, FILL)
    rows, f = J.item_rows([(0, 0, 65, 65)], params[:1])
    partial, means = torch.zeros(4, dtype=torch.float64, device=DEV), torch.full((1,), FILL, dtype=torch.float64, device=DEV)
    assert J.num_workgroups(65, 65) == 2 and J.num_workgroups(8, 8) == 1
    J.hip_color_jitter(big, dst, rows.to(DEV), f.to(DEV), partial, means, 8, 8)
    torch.cuda.synchronize()
    assert bool((dst == FILL).all()) and float(means[0]) == FILL and not bool(partial.any())


def test_color_jitter_lists_on_the_device(cases, full):
    cs, _ = cases
    pick = [0, 7, 24, 26, 27]
    out, means = J.color_jitter([cs[i]["x"].to(DEV) for i in pick], [cs[i]["params"] for i in pick], with_means=True)
    for i, got, m in zip(pick, out, means.tolist()):
        assert got.is_cuda and got.shape == cs[i]["want"].shape
        assert float((got.cpu().double() - cs[i]["want"]).abs().max()) <= BAR and abs(m - cs[i]["want_mean"]) <= E_FP32
    with pytest.raises(TypeError, match="fp32"):
        J.color_jitter([cs[0]["x"].to(DEV).double()], [cs[0]["params"]])


def _pipeline_bound(plan, crop, e):
    """tests/test_gpu_degrade.py's bound of one plan of blur / resize / clip / imresize ops, started from an input error ``e``."""
    size = crop
    for op in plan:
        if op["op"] == "resize":
            e = 2 * e + resize_bound(op["interp"], size, size, op["size"], op["size"]) + U24
        elif op["op"] == "blur":
            e = e + (op["kernel"].shape[0] ** 2 + 2) * U24 + U24
        elif op["op"] == "imresize_half":
            e = 1.6 * e + 2 * U24 + U24
        elif op["op"] not in ("clip", "jpeg_final"):
            raise AssertionError(op["op"])
        size = op["size"]
    return e


def test_one_sampler_batch_on_the_device():
    """The same sampler on a CUDA and on a CPU store, plans of the blur and resize stages (no noise is drawn).  The GT patches are
    cuts of the jittered crops: within the kernel bar.  The LQ before its final JPEG: within test_gpu_degrade's pipeline bound
    started from that bar (the JPEG round trip quantises; the device LQ is its own pre-JPEG image through it, bit for bit)."""
    import random

    import numpy as np

    from grl_image_restoration_amd import tasks as T

    g = np.random.RandomState(1)
    imgs = [g.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((70, 80), (64, 96), (90, 64))]
    make = lambda dev: PatchSampler("sr", PatchStore(imgs, dev), degrade=True, degrade_crop=64, patch=8, scale=4, batch=4, seed=5, jitter=True)
    s, cpu = make(DEV), make("cpu")
    work, extras = s.draw()
    cwork, cextras = cpu.draw()
    assert work == cwork and [e[3] for e in extras] == [e[3] for e in cextras], "CPU and CUDA samplers make identical draws"
    rng = random.Random(4)
    plans = [B.draw_plan(rng, 4, 64, stages=(0, 1, 5, 6)) for _ in range(4)]
    extras = [(p, b % 9, (2 * b) % 9, e[3]) for b, (p, e) in enumerate(zip(plans, extras))]
    lq, gt = s.next(work, extras)
    _, cgt = cpu.next(work, extras)
    assert lq.shape == (4, 3, 8, 8) and gt.shape == (4, 3, 32, 32) and lq.is_cuda and gt.is_cuda
    err = float((gt.cpu() - cgt).abs().max())
    print(f"GT patches: max|hip - cpu| = {err:.3e}, bar {BAR:.3e}")
    assert err <= BAR and not torch.equal(gt.cpu(), PatchSampler("sr", PatchStore(imgs, "cpu"), degrade=True, degrade_crop=64, patch=8, scale=4,
                                                                 batch=4, seed=5).next(work, [e[:3] for e in extras])[1])
    wt = torch.tensor(work, dtype=torch.int32)
    params = [e[3] for e in extras]
    crops = s.jitter_lists.run_(s.gt_store.sample(wt.to(DEV), 64, 1), params)
    ccrops = torch.stack(J.color_jitter(list(cpu.gt_store.sample(wt, 64, 1)), params))
    assert float((crops.cpu() - ccrops).abs().max()) <= BAR
    out, pre, q = B.apply_plans(crops, plans, parts=True)
    _, cpre, cq = B.apply_plans(ccrops, plans, parts=True)
    assert torch.equal(q.cpu(), cq) and torch.equal(out, T.jpeg_roundtrip(pre, q))
    for b, (_, r, c, _) in enumerate(extras):
        assert torch.equal(gt[b], crops[b, :, 4 * r : 4 * r + 32, 4 * c : 4 * c + 32]) and torch.equal(lq[b], out[b, :, r : r + 8, c : c + 8])
        e, bound = float((pre[b].cpu().double() - cpre[b].double()).abs().max()), _pipeline_bound(plans[b], 64, BAR)
        print(f"sample {b}: pre-JPEG LQ max|hip - cpu| = {e:.3e}, bound {bound:.3e}")
        assert e <= bound
