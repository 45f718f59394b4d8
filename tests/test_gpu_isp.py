"""The three ISP kernels (csrc/isp.hip: grl_isp_unprocess, grl_isp_process, grl_isp_roundtrip) against the float64 restatement of
``isp`` on the CPU, and the camera stage through ``apply_plans`` and ``PatchSampler`` on the device.  The tables are analytic
(y = t^0.8 and its inverse; one inverse table with a jump of 1e-2 put in by hand), so no scipy is needed.

The bar: four times the distance between the float64 restatement and the reference's own fp32 outputs
(tests/test_isp.py: REFERENCE_TO_RESTATEMENT = 1.002e-5, so 4.008e-5).  The margin covers another ``powf``, contracted
multiply-adds, and a table index one off where the table's steps are 1e-5 or smaller.  On the smooth tables no value may exceed
it.  On the jump table an index one off at the jump moves a value by the jump: at most 1 value in 10,000 may exceed the bar and none
by more than the jump.  (On the CPU, the restatement in fp32 against itself in float64 exceeds the bar at no value of these inputs.)
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import PatchSampler, PatchStore, _lib, bsr_degrade as B, isp
from tests.test_isp import REFERENCE_TO_RESTATEMENT, _plans_with_camera, analytic_bank, draws, image8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 4 * REFERENCE_TO_RESTATEMENT
JUMP = 1e-2
# odd sides, the smallest legal side, tiles of 64 x 4 and 32 x 32 crossed in both axes
SIZES = [(3, 3), (7, 9), (16, 16), (33, 20), (65, 35), (64, 64)]


@pytest.fixture(scope="module")
def banks():
    return build_banks()


def build_banks():
    return {"smooth": analytic_bank(), "jump": analytic_bank(jump_curve=4)}


def _cases(bank, kind):
    """Per size: the 8-bit image, its params, its normals, and the float64 restatement of every entry -- the process entry on the
    fp32 rounding of the restated raw plane, so that each entry is held against the restatement on its own input."""
    out = []
    for n, (h, w) in enumerate(SIZES):
        x = image8(40 + n, h, w)
        p = bank.params(draws(60 + n, curve=4 if kind == "jump" else None))
        z = torch.randn(h, w, generator=torch.Generator().manual_seed(n))
        raw = isp.add_raw_noise(isp.mosaic(isp.unprocess(x.double(), p)), p, z).float()
        out.append(dict(x=x, p=p, z=z, raw=raw, want_raw=raw.double(), want_rgb=isp.process(isp.demosaic(raw.double()), p),
                        want_rt=isp.process(isp.unprocess(x.double(), p), p)))
    return out


@pytest.fixture(scope="module")
def cases(banks):
    return build_cases(banks)


def build_cases(banks):
    return {kind: _cases(bank, kind) for kind, bank in banks.items()}


def _launch_all(cs, only=None):
    """One launch of each entry over the list (or over item ``only`` alone) with source and destination arenas in ONE buffer:
    [images | raw planes | results].  Returns per entry the list of results."""
    pick = list(range(len(cs))) if only is None else [only]
    n_img = sum(c["x"].numel() for c in cs)
    n_raw = sum(c["raw"].numel() for c in cs)
    res = {}
    for entry, src_key, planes in (("grl_isp_unprocess", "x", 1), ("grl_isp_process", "raw", 3), ("grl_isp_roundtrip", "x", 3)):
        buf = torch.full((n_img + n_raw + n_img,), -7.0, device=DEV)
        items, so, do, zo = {}, 0, n_img + n_raw, 0
        for i, c in enumerate(cs):
            h, w = c["z"].shape
            src = c[src_key].to(DEV).reshape(-1)
            buf[so : so + src.numel()] = src
            items[i] = (so, do, h, w, zo)
            so, do, zo = so + src.numel(), do + planes * h * w, zo + h * w
        normals = torch.cat([c["z"].reshape(-1) for c in cs]).to(DEV) if entry == "grl_isp_unprocess" else None
        isp.hip_isp(entry, buf, buf, [items[i] for i in pick], [cs[i]["p"] for i in pick], normals)
        torch.cuda.synchronize()
        res[entry] = {i: buf[items[i][1] : items[i][1] + planes * items[i][2] * items[i][3]].cpu().view(-1, items[i][2], items[i][3])
                      for i in pick}
        touched = torch.zeros_like(buf, dtype=torch.bool)
        for i in pick:
            touched[items[i][1] : items[i][1] + planes * items[i][2] * items[i][3]] = True
        tail = buf[n_img + n_raw :]
        assert bool((tail[~touched[n_img + n_raw :]] == -7.0).all()), "nothing outside the items' destinations is written"
    return res


@pytest.mark.parametrize("kind", ["smooth", "jump"])
def test_kernels_against_the_float64_restatement(cases, kind):
    cs = cases[kind]
    res = _launch_all(cs)
    over = total = 0
    worst = 0.0
    for entry, key in (("grl_isp_unprocess", "want_raw"), ("grl_isp_process", "want_rgb"), ("grl_isp_roundtrip", "want_rt")):
        for i, c in enumerate(cs):
            got, want = res[entry][i].double(), c[key].reshape(res[entry][i].shape)
            assert bool(torch.isfinite(got).all()) and 0 <= float(got.min()) and float(got.max()) <= 1
            if entry == "grl_isp_unprocess":
                # the restatement's raw plane was rounded to fp32 for the next entry; compare with the unrounded float64 one
                want = isp.add_raw_noise(isp.mosaic(isp.unprocess(c["x"].double(), c["p"])), c["p"], c["z"])[None]
            err = (got - want).abs()
            print(f"{kind} {entry} {tuple(got.shape)}: max|hip - float64| = {float(err.max()):.3e} ({float(err.max()) / BAR:.2f} of the bar)")
            worst = max(worst, float(err.max()))
            over += int((err > BAR).sum())
            total += err.numel()
    print(f"{kind}: worst {worst:.3e}, bar {BAR:.3e}, {over} of {total} values above it")
    if kind == "smooth":
        assert over == 0
    else:
        assert over <= total / 10000 and worst <= BAR + JUMP


def test_an_items_result_does_not_depend_on_the_list(cases):
    cs = cases["smooth"]
    together = _launch_all(cs)
    for i in (0, 3, 4):
        alone = _launch_all(cs, only=i)
        for entry in together:
            assert torch.equal(alone[entry][i], together[entry][i]), (entry, SIZES[i])


def _args(bank, **kw):
    h, w = 8, 8
    src = torch.rand(3 * h * w, device=DEV)
    dst = torch.full((3 * h * w,), -7.0, device=DEV)
    items = torch.tensor([[0, 0, h, w, 0, isp.TABLE_N, 0, 0]], dtype=torch.int64, device=DEV)
    rec = bank.params(draws(1)).rec.to(DEV)
    z = torch.zeros(h * w, device=DEV)
    tables = bank.tables(DEV)
    good = dict(src=src.data_ptr(), dst=dst.data_ptr(), src_elems=src.numel(), dst_elems=dst.numel(), items=items.data_ptr(),
                params=rec.data_ptr(), tables=tables.data_ptr(), tables_elems=tables.numel(), normals=z.data_ptr(),
                normals_elems=z.numel(), n_items=1, C=3, max_h=h, max_w=w)
    return dict(good, **kw), dst, (src, items, rec, z, tables)


def test_bad_arguments_launch_nothing(banks):
    L = _lib.lib()
    entries = (L.grl_isp_unprocess, L.grl_isp_process, L.grl_isp_roundtrip)
    for bad in (dict(src=None), dict(dst=None), dict(items=None), dict(params=None), dict(tables=None), dict(C=1), dict(max_h=2),
                dict(max_w=2), dict(n_items=0), dict(tables_elems=isp.TABLE_N - 1), dict(src_elems=0)):
        fields, dst, keep = _args(banks["smooth"], **bad)
        for fn in entries:
            assert fn(_lib.stream_ptr(), C.byref(_lib.GrlIspArgs(**fields))) == -1, bad
        torch.cuda.synchronize()
        assert bool((dst == -7.0).all()), bad
    fields, dst, keep = _args(banks["smooth"], normals=None)
    assert L.grl_isp_unprocess(_lib.stream_ptr(), C.byref(_lib.GrlIspArgs(**fields))) == -1
    assert all(fn(_lib.stream_ptr(), None) == -1 for fn in entries)


def test_an_item_outside_the_arena_is_skipped_and_its_neighbours_stay(banks):
    """Three 8 x 8 items; the middle one reaches past the destination (or the source, the tables, the normals) or has a side of 2:
    it is skipped whole, and the two others come out as they do alone."""
    bank, L = banks["smooth"], _lib.lib()
    h = w = 8
    n = 3 * h * w
    ps = [bank.params(draws(70 + i)) for i in range(3)]
    rec = torch.stack([p.rec for p in ps]).to(DEV)
    tables = bank.tables(DEV)
    src = torch.cat([image8(80 + i, h, w).reshape(-1) for i in range(3)]).to(DEV)
    z = torch.randn(3 * h * w, generator=torch.Generator().manual_seed(5)).to(DEV)
    T = isp.TABLE_N
    good = [[i * n, i * n, h, w, 2 * ps[i].curve * T, (2 * ps[i].curve + 1) * T, i * h * w, 0] for i in range(3)]

    def run(fn, rows):
        dst = torch.full((3 * n,), -7.0, device=DEV)
        items = torch.tensor(rows, dtype=torch.int64, device=DEV)
        args = _lib.GrlIspArgs(src=src.data_ptr(), dst=dst.data_ptr(), src_elems=src.numel(), dst_elems=dst.numel(), items=items.data_ptr(),
                               params=rec.data_ptr(), tables=tables.data_ptr(), tables_elems=tables.numel(), normals=z.data_ptr(),
                               normals_elems=z.numel(), n_items=3, C=3, max_h=h, max_w=w)
        assert fn(_lib.stream_ptr(), C.byref(args)) == 0
        torch.cuda.synchronize()
        return dst.cpu()

    for fn, planes in ((L.grl_isp_unprocess, 1), (L.grl_isp_process, 3), (L.grl_isp_roundtrip, 3)):
        ref = run(fn, good)
        assert not bool((ref[n : n + planes * h * w] == -7.0).any())
        for col, val in ((1, 3 * n - planes * h * w + 1), (0, 3 * n), (1, -1), (2, 2), (3, 2), (4, 22 * T), (5, 21 * T + 1), (4, -1)) + \
                        (((6, 3 * h * w - h * w + 1),) if planes == 1 else ()):
            rows = [list(r) for r in good]
            rows[1][col] = val
            got = run(fn, rows)
            assert bool((got[n : 2 * n] == -7.0).all()), (planes, col, val)
            assert torch.equal(got[:n], ref[:n]) and torch.equal(got[2 * n :], ref[2 * n :]), (planes, col, val)


def test_roundtrip_in_place(cases):
    cs = cases["smooth"]
    out = _launch_all(cs)["grl_isp_roundtrip"]
    buf = torch.cat([c["x"].reshape(-1) for c in cs]).to(DEV)
    items, so = [], 0
    for c in cs:
        h, w = c["z"].shape
        items.append((so, so, h, w, 0))
        so += 3 * h * w
    isp.hip_isp("grl_isp_roundtrip", buf, buf, items, [c["p"] for c in cs])
    for i, it in enumerate(items):
        assert torch.equal(buf[it[0] : it[0] + 3 * it[2] * it[3]].cpu().view(3, it[2], it[3]), out[i])


def test_camera_noise_lists_on_the_device(cases):
    cs = cases["smooth"]
    lq, hr = isp.camera_noise([c["x"].to(DEV) for c in cs], [c["x"].to(DEV) for c in cs], [c["p"] for c in cs], [c["z"].to(DEV) for c in cs])
    want_lq, want_hr = isp.camera_noise([c["x"].double() for c in cs], [c["x"].double() for c in cs], [c["p"] for c in cs],
                                        [c["z"] for c in cs])
    for got, want in zip(lq + hr, want_lq + want_hr):
        assert got.is_cuda and got.shape == want.shape and float((got.cpu().double() - want).abs().max()) <= BAR
    with pytest.raises(ValueError, match="at least 3"):
        isp.camera_noise([torch.rand(3, 2, 8, device=DEV)], None, [cs[0]["p"]], [torch.zeros(2, 8, device=DEV)])


def test_apply_plans_on_the_device_against_the_cpu(banks, monkeypatch):
    """stages=(2,) at scale 2: the camera stage alone through the arenas, with the normals the device generator drew handed to the
    CPU path, up to the final JPEG."""
    bank = banks["smooth"]
    x = torch.stack([image8(20 + s, 32, 32) for s in range(4)])
    plans = _plans_with_camera(bank, 4, 2, 32, (2,), 3)
    out, pre, q, hr = B.apply_plans(x.to(DEV), plans, torch.Generator(device=DEV).manual_seed(6), parts=True, hr=x.to(DEV).clone())
    gen = torch.Generator(device=DEV).manual_seed(6)
    drawn = [torch.randn(32, 32, generator=gen, device=DEV).cpu() for _ in range(3)]
    monkeypatch.setattr(B, "_camera_normals", lambda g, side, device: drawn.pop(0))
    _, want_pre, want_q, want_hr = B.apply_plans(x, plans, None, parts=True, hr=x.clone())
    assert not drawn and torch.equal(q.cpu(), want_q)
    acts = [any(op["op"] == "camera" for op in p) for p in plans]
    for b, act in enumerate(acts):
        e_lq, e_hr = float((pre[b].cpu() - want_pre[b]).abs().max()), float((hr[b].cpu() - want_hr[b]).abs().max())
        print(f"sample {b} acting {act}: max|hip - cpu| LQ {e_lq:.3e}, HR {e_hr:.3e}, bar {BAR:.3e}")
        assert e_lq <= BAR and e_hr <= BAR
        if act:
            assert not torch.equal(pre[b].cpu(), x[b]) and not torch.equal(hr[b].cpu(), x[b])
        else:
            assert torch.equal(pre[b].cpu(), x[b]) and torch.equal(hr[b].cpu(), x[b])
    from grl_image_restoration_amd import tasks as T

    assert torch.equal(out, T.jpeg_roundtrip(pre, q))


def test_one_sampler_batch_with_a_camera(banks):
    """Plans without the noise stages, so that the generator serves the camera stage alone: the samples where the op did not act
    are then bit for bit those of the same plans without it."""
    bank = banks["smooth"]
    g = np.random.RandomState(1)
    store = PatchStore([g.randint(0, 256, (70, 80, 3)).astype(np.uint8), g.randint(0, 256, (64, 96, 3)).astype(np.uint8)], DEV)
    s = PatchSampler("sr", store, degrade=True, degrade_crop=64, patch=8, scale=4, batch=8, seed=2, usm=True, camera=bank)
    work, _ = s.draw()
    for seed in range(200):
        rng = random.Random(seed)
        plans = [B.draw_plan(rng, 4, 64, stages=(0, 1, 2, 4, 5, 6), camera=bank) for _ in range(8)]
        acts = [any(op["op"] == "camera" for op in p) for p in plans]
        if 2 <= sum(acts) <= 6:
            break
    extras = [(p, b % 9, (2 * b) % 9) for b, p in enumerate(plans)]
    bare = [([op for op in p if op["op"] != "camera"], r, c) for p, r, c in extras]
    lq, gt = s.next(work, extras)
    lq0, gt0 = s.next(work, bare)
    assert lq.shape == (8, 3, 8, 8) and gt.shape == (8, 3, 32, 32) and lq.is_cuda and gt.is_cuda
    for t in (lq, gt):
        assert bool(torch.isfinite(t).all()) and 0 <= float(t.min()) and float(t.max()) <= 1
    assert torch.equal((lq.cpu() * 255).round().div(255), lq.cpu()), "the k / 255 grid"
    for b, act in enumerate(acts):
        assert torch.equal(gt[b], gt0[b]) != act and torch.equal(lq[b], lq0[b]) != act, (b, act)
