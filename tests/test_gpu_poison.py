"""The poison pass: every kernel family with NaN-poisoned outputs and workspaces (ops.set_poison), guard bands around them
(guards=True, checked after every test by ops.check_guards) and the LDS of every CU filled with NaN bytes before every launch
(_lib.set_dirty_lds).  A kernel that reads memory nobody wrote, or writes past the end of a tensor, passes the ordinary parity tests:
torch.empty hands out zeros in a fresh process, LDS still holds the previous workgroup's finite numbers, a write a few elements past
the end lands in the allocator's rounding slack.

(a) The core kernels: the existing test functions are called under ``dirty``, so reference and bar stay theirs.
(b) The task, data, metric and loss kernels: the package wrapper is called once clean and once under ``dirty`` on the same inputs; the
    second result is finite where the first is, bit-identical to it (a byte workspace poisoned with 0x7F reads back as a large
    FINITE float, so "finite" alone would pass), and within the op's own bar of the reference its own GPU module uses.  Where a
    kernel accumulates with fp32 atomics the module's bar stands in for bit identity.
"""
import contextlib

import numpy as np
import pytest
import torch

import tests.test_gpu_attention_skip as SKIP
import tests.test_gpu_attention_trips as TRIPS
import tests.test_gpu_blur as GB
import tests.test_gpu_degrade as GD
import tests.test_gpu_disc as DISC
import tests.test_gpu_dual_pixel as DP
import tests.test_gpu_ensemble as ENS
import tests.test_gpu_image8 as I8
import tests.test_gpu_isp as ISP
import tests.test_gpu_jitter as JIT
import tests.test_gpu_kernels as K
import tests.test_gpu_lpips as LPIPS
import tests.test_gpu_metrics as MET
import tests.test_gpu_model as MODEL
import tests.test_gpu_niqe as NIQE
import tests.test_gpu_optim_clip_ema as CLIP
import tests.test_gpu_patches as PAT
import tests.test_gpu_perceptual as PERC
import tests.test_gpu_remix as RMX
import tests.test_gpu_resize as RSZ
import tests.test_gpu_style as STYLE
import tests.test_gpu_tail_prefetch as TAIL
import tests.test_gpu_tasks as TASKS
import tests.test_gpu_train as TR
import tests.test_gpu_train_graph as TG
import tests.test_gpu_train_step as TS
import tests.test_gpu_usm as USM
from grl_image_restoration_amd import PatchSampler, PatchStore, _lib, bsr_degrade as BD, ensemble as E, image8 as I, jitter as J
from grl_image_restoration_amd import metrics as M, ops, remix as R, tasks as T
from tests.test_jpeg import levels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@contextlib.contextmanager
def _switches(poison, lds):
    prev_guards = ops._GUARDS
    prev_poison = ops.set_poison(poison, guards=poison)
    prev_lds = _lib.set_dirty_lds(lds)
    try:
        yield
    finally:
        _lib.set_dirty_lds(prev_lds)
        ops.set_poison(prev_poison, guards=prev_guards)


@pytest.fixture
def dirty():
    """Poisoned and guarded allocations, dirty LDS; afterwards both switches as they were and every guard band verified."""
    try:
        with _switches(True, True):
            yield
    finally:
        ops.check_guards()


@pytest.fixture
def poison_only():
    """``dirty`` without the LDS fill: for graph captures (the extra launch and its hipFuncSetAttribute stay out of the capture)."""
    try:
        with _switches(True, False):
            yield
    finally:
        ops.check_guards()


def test_the_switches_are_on_under_the_fixture_and_off_after_it(dirty):
    assert ops._POISON and ops._GUARDS and _lib._DIRTY_LDS
    t = ops.empty(3, 5, dtype=torch.float32, device=DEV)
    b = ops.empty(7, dtype=torch.uint8, device=DEV)
    assert t.storage_offset() > 0 and t.data_ptr() % 256 == 0 and bool(torch.isnan(t).all()) and bool((b == 0x7F).all())
    with _switches(False, False):
        assert not ops._POISON and not ops._GUARDS and not _lib._DIRTY_LDS
        assert ops.empty(3, dtype=torch.float32, device=DEV).storage_offset() == 0
    assert ops._POISON and ops._GUARDS and _lib._DIRTY_LDS


def test_check_guards_reports_a_device_write_past_the_end():
    """The guard check itself on the device (the write goes through the registry's base tensor: inside the allocation)."""
    with _switches(True, False):
        t = ops.empty(5, 3, dtype=torch.float16, device=DEV)
        base = ops._GUARDED[-1][0]
        base[ops.GUARD_BYTES + t.numel() * 2] = 0
    with pytest.raises(AssertionError, match=r"\(5, 3\) torch.float16.*above the tensor"):
        ops.check_guards()
    assert ops._GUARDED == []


# ---- (a) core kernels: the existing tests, under poison ------------------------------------------------------------------------------
_KC = {c[0]: c for c in K.CASES}
_TC = {c[0]: c for c in TR.ATT_CASES}


def _p(fn, *cases, ids=None):
    return [pytest.param(fn, c, id=f"{fn.__name__}-{ids[i] if ids else '-'.join(map(str, c))}") for i, c in enumerate(cases)]


INFERENCE = (
    _p(K.test_linear_groupnorm_and_plain, (300, 128, 64), (256, 192, 96))
    + _p(K.test_linear_ln_residual_and_gelu, (300, 384, 192, 180), (300, 128, 64, 64))
    + _p(K.test_fused_mlp, (50, 60, 120), (300, 64, 128))
    + _p(K.test_streaming_qkv, (333, 60, 3))
    + _p(K.test_fused_block_tail, (1000, 180, 360, 500))
    + _p(K.test_block_tail_register_resident, (128, 128), (2048, 1024))
    + _p(K.test_qkv_anchor_one_pass, (1, 8, 64, 64, 12, 2))
    + _p(K.test_qkv_anchor_split_precision, (2, 4, 64))
    + [pytest.param(K.test_attention_vs_oracle_indexing, (_KC[n], off, planes), id=f"attention-{n}-{off}-{'planes' if planes else 'slots'}")
       for n in ("win8_shift", "win12_ragged", "a2w_64_df4_tiny", "w2a_8x16_df4") for off in ("lazy", "online") for planes in (False, True)]
    + _p(K.test_attention_fp32_output_and_lse, (_KC["win12_ragged"],), ids=["win12_ragged"])
    + _p(K.test_attention_split_precision_operands, (_KC["win12_ragged"],), ids=["win12_ragged"])
    + _p(K.test_conv3x3, (1, 17, 33, 3, 180, 0, False), (1, 16, 16, 64, 3, 0, True), (2, 24, 40, 45, 180, 0, True))
    + _p(K.test_conv3x3_stage_shape_192, (1, 17, 70, True), (3, 8, 32, True))
    + _p(K.test_conv3x3_pixel_shuffle, (2, 3, 64))
    + _p(K.test_cab_conv2_register_resident_filters, ((5, 9, 33),), ((1, 20, 50),))
    + _p(K.test_linear_split_precision, (257, 384, 192, "plain"))
    + _p(K.test_linear_split_layernorm_epilogue, (512, 256, 128, 128, "f16"))
    + _p(K.test_conv3x3_split_precision, (1, 17, 33, 3, 64, 0))
    + _p(K.test_se_gate, ()) + _p(K.test_layernorm, ()) + _p(K.test_layernorm_res, ())
    + _p(TAIL.test_one_launch_equals_prefetch_free_launches, (32, 128), (32 * 257, 128))
    + _p(SKIP.test_against_float64, ("win", 10.0))
    + _p(TRIPS.test_random_init_regime, ("win32_border",))
)


@pytest.mark.parametrize("fn,case", INFERENCE)
def test_inference_kernels_under_poison(dirty, fn, case):
    fn(*case)


TRAINING = (
    _p(TR.test_linear_fn_gradients, (300, 90, 90))
    + _p(TR.test_conv3x3_fn_gradients, (1, 17, 33, 3, 64), (1, 16, 16, 64, 3), (1, 16, 32, 180, 45))
    + _p(TR.test_attention_fn_gradients, *[(_TC[n],) for n in ("win8_shift", "win12_ragged", "w2a_8x16_df4", "a2w_6x64_df2_odd_tiles")],
         ids=["win8_shift", "win12_ragged", "w2a_8x16_df4", "a2w_6x64_df2_odd_tiles"])
    + _p(TR.test_gemm_tn_real_widths_and_virtual_ones_column, (1,), (9,))
    + _p(TR.test_layernorm_train_kernels_match_torch, (5, 256), (777, 64))
    + _p(TR.test_cpb_table_kernels_match_torch, (1, 2, (16, 16), 4))
    + _p(TR.test_se_gate_kernels_match_torch, (3, 64, 4))
    + _p(TR.test_layer_norm_residual_matches_the_torch_chain, (250, True))
    + _p(TR.test_fused_adamw_matches_torch, ())
)


@pytest.mark.parametrize("fn,case", TRAINING)
def test_training_kernels_under_poison(dirty, fn, case):
    fn(*case)


PATCHING = (
    _p(TR.test_attention_backward_split_launches, (_TC["win12_ragged"], "2"), ids=["win12_ragged-2"])
    + _p(TR.test_head_planes_kernels_match_the_torch_chain, (257, 3, 30, True), (300, 2, 16, True))
    + _p(TR.test_se_residual_matches_the_torch_chain, (2, 64, 64, 4))
)


@pytest.mark.parametrize("fn,case", PATCHING)
def test_training_kernels_that_set_switches_under_poison(dirty, monkeypatch, fn, case):
    fn(*case, monkeypatch)


def test_clip_and_ema_step_under_poison(dirty):
    CLIP.test_norm_is_the_float64_norm_reproducible_and_scaled_exactly(CLIP.build_data())


@pytest.mark.parametrize("name", ["tiny_sr2_yaml_64", "base_sr4_yaml_32"])
def test_whole_network_forward_under_poison(dirty, name):
    MODEL.test_hip_forward_matches_reference_golden(name)


def test_whole_network_gradients_under_poison(dirty):
    TS.test_training_gradients_other_geometries_vs_oracle_autograd("tiny", "yaml", 2, (32, 32), "sr")


def test_captured_train_step_under_poison(poison_only):
    """The capture-and-replay path (where an unwritten workspace once made the captured step fail depending on what ran before):
    the fills and the guard patterns are captured with the step, so every replay starts from poisoned workspaces."""
    TG.test_graphed_train_step_follows_lr_schedule_and_resume()


# ---- (b) task, data, metric and loss kernels: clean, then dirty, on the same inputs -----------------------------------------------------
def _clean(run):
    """``run()`` with poison, guards and the LDS fill off (inside a ``dirty`` test)."""
    with _switches(False, False):
        out = run()
        torch.cuda.synchronize()
    return out


def _flat(x):
    if isinstance(x, torch.Tensor):
        return [x]
    if isinstance(x, dict):
        return [t for k in sorted(x) for t in _flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [t for v in x for t in _flat(v)]
    return []


def _same_bits(clean, got, what):
    """Every tensor of ``got`` is finite where its clean twin is and equals it bit for bit (NaN payloads included)."""
    a, b = _flat(clean), _flat(got)
    assert len(a) == len(b) and len(a) > 0, what
    for n, (c, g) in enumerate(zip(a, b)):
        assert c.shape == g.shape and c.dtype == g.dtype, (what, n)
        c, g = c.detach().contiguous().cpu(), g.detach().contiguous().cpu()
        if c.dtype.is_floating_point:
            assert bool(torch.isfinite(g)[torch.isfinite(c)].all()), (what, n, "not finite under poison")
        cb, gb = (np.ascontiguousarray(t.numpy()).reshape(-1).view(np.uint8) for t in (c, g))
        assert np.array_equal(cb, gb), (what, n, f"{int((cb != gb).sum())} bytes differ under poison")


def _twice(run, what):
    """(clean, dirty) results of ``run``; asserts the second is finite where the first is and bit-identical."""
    assert ops._POISON and ops._GUARDS and _lib._DIRTY_LDS
    clean = _clean(run)
    got = run()
    torch.cuda.synchronize()
    _same_bits(clean, got, what)
    return got


@pytest.mark.parametrize("Cn", [1, 3])
def test_jpeg_round_trip(dirty, Cn):
    """Sides that are no multiples of the 16 x 16 MCU: the edge blocks replicate, the merge pass taps the neighbour of the last
    chroma sample.  Against the int64 CPU restatement, bit for bit (tests/test_gpu_jpeg.py)."""
    x = torch.randint(0, 256, (2, Cn, 19, 37), generator=torch.Generator().manual_seed(3 + Cn)).float() / 255
    q = [10, 90]
    got = _twice(lambda: T.jpeg_roundtrip(x.to(DEV), q), f"jpeg C={Cn}")
    want = T._torch_jpeg(x, torch.tensor(q, dtype=torch.int32))
    assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    levels(got.cpu())


@pytest.mark.parametrize("name", ["ragged_same", "ragged_valid"])
def test_blur(dirty, name):
    x, taps, add, pad, want = GB.extra_case(name)
    kw = dict(want_center=True) if pad == "valid" else {}
    got = _twice(lambda: T.blur(x.to(DEV), taps.to(DEV), pad, add=add.to(DEV), **kw), name)
    lq = got[0] if pad == "valid" else got
    err, b = float((lq.cpu() - want).abs().max()), GB.bound(taps.shape[0], x)
    print(f"{name}: |hip - cpu| {err:.3e}, bound {b:.3e}")
    assert lq.shape == want.shape and err <= b
    if pad == "valid":
        Kt = taps.shape[0]
        Ho, Wo = lq.shape[-2:]
        assert torch.equal(got[1].cpu(), x[..., Kt // 2 : Kt // 2 + Ho, Kt // 2 : Kt // 2 + Wo])


def test_usm_fixture_case(dirty):
    fx = USM.Fixture()
    c = fx.cases["B"]
    x = c["x"].to(DEV)
    out, blur, mask = _twice(lambda: T.usm_sharp(x, threshold=c["threshold"], parts=True), "usm B")
    _twice(lambda: T.usm_sharp(x, threshold=c["threshold"], quantise=True), "usm B quantised")
    USM.test_kernel_on_the_fixture_at_the_decided_threshold(fx, "B")          # the fixture's bars, under poison
    assert np.abs(blur.double().cpu().numpy() - c["blur"]).max() <= USM.BLUR_TOL
    assert np.abs(out.double().cpu().numpy() - c["out"]).max() <= USM.OUT_TOL
    assert np.array_equal(mask.cpu().numpy() != 0, c["mask"])


def test_usm_31_taps(dirty):
    Kt = 31
    i = torch.arange(Kt, dtype=torch.float64) - Kt // 2
    taps = torch.exp(-i * i / (2 * (0.15 * Kt + 0.35) ** 2))
    taps = (taps / taps.sum()).float()
    x = torch.randint(0, 256, (1, 3, 70, 45), generator=torch.Generator().manual_seed(Kt)).float().div(255)
    _twice(lambda: T.hip_usm(x.to(DEV), taps.to(DEV), 0.5, 10.0, parts=True), "usm K=31")
    USM.test_other_kernel_sizes_against_the_cpu_restatement(Kt)               # decided threshold, the module's bounds, under poison


def _resize_fixture_cases():
    meta, z = RSZ.golden("imresize")
    area = lambda n: z[f"{n}__in"].numel()
    down = min((n for n, c in meta["cases"].items() if c["scale"] < 1), key=area)
    up = min((n for n, c in meta["cases"].items() if c["scale"] > 1), key=area)
    return [down, up]


@pytest.mark.parametrize("which", [0, 1], ids=["smallest_down", "smallest_up"])
def test_imresize_fixture(dirty, which):
    name = _resize_fixture_cases()[which]
    meta, z = RSZ.golden("imresize")
    c, x = meta["cases"][name], z[f"{name}__in"]
    exact, ref32 = z[f"{name}__ref64"].float(), z[f"{name}__ref32"]
    got = _twice(lambda: T.imresize(x.to(DEV), c["scale"], c["antialiasing"]), name).cpu()
    d64, d32 = (got - exact).abs().max().item(), (got - ref32).abs().max().item()
    print(f"{name} {tuple(x.shape)} x {c['scale']}: |hip - ref64| = {d64:.3e}, |hip - ref32| = {d32:.3e}")
    assert got.shape == exact.shape and d64 <= RSZ.BAR and d32 <= c["ref32_vs_ref64"] + RSZ.BAR


def test_imresize_partial_tiles_both_ways(dirty):
    x = torch.randint(0, 256, (1, 3, 263, 1001), generator=torch.Generator().manual_seed(12)).float() / 255
    got = _twice(lambda: T.imresize(x.to(DEV), 1 / 3), "imresize 263x1001 / 3")
    _twice(lambda: T.imresize(x.to(DEV), 1 / 3, quantize=True), "imresize 263x1001 / 3 quantised")
    want = T.imresize(x, 1 / 3)
    assert got.shape == want.shape and (got.cpu() - want).abs().max().item() <= RSZ.BAR


def test_demosaic(dirty):
    meta, z = TASKS.golden("dm_matlab")
    name = min(list(TASKS.dm_cases()), key=lambda n: z[f"{n}__cfa4"].numel())
    x = z[f"{name}__cfa4"]
    exact, ref32 = z[f"{name}__ref64"].float(), z[f"{name}__ref32"]
    rgb = TASKS._rgb_from_cfa4(x)
    for what, run in (("cfa4", lambda: T.dm_matlab(x.to(DEV))), ("rgb", lambda: T.demosaic_gt(rgb.to(DEV)))):
        got = _twice(run, f"{name} {what}").cpu()
        if name in meta["eight_bit"]:
            assert torch.equal(got, exact), what
        else:
            assert (got - exact).abs().max() <= 1e-6, what
        assert (got - ref32).abs().max() <= TASKS.REF32, what


def test_image_metrics(dirty):
    z = MET._golden()
    inputs = {n: MET._inputs(z, n) for n in MET._cases()}
    name = min((n for n, (r, t, s) in inputs.items() if s > 1 and r.shape[1] == 3), key=lambda n: inputs[n][0].numel())
    r, t, scale = inputs[name]
    _twice(lambda: M.hip_image_metrics(r.to(DEV), t.to(DEV), scale, 63), f"{name} all six metrics")
    for group in MET._groups(3):
        got = _twice(lambda: M.image_metrics(r.to(DEV), t.to(DEV), group, scale), f"{name} {group}")
        MET.check_against_golden(z, name, group, got)


def test_niqe(dirty):
    shape, seed = (3, 1, 389, 300), 2
    x = NIQE._textures(*shape, seed)
    got_f = _twice(lambda: M.niqe_features(x.to(DEV)), "niqe features")
    got = _twice(lambda: M.niqe(x.to(DEV), NIQE.PARAMS), "niqe")
    NIQE.check_features(got_f, M.niqe_features(x), shape)
    assert (got.cpu() - M.niqe(x, NIQE.PARAMS)).abs().max().item() <= NIQE.PATH_SCORE_BAR


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("scale,patch", [(1, 33), (2, PAT.P)])
def test_patches(dirty, channels, scale, patch):
    lq_imgs, gt_imgs, work, want_lq, want_gt = PAT.reference_case(channels, scale, patch)
    with _switches(False, False):
        gpu = PatchSampler("sr", PatchStore(gt_imgs, DEV), PatchStore(lq_imgs).to(DEV), patch=patch, batch=PAT.B, scale=scale)
    lq, gt = _twice(lambda: gpu.next(work), f"patches C={channels} x{scale} P={patch}")
    assert torch.equal(lq.cpu(), want_lq) and torch.equal(gt.cpu(), want_gt)


def test_dual_pixel_batch(dirty):
    patch, batch = 33, 3
    left, right, gt, work, want_lq, want_gt = DP.reference_batch(patch, batch)
    with _switches(False, False):
        L_, R_, G = DP.stores(DEV)
        gpu = PatchSampler("sr", G, L_, patch=patch, batch=batch, lq_r_store=R_)
    lq, g = _twice(lambda: gpu.next(work), "dual-pixel batch")
    assert lq.shape == (batch, 6, patch, patch) and torch.equal(lq.cpu(), want_lq) and torch.equal(g.cpu(), want_gt)


@pytest.mark.parametrize("name", ["odd_crop", "dual_pixel"])
def test_remix(dirty, name):
    (lq, gt), scale, p, plan = RMX.CASES[name]
    plan = plan()
    got = _twice(lambda: R.batch_remix(lq.to(DEV), gt.to(DEV), plan, scale, patch=p), name)
    want = R.batch_remix(lq, gt, plan, scale, patch=p)
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


def test_jitter_mixed_list(dirty):
    cs = JIT.kernel_cases()
    imgs, params = [c["x"].to(DEV) for c in cs], [c["params"] for c in cs]
    out, means = _twice(lambda: J.color_jitter(imgs, params, with_means=True), "jitter")
    worst = worst_mean = 0.0
    for c, o, m in zip(cs, out, means.cpu().tolist()):
        want, want_mean = J.jitter_image(c["x"].double(), c["params"], with_mean=True)
        worst = max(worst, float((o.double().cpu() - want).abs().max()))
        worst_mean = max(worst_mean, abs(m - float(want_mean)))
    print(f"jitter: worst {worst:.3e} (bar {JIT.BAR:.3e}), worst mean {worst_mean:.3e} (bar {JIT.E_FP32:.3e})")
    assert worst <= JIT.BAR and worst_mean <= JIT.E_FP32


def test_isp_jump_case(dirty):
    with _switches(False, False):
        cases = ISP.build_cases(ISP.build_banks())
    cs = cases["jump"]
    _twice(lambda: ISP._launch_all(cs), "isp jump")
    ISP.test_kernels_against_the_float64_restatement(cases, "jump")


def test_bsr_degrade_mixed_lists(dirty):
    """tests/test_gpu_degrade.py's mixed lists around the 16 x 16 tile for three channels, through item_lists (pack, launch, slice)."""
    Cn = 3
    g = torch.Generator().manual_seed(7 + Cn)
    xs = [torch.rand(Cn, h, w, generator=g) for h, w in GD.TILE_SHAPES]
    imgs, sizes, interps = [], [], []
    for x in xs:
        h, w = x.shape[1:]
        for size in ((max(1, h // 2), max(1, (w + 2) // 3)), (2 * h + 1, 3 * w - 1)):
            for ip in (1, 2, 3):
                imgs.append(x), sizes.append(size), interps.append(ip)
    got = _twice(lambda: BD.cv_resize([x.to(DEV) for x in imgs], sizes, interps), "cv_resize")
    want = BD.cv_resize([x.double() for x in imgs], sizes, interps)
    for x, size, ip, gi, w in zip(imgs, sizes, interps, got, want):
        err, b = float((gi.double().cpu() - w).abs().max()), GD.resize_bound(ip, x.shape[1], x.shape[2], *size)
        assert gi.shape == w.shape and err <= b, (tuple(x.shape), size, ip, err, b)
    taps = {1: torch.ones(1, 1), 31: torch.rand(31, 31, generator=g)}
    taps[31] = taps[31] / taps[31].sum()
    imgs, ks, strides = [], [], []
    for x in xs:
        for Kt in (1, 31):
            for s in (1, 2, 5):
                imgs.append(x), ks.append(Kt), strides.append(s)
    got = _twice(lambda: BD.blur_items([x.to(DEV) for x in imgs], [taps[k] for k in ks], strides), "blur_items")
    want = BD.blur_items([x.double() for x in imgs], [taps[k].double() for k in ks], strides)
    for x, Kt, s, gi, w in zip(imgs, ks, strides, got, want):
        err, b = float((gi.double().cpu() - w).abs().max()), GD.blur_bound(Kt, x)
        assert gi.shape == w.shape and err <= b, (tuple(x.shape), Kt, s, err, b)


@pytest.mark.parametrize("hw", [(3, 5), (33, 65)], ids=ENS.ids)
def test_ensemble_pack_and_merge(dirty, hw):
    H, W = hw
    x = ENS.values((2, 3, H, W), seed=23)
    a, b = _twice(lambda: E.dihedral_pack(x.to(DEV)), "dihedral_pack")
    wa, wb = E.dihedral_pack(x)
    assert torch.equal(a.cpu(), wa) and torch.equal(b.cpu(), wb)
    sq = ENS.values((1, 3, H, H), seed=24)                     # square: one buffer of eight
    a, b = _twice(lambda: E.dihedral_pack(sq.to(DEV)), "dihedral_pack square")
    wa, wb = E.dihedral_pack(sq)
    assert torch.equal(a.cpu(), wa) and torch.equal(b.cpu(), wb) and b.data_ptr() == a.data_ptr() + a.numel() * 4
    for dtype in (torch.float32, torch.float16):
        vs = [ENS.values((2, 3, W, H) if k % 2 else (2, 3, H, W), seed=230 + k, dtype=dtype) for k in range(8)]
        got = _twice(lambda: E.dihedral_merge([v.to(DEV) for v in vs]), f"dihedral_merge {dtype}")
        assert ENS.same(got, E.dihedral_merge(vs))
        assert ENS.same(_twice(lambda: E.dihedral_merge(ENS.eight_views(vs)), f"dihedral_merge views {dtype}"), E.dihedral_merge(vs))


@pytest.mark.parametrize("shape,rep", [((2, 3, 5, 7), 1), ((1, 3, 67, 129), 1), ((1, 3, 4, 5), 3)], ids=["2x3x5x7", "1x3x67x129", "rep3"])
def test_image8(dirty, shape, rep):
    x = I8.adversarial(shape, 400)
    got = _twice(lambda: I.pack8(x.to(DEV), rep), f"pack8 {shape} rep {rep}")
    assert torch.equal(got.cpu(), I._torch_pack8(x, rep))


def test_lpips_tap(dirty):
    B, C, H, W = 2, 64, 5, 7
    f, w = LPIPS._tap_inputs(B, C, H, W, seed=C + H)
    tok, wd = LPIPS._tok(f).to(DEV), w.to(DEV)

    def run():
        out = torch.full((B,), 5.0, dtype=torch.float64, device=DEV)
        pooled = ops.lpips_tap(tok, wd, B, H, W, out, accumulate=False)
        return out, pooled

    _twice(run, "lpips tap")
    LPIPS.test_tap_kernel_against_float64_torch(C, H, W)


def test_vgg_tap_kernels(dirty):
    B, C, H, W = 2, 64, 6, 10
    fx, fg = PERC._tap_inputs(B, C, H, W, seed=C + H)
    tx, tg = PERC._tok(fx), PERC._tok(fg)
    dpool = PERC._tok(torch.randn(B, C, H // 2, W // 2, generator=torch.Generator().manual_seed(3)).cuda())

    def run():
        loss, lsum = torch.full((1,), 5.0, device="cuda"), torch.zeros(1, device="cuda")
        pooled = ops.vgg_tap(tx, tg, B, H, W, loss, 0.37 / fx.numel(), accumulate=False, pool=True, pool_dtype=torch.float16, layer_sum=lsum)
        return loss, lsum, pooled, ops.vgg_tap_bwd(tx, tg, B, H, W, 3 * 0.37 / fx.numel(), dpool)

    _twice(run, "vgg tap")
    PERC.test_tap_kernels_against_torch(B, C, H, W, True, torch.float16)


@pytest.mark.parametrize("nb,C,hw", [STYLE.KSHAPES[0], (1, 256, 1)])
def test_gram_forward_and_backward(dirty, nb, C, hw):
    f = STYLE._features(nb, C, hw).cuda()
    g = torch.Generator().manual_seed(9)
    D, d0 = torch.randn(nb, C, C, generator=g).cuda(), torch.randn(nb * hw, C, generator=g)

    def run():
        rb = torch.zeros(nb, dtype=torch.float32, device="cuda")
        d = d0.cuda()
        ops.vgg_gram_bwd(f, D, hw, 0.37, d)
        return ops.vgg_gram(f, nb, hw, rowbound=rb), rb, d

    _twice(run, "gram")
    if (nb, C, hw) in STYLE.KSHAPES:
        STYLE.test_gram_forward_against_float64(nb, C, hw)
        STYLE.test_gram_backward_adds_into_the_gradient_matrix(2, C, hw)
    else:
        Gm = run()[0]
        g64, g32 = STYLE._gram_refs(f.cpu(), nb, C, hw)
        err, ref = float((Gm[0].cpu().double() - g64[0]).abs().max()), float((g32[0].double() - g64[0]).abs().max())
        assert err <= 4 * ref, (err, ref)
        STYLE.test_gram_backward_adds_into_the_gradient_matrix(nb, C, hw)


def test_discriminator_fixture(dirty):
    """Forward and gradients of the nf = 8 reference fixture at the module's bars; the eval logits also bit for bit against the
    clean run (the gradients accumulate with fp32 atomics: the module's bars stand in)."""
    with _switches(False, False):
        nets = DISC.build_nets()
        _, gpu = DISC._pair(nets, 8)
        gpu.eval()
    x = torch.from_numpy(DISC._fixture_state()[1]["d__A__x"]).cuda()

    def run():
        with torch.no_grad():
            return gpu(x)

    _twice(run, "discriminator eval logits")
    DISC.test_whole_discriminator(nets, 8, (2, 3, 16, 24))
