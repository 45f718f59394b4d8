"""GRL_DETERMINISTIC=1 on the GPU: the kernel paths and launch shapes that only this switch reaches -- needs the MI355X.

The switch promises bit-identical training gradients run to run (README, DESIGN Knobs, INTEGRATION ABI 21, switches.py).  It routes
the backward pass through code the rest of the suite never executes:

  grl_gemm_tn        c_fix / c_bias_fix: every slab's partial tile as round(acc * 2^30) added with 64-bit integer atomics, converted
                     back by ops.gemm_tn (c_fix * 2^-30 * out_scale)                                         -> section 1
  grl_attention_bwd  d_table_fix: no split launches, attn_dq_kernel with ONE wave (64 queries) per workgroup -- at Nq > 64 several
                     one-wave workgroups per window, each with its own table window -- and fix_add (2^32 x the g_scale-d value) at
                     the Toeplitz ring, the per-pair scatter and the LDS-histogram flush                     -> section 2
  se_mlp_bwd         parallel = 0: one workgroup walks the batch; se_colsum: torch's reduction              -> section 3
  torch fall-backs   LayerNorm, LayerNorm + residual, CPB tables, head planes                               -> section 4 (whole network)

Checkers.  gemm_tn: float64 sums of the fp16-rounded operands, sum_m r16(a_scale a[m, n]) r16(b[row(m, tap), k]) / a_scale, with the
DERIVED bound  out_scale * (M * 2^-24 * sum_m |terms| + splits * 2^-31)  per element (terms in the a_scale-d domain: fp32
accumulation of at most M terms, then one rounding to 2^-30 per slab).  Attention: the closed form of oracle/backward_math.py at
the project's 1e-2 norm-wise bar (tests/test_gpu_train.py).  Squeeze-excite: the torch chain at the bars of the default-mode tests.
Whole network: the bars of the default-mode tests, called as they are.  Bit identity is torch.equal, no tolerance.

attn_dq_kernel instance per ATT_CASES entry in the mode (launcher arithmetic: blk = 64 queries, tab_window = window_floats(64, ...),
GHIST iff 2 * 4 * tab_window + 25 472 B > 160 KiB, i.e. tab_window > 17 296 floats; `default` = the 256-query launch for comparison):

  case                        tab_window (mode)   default   instance   table-gradient path
  win8_shift                        228              228     <false>    per-pair LDS scatter -> fix_add flush
  win32_shift                     2 148            2 524     <false>    Toeplitz ring (LDS)  -> fix_add flush
  win32_shift8                    2 148            2 524     <false>    Toeplitz ring (LDS)  -> fix_add flush   (border windows: tile<0>)
  win12_ragged                      440              532     <false>    per-pair LDS scatter -> fix_add flush
  win16_d32                         624              964     <false>    per-pair LDS scatter -> fix_add flush
  a2w_64_df2                      6 276            6 844     <false>    Toeplitz ring (LDS)  -> fix_add flush
  w2a_64_df2                      3 140            3 424     <false>    Toeplitz ring (LDS)  -> fix_add flush
  a2w_48x96_df4                   6 192            7 024     <false>    per-pair LDS scatter -> fix_add flush
  w2a_8x16_df4                      120              172     <false>    per-pair LDS scatter -> fix_add flush
  w2a_64x128_df2_bigtable         6 500            6 500     <false>    Toeplitz ring (LDS)  -> fix_add flush
  a2w_64x128_df2_bigtable        12 420           12 992     <false>    Toeplitz ring (LDS)  -> fix_add flush
  a2w_6x64_df2_odd_tiles            760              760     <false>    Toeplitz ring (LDS)  -> fix_add flush

No shipped geometry reaches attn_dq_kernel<true>, in the mode or out of it: since the per-workgroup table windows the largest
window (a2w 64x128 /2, 12 992 floats) fits LDS twice.  The two fix_add call sites inside `if constexpr (GHIST)` (ring and scatter
with ftab != nullptr) are therefore not executed by any test here; the flush is the one that runs.  (test_dq_instances_in_the_mode
recomputes the table from the launcher's formulas.)

Sources of run-to-run difference found with these tests, and their fixes:
  se_colsum_kernel  ceil(rows_per_image / 64) fp32 atomics per address in hardware order, in the forward (the CAB's average pool) and
                    the backward (d_gate) of SeResidualFn, whatever the switch said.  Fix: ops.se_colsum takes torch's reduction in
                    the mode.  Before the fix, in the mode: both restorer tests had EVERY tensor differ between two passes (158 of
                    158 and 152 of 152, the loss included), test_se_residual_in_the_mode[2-4096-180-10] differed in y, d_u and
                    all four parameter gradients; the kernel launch alone: see the table.

Out of scope: GraphedTrainStep under the switch.

Measured on an MI355X, 2026-10-20 (figure / bound):
  gemm_tn taps 1, fp32 b, b_ones (4 slabs)    max|c - ref| 2.03e-11 / 2.31e-08 there; max err/bound 8.8e-04 / 1; bias 1.6e-04 / 1
  gemm_tn taps 1, fp16 b; fp16 a and b        the same figures (the same fp16 operands reach the MFMA)
  gemm_tn taps 9, b_ones (2 slabs)            max|c - ref| 6.30e-12 / 3.28e-09 there; max err/bound 2.0e-03 / 1; bias 5.4e-05 / 1
  gemm_tn taps 16 (1 slab)                    max|c - ref| 1.21e-12 / 5.57e-11 there; max err/bound 4.9e-02 / 1
  gemm_tn headroom                            128.0 and -128.0, exact
  every gemm_tn case                          3 calls torch.equal
  attention, worst of dq dk dv dscale dbias   win8_shift 5.0e-04, win32_shift 6.5e-04, win12_ragged 5.2e-04, win16_d32 6.0e-04,
    (each / 1e-2)                             win32_shift8 2.7e-03, a2w_64_df2 4.2e-03, w2a_64_df2 9.6e-04, a2w_48x96_df4 2.7e-03, w2a_8x16_df4 6.6e-04,
                                              w2a_64x128_df2_bigtable 6.4e-04, a2w_64x128_df2_bigtable 6.5e-04, a2w_6x64_df2_odd_tiles 1.4e-03
  attention, every case                       2 runs torch.equal in all five; SPLITS=3 torch.equal; dk, dv torch.equal to the default
                                              unsplit launch; max|dq - dq(default)| 0 in every case (not asserted); max|dbias -
                                              dbias(default)| 5.5e-12 .. 1.1e-10
  se_mlp parallel = 0, worst of six           B8 1.6e-07, B3 1.2e-07, B16 3.5e-07, B1 1.6e-07 / 2e-5; 2 runs torch.equal
  se_residual in the mode, worst of seven     HW4096 1.3e-07, HW100 2.4e-07 / 3e-5; 3 runs torch.equal
  se_colsum KERNEL, 10 launches, B2 C180      HW4096: pool 9 of 9 repeats differ (up to 275 of 360 elements, 1.8e-07 of 0.35), d_gate 9 of 9
    (what the mode ran before the fix)        (up to 309 of 360, 7.6e-05 of 237); HW100 (2 partials per address): 0 of 9
  restorer base 2x2 x4 64x64                  fixture bars hold (loss 0.092266 / 0.092261 +- 2e-4, worst gradient 6.6e-03 / 2e-2); tensors
                                              that differ between two passes: the mode 0 / 0 of 158; default mode 158 (for the record)
  restorer base deblur 48x96                  the mode 0 / 0 of 152; default mode 152 (for the record)
  discriminator nf8_fixture                   its own bounds hold; gradients that differ: the mode 0 / 0 of 12; default mode 6 (for the record)
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U24, U31 = 2.0 ** -24, 2.0 ** -31


@pytest.fixture
def det(monkeypatch):
    monkeypatch.setenv("GRL_DETERMINISTIC", "1")
    return monkeypatch


# ---- 1. grl_gemm_tn, fixed-point accumulation ----------------------------------------------------------------------------------
def _r16(t):
    """Round to fp16 as the kernel's loader does (fp32 value -> fp16, round to nearest even), returned in float64."""
    return t.float().half().double()


def _splits(M, N, K, taps, b_ones):
    """The slab count ops.gemm_tn picks (default GRL_GEMM_TN_WGS)."""
    tiles = ((N + 63) // 64) * ((K + int(b_ones) + 63) // 64) * taps
    wgs = 512 if tiles <= 9 else (1536 if tiles >= 81 else 1024)
    return max(1, min((M + 255) // 256, (wgs + tiles - 1) // tiles))


def _pow2_scale(a):
    """Power of two that brings max|a| to about 64."""
    return 2.0 ** round(math.log2(64.0 / float(a.abs().max())))


def _tap_rows(b, taps, hw, images):
    """[taps, M, K]: b[row(m, tap), :] per tap (zero outside the image), by explicit shifted slices -- b is [rows, K] in float64."""
    K = b.shape[1]
    if taps == 1:
        return b.unsqueeze(0)
    H, W = hw
    if taps == 9:
        bp = F.pad(b.view(images, H, W, K), (0, 0, 1, 1, 1, 1))
        return torch.stack([bp[:, t // 3 : t // 3 + H, t % 3 : t % 3 + W].reshape(-1, K) for t in range(9)])
    bp = F.pad(b.view(images, 2 * H, 2 * W, K), (0, 0, 1, 1, 1, 1))             # input pixel (2y + ky - 1, 2x + kx - 1)
    return torch.stack([bp[:, t // 4 : t // 4 + 2 * H : 2, t % 4 : t % 4 + 2 * W : 2].reshape(-1, K) for t in range(16)])


def _gemm_tn_check(label, a, b, N, K, taps, hw, images, b_ones, a_scale, a16=None, b16=False):
    """Run ops.gemm_tn three times in the mode; compare with the float64 sums of the fp16-rounded operands at the derived bound."""
    from grl_image_restoration_amd import ops

    M = a.shape[0]
    out_scale = 1.0 / a_scale
    a_s = _r16(a * a_scale)[:, :N] if a16 is None else a16.double()[:, :N]       # the a_scale-d operand as the MFMA sees it
    rows = _tap_rows(_r16(b)[:, :K], taps, hw, images)                          # [taps, M, K]
    ref = torch.einsum("mn,tmk->tnk", a_s, rows) * out_scale
    tot = torch.einsum("mn,tmk->tnk", a_s.abs(), rows.abs())                     # sum_m |terms|, a_scale-d domain
    splits = _splits(M, N, K, taps, b_ones)
    bound = out_scale * (M * U24 * tot + splits * U31)
    ad = (a if a16 is None else a16).cuda()
    bd = b.cuda().half() if b16 else b.cuda()
    outs = [ops.gemm_tn(ad, bd, N, K, taps=taps, hw=hw, a_scale=a_scale, out_scale=out_scale, b_ones=b_ones) for _ in range(3)]
    cs = [o[0] if b_ones else o for o in outs]
    assert cs[0].shape == (taps, N, K) and cs[0].dtype == torch.float32
    err = (cs[0].double().cpu() - ref).abs()
    worst = float((err / bound).max())
    print(f"gemm_tn fix {label}: splits {splits}; max|c - ref| {float(err.max()):.3e}, bound there {float(bound.flatten()[err.argmax()]):.3e}; "
          f"max err/bound {worst:.3e} (bound 1)")
    assert bool((err <= bound).all()), (label, worst)
    assert all(torch.equal(cs[0], c) for c in cs[1:]), label
    if b_ones:                                                                   # bias: the centre tap's column sums of a
        cbs = [o[1] for o in outs]
        assert cbs[0].shape == (N,)
        refb = a_s.sum(0) * out_scale
        boundb = out_scale * (M * U24 * a_s.abs().sum(0) + splits * U31)
        errb = (cbs[0].double().cpu() - refb).abs()
        print(f"gemm_tn fix {label}: bias max|d| {float(errb.max()):.3e}, max err/bound {float((errb / boundb).max()):.3e} (bound 1)")
        assert bool((errb <= boundb).all()), label
        assert all(torch.equal(cbs[0], c) for c in cbs[1:]), label


def test_gemm_tn_fixed_point_taps1(det):
    """M = 777, N = 68, K = 36: 4 slabs (7 + 7 + 7 + 4 pieces of 32 rows, the last piece 9 rows), N and K + 1 cross a 64-tile edge."""
    g = torch.Generator().manual_seed(61)
    M, N, K = 777, 68, 36
    a, b = torch.randn(M, N, generator=g) * 1e-6, torch.randn(M, K, generator=g)
    s = _pow2_scale(a)
    _gemm_tn_check("taps1 fp32 b, b_ones", a, b, N, K, 1, None, 1, True, s)
    # fp16 b: rows in 16-byte pieces (ldb = 40); then fp16 a as the data-gradient launch leaves it: pre-scaled, lda = 72
    b40 = F.pad(b, (0, 4))
    _gemm_tn_check("taps1 fp16 b", a, b40, N, K, 1, None, 1, False, s, b16=True)
    a16 = F.pad(a * s, (0, 4)).half()
    _gemm_tn_check("taps1 fp16 a, fp16 b", a, b40, N, K, 1, None, 1, False, s, a16=a16, b16=True)


def test_gemm_tn_fixed_point_taps9(det):
    """3 images of 9 x 11 pixels, N = 12, K = 20: border pixels carry most of the rows; the bias is the centre tap's column sum."""
    g = torch.Generator().manual_seed(62)
    images, hw, N, K = 3, (9, 11), 12, 20
    M = images * hw[0] * hw[1]
    a, b = torch.randn(M, N, generator=g) * 1e-6, torch.randn(M, K, generator=g)
    _gemm_tn_check("taps9 b_ones", a, b, N, K, 9, hw, images, True, _pow2_scale(a))


def test_gemm_tn_fixed_point_taps16(det):
    """4x4 stride-2 taps: output grid 3 x 5, input grid 6 x 10, 2 images, N = 16, K = 8."""
    g = torch.Generator().manual_seed(63)
    images, hw, N, K = 2, (3, 5), 16, 8
    M = images * hw[0] * hw[1]
    a, b = torch.randn(M, N, generator=g) * 1e-6, torch.randn(4 * M, K, generator=g)
    _gemm_tn_check("taps16", a, b, N, K, 16, hw, images, False, _pow2_scale(a))


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_gemm_tn_fixed_point_headroom_exact(det, sign):
    """a_scale a = 64, b = 2^14, M = 2048: every product and partial sum is a power of two, exact in fp32; the a_scale-d sum is 2^31 and
    its fixed-point image 2^61 (usable range |sum| < 2^33, include/grl_hip.h).  The result is M a b exactly."""
    from grl_image_restoration_amd import ops

    M, N, K, a_scale = 2048, 4, 4, 2.0 ** 24
    a = torch.full((M, N), sign * 64.0 / a_scale).cuda()
    b = torch.full((M, K), 2.0 ** 14).cuda()
    c = ops.gemm_tn(a, b, N, K, a_scale=a_scale, out_scale=1.0 / a_scale)
    want = sign * M * (64.0 / a_scale) * 2.0 ** 14
    print(f"gemm_tn fix headroom: c[0, 0, 0] {float(c[0, 0, 0])!r}, exact {want!r}")
    assert c.shape == (1, N, K) and torch.equal(c.cpu(), torch.full((1, N, K), want))


# ---- 2. grl_attention_bwd with d_table_fix -------------------------------------------------------------------------------------
def _window_floats(blk, ww, wh, other_h, D, trows):
    rows = blk // ww if blk % ww == 0 else (blk - 1) // ww + 2
    rows = min(rows, wh)
    return min(((rows + other_h - 1) * D + D + 6) & ~3, (trows + 3) & ~3)


def _dq_launch(case, deterministic):
    """(tab_window, GHIST) of the attn_dq_kernel launch of one ATT_CASES entry, from the launcher's own arithmetic."""
    _, mode, _, win, _, df, _, _ = case[:8]
    awin = (win[0] // df, win[1] // df)
    q, k = {"w": (win, win), "a2w": (awin, win), "w2a": (win, awin)}[mode]
    Nq, D = q[0] * q[1], q[1] + k[1] - 1
    trows = (q[0] + k[0] - 1) * D
    waves = 1 if deterministic else min(4, (Nq + 63) // 64)
    tw = _window_floats(waves * 64, q[1], q[0], k[0], D, trows)
    rest = 2 * 128 * 64 + 32 * (128 * 2 + 8) + 128 * 4 + 128
    return tw, 2 * 4 * tw + rest > 160 * 1024


def test_dq_instances_in_the_mode():
    """The table of the module docstring: which attn_dq_kernel instance every case takes (no launch: host arithmetic only)."""
    from tests.test_gpu_train import ATT_CASES

    for case in ATT_CASES:
        (tw, gh), (tw0, gh0) = _dq_launch(case, True), _dq_launch(case, False)
        print(f"{case[0]:28s} tab_window {tw:6d} (default {tw0:6d})  attn_dq_kernel<{str(gh).lower()}> (default <{str(gh0).lower()}>)")
        assert not gh and not gh0          # the docstring's statement; a geometry that changes it must be written down there


def _att_cases():
    from tests.test_gpu_train import ATT_CASES

    return ATT_CASES


@pytest.mark.parametrize("case", _att_cases(), ids=[c[0] for c in _att_cases()])
def test_attention_bwd_in_the_mode(case, monkeypatch):
    """Closed form at the project's bar, two runs bit-identical, dk / dv bit-identical to the unsplit default launch, and the split
    switch without effect in the mode."""
    from tests.test_gpu_train import attention_fn_case

    keys = ("dq", "dk", "dv", "dscale", "dbias")
    monkeypatch.setenv("GRL_DETERMINISTIC", "1")
    errs, g1 = attention_fn_case(case)
    print(f"{case[0]} mode: worst error {max(errs.values()):.3e} (bound 1e-2)")
    assert max(errs.values()) < 1e-2, errs
    _, g2 = attention_fn_case(case)
    diff = [k for k in keys if not torch.equal(g1[k], g2[k])]
    assert not diff, (case[0], "two runs in the mode differ in", diff)
    monkeypatch.setenv("GRL_ATTN_BWD_SPLITS", "3")
    _, g3 = attention_fn_case(case)
    diff = [k for k in keys if not torch.equal(g1[k], g3[k])]
    assert not diff, (case[0], "GRL_ATTN_BWD_SPLITS=3 changes the mode's result in", diff)
    monkeypatch.setenv("GRL_DETERMINISTIC", "0")
    monkeypatch.setenv("GRL_ATTN_BWD_SPLITS", "1")
    _, g0 = attention_fn_case(case)
    print(f"{case[0]} mode vs default (unsplit): max|dq - dq0| {float((g1['dq'] - g0['dq']).abs().max()):.3e} of max|dq| "
          f"{float(g0['dq'].abs().max()):.3e} (not asserted); max|dbias - dbias0| {float((g1['dbias'] - g0['dbias']).abs().max()):.3e}")
    assert torch.equal(g1["dk"], g0["dk"]) and torch.equal(g1["dv"], g0["dv"]), case[0]


# ---- 3. the squeeze-excite path -----------------------------------------------------------------------------------------------
def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("B,C,Cmid", [(8, 180, 10), (3, 64, 4), (16, 256, 64), (1, 180, 10)])
def test_se_mlp_bwd_one_workgroup_walks_the_batch(det, B, C, Cmid):
    from tests.test_gpu_train import se_gate_case

    kernel, ref = se_gate_case(B, C, Cmid)
    worst = max(_rel(a, b) for a, b in zip(kernel, ref))
    print(f"se_mlp (parallel = 0) B{B} C{C} Cmid{Cmid}: worst relative error {worst:.3e} (bound 2e-5)")
    for a, b in zip(kernel, ref):
        assert a.shape == b.shape and _rel(a, b) < 2e-5
    again = se_gate_case(B, C, Cmid)[0]
    assert all(torch.equal(a, b) for a, b in zip(kernel, again))


@pytest.mark.parametrize("B,HW,C,Cmid", [(2, 4096, 180, 10), (2, 100, 180, 10)])
def test_se_residual_in_the_mode(det, B, HW, C, Cmid):
    """64 column-sum partials per address (4096 rows per image) and a ragged last partial (100 rows): forward and all six gradients
    bit-identical over three runs, and at the default-mode bar against the torch chain."""
    from tests.test_gpu_train import se_residual_case

    names = ("y", "d_x1", "d_u", "d_w1", "d_b1", "d_w2", "d_b2")
    kernel, ref = se_residual_case(B, HW, C, Cmid, det)
    worst = max(_rel(a, b) for a, b in zip(kernel, ref))
    print(f"se_residual in the mode B{B} HW{HW}: worst relative error {worst:.3e} (bound 3e-5)")
    for a, b in zip(kernel, ref):
        assert a.shape == b.shape and _rel(a, b) < 3e-5
    for _ in range(2):
        again = se_residual_case(B, HW, C, Cmid, det, modes=("1",))[0]
        diff = [n for n, a, b in zip(names, kernel, again) if not torch.equal(a, b)]
        assert not diff, diff


# ---- 4. whole network -----------------------------------------------------------------------------------------------------------
def _two_passes(m, x0, gt):
    """Two forward + backward passes from grad = None: [(loss, input gradient, {name: gradient})] x 2."""
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        loss = (m(x) - gt).abs().mean()
        loss.backward()
        runs.append((loss.detach().clone(), x.grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    return runs


def _differing(runs):
    (l1, x1, g1), (l2, x2, g2) = runs
    assert set(g1) == set(g2)
    out = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    return (["loss"] if not torch.equal(l1, l2) else []) + (["input gradient"] if not torch.equal(x1, x2) else []) + out


def _restorer_identity(label, m, x, gt, monkeypatch, n_params=None):
    monkeypatch.setenv("GRL_DETERMINISTIC", "0")
    diff0 = _differing(_two_passes(m, x, gt))
    monkeypatch.setenv("GRL_DETERMINISTIC", "1")
    runs = _two_passes(m, x, gt)
    diff = _differing(runs)
    n = len(runs[0][2])
    print(f"{label}: tensors that differ between two passes: default mode {len(diff0)} of {n + 2} (for the record), the mode {len(diff)} (bound 0)")
    if diff:
        print(f"{label}: differ in the mode: " + ", ".join(diff))           # every name, not the first
    assert n_params is None or n == n_params
    assert not diff, (label, len(diff))


def test_restorer_training_step_in_the_mode(monkeypatch):
    """GRL-Base 2 x 2 blocks, x4, 64 x 64 LQ: the fixture bars of the default-mode test hold in the mode, and two passes give the same
    bits for the loss, the input gradient and all 156 parameter gradients."""
    from grl_image_restoration_amd import GRL
    from oracle import grl_oracle as O
    from tests import test_gpu_train_step as TS

    monkeypatch.setenv("GRL_DETERMINISTIC", "1")
    TS.test_training_step_gradients_match_reference()
    meta, z = TS._grad_fixture()
    m = GRL(**meta["cfg"]).eval()
    m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, meta["weight_seed"]), strict=True)
    m = m.cuda()
    _restorer_identity("restorer base 2x2 sr4 64x64", m, torch.from_numpy(z["input"]).cuda(), torch.from_numpy(z["target"]).cuda(), monkeypatch, 156)


def test_restorer_other_geometry_in_the_mode(monkeypatch):
    """("base", "deblur", 1, (48, 96)): window 12, non-Toeplitz tables, the CAB -- bit identity of two passes."""
    from grl_image_restoration_amd import GRL, make_config
    from oracle import grl_oracle as O

    hw = (48, 96)
    cfg = make_config("base", "deblur", upscale=1, img_size=hw[0], depths=[2, 2], num_heads_window=[3, 3], num_heads_stripe=[3, 3])
    m = GRL(**cfg).eval()
    m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 3), strict=True)
    m = m.cuda()
    lq, gt = O.synthetic_pair("deblur", hw, 1, batch=2, seed=31)
    lq, gt = lq[..., : hw[0], : hw[1]].contiguous(), gt[..., : hw[0], : hw[1]].contiguous()
    _restorer_identity("restorer base deblur 48x96", m, lq.cuda(), gt.cuda(), monkeypatch)


def test_discriminator_in_the_mode(monkeypatch):
    """nf8_fixture of test_whole_discriminator under the switch (grl_gemm_tn at taps 16 in fixed point): its emulation-derived bounds
    hold, and the D-loss gradients of two runs are the same bits."""
    from tests import test_gpu_disc as TD

    monkeypatch.setenv("GRL_DETERMINISTIC", "1")
    sd, z = TD._fixture_state()
    nets = {8: sd}
    TD.test_whole_discriminator(nets, 8, (2, 3, 16, 24))
    x, xf = torch.from_numpy(z["d__A__x"]).cuda(), torch.from_numpy(z["d__A__xf"]).cuda()
    grads = {}
    for mode in ("1", "1", "0", "0"):
        monkeypatch.setenv("GRL_DETERMINISTIC", mode)
        _, gpu = TD._pair(nets, 8)
        (TD._bce(gpu(x), True) + TD._bce(gpu(xf), False)).backward()
        grads.setdefault(mode, []).append({k: p.grad.clone() for k, p in gpu.named_parameters()})
    diff = {mode: [k for k in a if not torch.equal(a[k], b[k])] for mode, (a, b) in grads.items()}
    print(f"discriminator nf8: gradients that differ between two runs: default mode {len(diff['0'])} of {len(grads['0'][0])} (for the record), "
          f"the mode {len(diff['1'])} (bound 0)")
    assert not diff["1"], diff["1"]
