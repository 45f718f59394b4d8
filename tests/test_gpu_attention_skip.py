"""Row-streaming attention kernel, round 8: a workgroup in a bottom-border window (stripe) of a shifted view steps over the key
chunks of the other row region, whose softmax weights are fp16 zeros (DESIGN.md section 5 states the bound), and runs the unmasked
statement when no column border is left (csrc/attention_rows.hip, rows_visit).

  * every shape against the float64 softmax of the same fp16-rounded operands, built as in tests/test_gpu_kernels.py::_attention_case
    with that function's tolerances: 1.5e-3 (x 3 at scale 100) x max(1, |ref|max) on the output, 2e-3 on the log2-sum-exp2;
  * aimed cases in the manner of tests/test_gpu_attention_trips.py with the visiting order of the new rule: peaks in the first and
    the last VISITED chunk and a staircase that trips in every visited chunk (buffer parity, prefetch and prime count visits);
  * invariance: key / value rows of the other row region hold large finite values or zeros -- outputs and log-sum-exp are equal
    bit for bit (in the old kernel their weights were fp16 zeros, in the new one they are not read); and, as the proof that the
    rule is in force on the GPU, NaN in the V rows of the chunks stepped over does not reach the output;
  * the mirror of the rule on the CPU: chunk counts per workgroup, and every chunk stepped over is masked for every (query, key)
    pair by the ORACLE's shift mask.

Frames: the kernel sees the transposed view of every grid where a shape says so; `_kgeom`, `_kview` and `_visit` speak the
kernel's frame (rows = what the kernel streams), the reference does not change.
"""
import functools
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import grl_oracle as O
from tests.test_gpu_attention_trips import _from_windows, _window_view
from tests.test_gpu_kernels import _dev, _slots, _windows

LOG2E = 1.4426950408889634
RW, RROWS = 4, 4     # waves per workgroup (2 query rows x 32 queries each), key rows per chunk

SHAPES = {
    # name: mode, (H, W), window / stripe, shift, df, nh, d, transposed
    "win": ("w", (64, 64), (32, 32), (16, 16), 1, 1, 30, False),            # interior, right, bottom and corner window
    "a2w": ("a2w", (128, 128), (64, 64), (32, 32), 2, 1, 30, False),         # anchors 32x32 -> stripe 64x64, boundary at anchor row 16
    "w2a": ("w2a", (128, 128), (64, 64), (32, 32), 2, 1, 30, False),
    "w2a_T": ("w2a", (128, 128), (64, 64), (32, 32), 2, 1, 30, True),        # the kernel's bottom border is the reference's right one
    "win_d32": ("w", (64, 64), (32, 32), (16, 16), 1, 1, 32, False),         # attn_rows_kernel<true>
    # anchor stripe of 8 rows, shift 4: the one workgroup of a stripe owns anchor rows 0 .. 7 and straddles the boundary -> no skipping
    "a2w_straddle": ("a2w", (32, 64), (16, 64), (8, 32), 2, 1, 30, False),
    # boundary at row 14, inside the chunk of key rows 12 .. 15: that chunk stays for both regions and keeps the row mask (`mixed`);
    # the workgroup of query rows 8 .. 15 straddles
    "win_unaligned": ("w", (64, 64), (32, 32), (18, 16), 1, 1, 30, False),
}
ALL = sorted(SHAPES)
SCALES = [10.0, 100.0]
# geometry of the benchmark (256x256 tile, window 32 shifted by 16, stripes 64x64 shifted by 32, anchors at /2); CPU mirror only
BENCH = {
    "bench_win": ("w", (256, 256), (32, 32), (16, 16), 1, 1, 30, False),
    "bench_a2w": ("a2w", (256, 256), (64, 64), (32, 32), 2, 1, 30, False),
    "bench_w2a": ("w2a", (256, 256), (64, 64), (32, 32), 2, 1, 30, False),
}
# chunks visited by a bottom-border workgroup / chunks of the window (4 of 8 for window and tokens -> anchors, 16 of 32 for anchors -> tokens)
EXPECT = {"win": (4, 8), "win_d32": (4, 8), "w2a": (4, 8), "w2a_T": (4, 8), "a2w": (16, 32),
          "bench_win": (4, 8), "bench_w2a": (4, 8), "bench_a2w": (16, 32)}


def _spec(shape):
    return SHAPES[shape] if shape in SHAPES else BENCH[shape]


def _grids(shape):
    mode, (H, W), win, shift, df, nh, d, tr = _spec(shape)
    awin, ashift = (win[0] // df, win[1] // df), (shift[0] // df, shift[1] // df)
    if mode == "w":
        qg = kg = (H, W, win, shift)
    elif mode == "a2w":
        qg, kg = (H // df, W // df, awin, ashift), (H, W, win, shift)
    else:
        qg, kg = (H, W, win, shift), (H // df, W // df, awin, ashift)
    return qg, kg


def _kgeom(shape):
    """Per grid (q, k) in the KERNEL's frame: dict(Himg, Wimg, wh, ww, shy, shx)."""
    tr = _spec(shape)[7]
    out = []
    for Hh, Ww, win, shift in _grids(shape):
        g = dict(Himg=Hh, Wimg=Ww, wh=win[0], ww=win[1], shy=shift[0], shx=shift[1])
        if tr:
            g = dict(Himg=Ww, Wimg=Hh, wh=win[1], ww=win[0], shy=shift[1], shx=shift[0])
        out.append(g)
    return out


# ---- the mirror of rows_geom / rows_span / the start chunk / rows_visit (csrc/attention_rows.hip) ----
def _region1d(p, n, s, sh):
    if sh == 0:
        return 0
    return 0 if p < n - s else (1 if p < n - sh else 2)


def _skippable(k, wy, hk0, rq):
    return all(_region1d(wy * k["wh"] + hk0 + r, k["Himg"], k["wh"], k["shy"]) != rq for r in range(RROWS))


def _rows_visit(q, k, wy, nwy, hqa, hqb, hk_s, masked=True):
    """(lo, hi, skip, mixed) of a workgroup with query rows hqa .. hqb and start chunk row hk_s in window row wy."""
    full = (0, k["wh"], False, False)
    if not masked or q["shy"] <= 0 or wy != nwy - 1:
        return full
    rq = _region1d(wy * q["wh"] + hqa, q["Himg"], q["wh"], q["shy"])
    if rq != _region1d(wy * q["wh"] + hqb, q["Himg"], q["wh"], q["shy"]) or _skippable(k, wy, hk_s, rq):
        return full
    lo, hi = hk_s, hk_s + RROWS
    while lo > 0 and not _skippable(k, wy, lo - RROWS, rq):
        lo -= RROWS
    while hi < k["wh"] and not _skippable(k, wy, hi, rq):
        hi += RROWS
    if lo == 0 and hi == k["wh"]:
        return full
    lab = lambda hk: _region1d(wy * k["wh"] + hk, k["Himg"], k["wh"], k["shy"])
    return lo, hi, True, lab(lo) != rq or lab(hi - 1) != rq


def _visit(shape, wy):
    """The workgroups of a window in window row `wy` (kernel frame): list of dict(rows=(hqa, hqb), segs=(sga, sgb),
    waves=[(first query row, first query column)], chunks=[(sk, chunk row)] in visiting order, nch, skip, mixed)."""
    q, k = _kgeom(shape)
    nwy = q["Himg"] // q["wh"]
    qseg, nks, nrc = q["ww"] // 32, k["ww"] // 32, k["wh"] // RROWS
    units = (q["wh"] // 2) * qseg
    upw = min(RW, units)
    out = []
    for qs in range((units + upw - 1) // upw):
        u0, u1 = qs * upw, min(qs * upw + upw, units) - 1
        hqa, hqb = 2 * (u0 // qseg), 2 * (u1 // qseg) + 1
        sga, sgb = (u0 % qseg, u1 % qseg) if u0 // qseg == u1 // qseg else (0, qseg - 1)
        rc = min(((hqa + hqb + 1) * k["wh"]) // (2 * q["wh"] * RROWS), nrc - 1)
        sc = min(((sga + sgb + 1) * k["ww"]) // (2 * q["ww"]), nks - 1)
        lo, hi, skip, mixed = _rows_visit(q, k, wy, nwy, hqa, hqb, RROWS * rc)
        c0, n = sc * nrc + rc, nks * nrc
        seq = [divmod((c0 + i) % n, nrc) for i in range(n)]
        out.append(dict(rows=(hqa, hqb), segs=(sga, sgb), waves=[(2 * (u // qseg), 32 * (u % qseg)) for u in range(u0, u1 + 1)],
                        chunks=[(s_, r_) for s_, r_ in seq if lo <= RROWS * r_ < hi], nch=n, skip=skip, mixed=mixed))
    return out


def _kview(shape, t, grid):
    """(tokens, nh, c) -> (window row, window column, nh, row, column, c) in the kernel's frame (a copy)."""
    tr, nh = _spec(shape)[7], _spec(shape)[5]
    Hh, Ww, win, _ = grid
    v = _window_view(t, grid, nh).view(Hh // win[0], Ww // win[1], nh, win[0], win[1], t.shape[-1])
    return v.permute(1, 0, 2, 4, 3, 5).contiguous() if tr else v


def _unkview(shape, v, grid):
    tr, nh = _spec(shape)[7], _spec(shape)[5]
    if tr:
        v = v.permute(1, 0, 2, 4, 3, 5)
    return _from_windows(v.reshape(-1, nh, grid[2][0] * grid[2][1], v.shape[-1]), grid, nh)


# ---- reference and launch ----
def _reference(shape, qf, kf, vf, bias):
    """float64 softmax of the fp16-rounded operands: (ref (tokens, nh, d), log2-sum-exp2 (tokens, nh))."""
    from grl_image_restoration_amd import tables

    mode, (H, W), win, shift, df, nh, d, tr = _spec(shape)
    qg, kg = _grids(shape)
    ones, one31 = d < 32, d <= 30
    qs, ks, vs = _slots(qf, d), _slots(kf, d, one31=one31), _slots(vf, d, ones)
    rows = (qg[2][0] + kg[2][0] - 1) * (qg[2][1] + kg[2][1] - 1)
    tab_k = tables.kernel_table(bias)
    tab = torch.flip(tab_k[:, : tab_k.shape[1] - (-rows) % 4], dims=(1,))
    if mode == "w":
        index, mask = O.rel_index(win), O.shift_mask((H, W), win, shift, mode="w")
    else:
        index, mask = O.rel_index(win, df, mode == "w2a"), O.shift_mask((H, W), win, shift, df, mode)
    qw, kw, vw = (_windows(t, 1, g_[0], g_[1], g_[2], g_[3], nh) for t, g_ in ((qs, qg), (ks, kg), (vs, kg)))
    s = qw[..., :d].double() @ kw[..., :d].double().transpose(-1, -2)
    s += tab.double()[:, index.reshape(-1)].view(nh, *index.shape).unsqueeze(0)
    s += (mask.double() * LOG2E).unsqueeze(1)
    smax = s.max(dim=-1, keepdim=True).values
    p = torch.exp2(s.sub_(smax))
    den = p.sum(-1)
    ref = _from_windows((p @ vw.double()) / den.unsqueeze(-1), qg, nh)[..., :d]
    lse_ref = _from_windows((torch.log2(den) + smax[..., 0]).unsqueeze(-1), qg, nh)[..., 0]
    return ref, lse_ref


def _launch(shape, qf, kf, vf, bias, bound):
    """qf (already scaled, log2 domain) / kf / vf: (tokens, nh, d) float; bias (rows, nh), natural-log domain; bound: per-head bound
    of |q.k| / log2e.  Launches the lazy-offset path: (output (tokens, nh, d) float, log2-sum-exp2 (tokens, nh) float), on the CPU."""
    from grl_image_restoration_amd import ops, tables

    mode, (H, W), win, shift, df, nh, d, tr = _spec(shape)
    qg, kg = _grids(shape)
    ones, one31 = d < 32, d <= 30
    qs, ks, vs = _slots(qf, d), _slots(kf, d, one31=one31), _slots(vf, d, ones)
    rows = (qg[2][0] + kg[2][0] - 1) * (qg[2][1] + kg[2][1] - 1)
    assert bias.shape == (rows, nh)
    tab_k = tables.kernel_table(ops.transpose_table(bias, qg[2], kg[2]) if tr else bias)
    dev = _dev()
    TG = ops.TokenGrid

    def lay(t):   # head planes [nh, tokens, 32]
        return t.view(t.shape[0], nh, 32).permute(1, 0, 2).contiguous().to(dev)

    qd, kd, vd = lay(qs), lay(ks), lay(vs)
    out = lay(torch.zeros(qg[0] * qg[1], nh * 32, dtype=torch.float16))
    lse = torch.zeros(nh, qg[0] * qg[1], dtype=torch.float32, device=dev)
    grids = tuple(TG(t, 0, g_[0], g_[1], g_[2][0], g_[2][1], g_[3][0], g_[3][1]) for t, g_ in ((qd, qg), (kd, kg), (vd, kg), (out, qg)))
    if tr:
        grids = tuple(g_.T() for g_ in grids)
    sw = (lambda t: (t[1], t[0])) if tr else (lambda t: t)
    assert ops.attention_rows_ok(sw(qg[2]), sw(kg[2]), sw(qg[3]), sw(kg[3]), True, d), "the case must reach the row-streaming kernel"
    tab_ceil = tables.kernel_table(bias)
    ops.attention(*grids, B=1, nh=nh, table=tab_k.to(dev), masked=True, ones_col=d if ones else -1, head_dim=d, k_one31=one31,
                  lazy_floor=tables.lazy_floor(bound).to(dev), lse=lse, lazy_ceil=tables.lazy_ceil(bound, tab_ceil).to(dev))
    torch.cuda.synchronize()
    return out.permute(1, 0, 2).float().cpu()[..., :d], lse.t().cpu()


def _compare(shape, got, lse, ref, lse_ref, hi):
    assert torch.isfinite(got).all(), "non-finite output: the poison path fired"
    err = (got.double() - ref).abs().max().item()
    e2 = (lse.double() - lse_ref).abs().max().item()
    print(f"{shape}: max|err| = {err:.3e} (ref max {ref.abs().max().item():.2f}), lse {e2:.3e}")
    assert err < 1.5e-3 * (3.0 if hi else 1.0) * max(1.0, ref.abs().max().item()), err
    assert e2 < 2e-3, e2


@functools.lru_cache(maxsize=None)
def _random_operands(shape, scale):
    """Unit q / k directions, v and a bias in 0 .. 16 as in _attention_case; every head at logit scale `scale`."""
    nh, d = _spec(shape)[5], _spec(shape)[6]
    qg, kg = _grids(shape)
    g = torch.Generator().manual_seed(23 + ALL.index(shape))
    qn = F.normalize(torch.randn(qg[0] * qg[1], nh, d, generator=g), dim=-1)
    kn = F.normalize(torch.randn(kg[0] * kg[1], nh, d, generator=g), dim=-1)
    vf = torch.randn(kg[0] * kg[1], nh, d, generator=g)
    rows = (qg[2][0] + kg[2][0] - 1) * (qg[2][1] + kg[2][1] - 1)
    bias = torch.rand(rows, nh, generator=g) * 16
    return torch.full((nh,), scale), qn, kn, vf, bias


@functools.lru_cache(maxsize=None)
def _random_reference(shape, scale):
    sc, qn, kn, vf, bias = _random_operands(shape, scale)
    return _reference(shape, qn * (sc * LOG2E).view(1, -1, 1), kn, vf, bias)


# ---- the mirror, on the CPU ----
@pytest.mark.parametrize("shape", ALL + sorted(BENCH))
def test_mirror_chunk_counts(shape):
    """Bottom-border workgroups visit 4 of 8 chunks (window, tokens -> anchors) and 16 of 32 (anchors -> tokens) and run without
    the row mask; every other workgroup visits all chunks.  The straddling shape skips nothing; the unaligned one keeps the row mask."""
    q, k = _kgeom(shape)
    nwy = q["Himg"] // q["wh"]
    for wy in range(nwy):
        for wg in _visit(shape, wy):
            assert len(set(wg["chunks"])) == len(wg["chunks"])
            if wy < nwy - 1 or shape == "a2w_straddle":
                assert not wg["skip"] and len(wg["chunks"]) == wg["nch"], (shape, wy, wg)
            elif shape == "win_unaligned":
                want = {(0, 7): 4, (8, 15): 8}.get(wg["rows"], 5)       # rows 0 .. 13 | straddling | rows 14 .. 31 (chunk rows 12 .. 28)
                assert len(wg["chunks"]) == want and wg["mixed"] == wg["skip"], (shape, wy, wg)
            else:
                assert wg["skip"] and not wg["mixed"] and (len(wg["chunks"]), wg["nch"]) == EXPECT[shape], (shape, wy, wg)
    # the order is the old one minus the chunks stepped over, from the same start chunk
    for a, b in zip(_visit(shape, 0), _visit(shape, nwy - 1)):
        assert b["chunks"] == [c for c in a["chunks"] if c in set(b["chunks"])] and b["chunks"][0] == a["chunks"][0]


@pytest.mark.parametrize("shape", [s for s in ALL if not SHAPES[s][7]])
def test_mirror_skips_only_what_the_oracle_masks(shape):
    """Every chunk a workgroup steps over is masked by the oracle's shift mask for every (query of the workgroup, key of the chunk)
    pair in every bottom-border window; and a workgroup that runs the unmasked statement sees no masked pair in what it visits."""
    mode, (H, W), win, shift, df, nh, d, tr = SHAPES[shape]
    qg, kg = _grids(shape)
    q, k = _kgeom(shape)
    mask = O.shift_mask((H, W), win, shift, mode="w") if mode == "w" else O.shift_mask((H, W), win, shift, df, mode)
    nwy, nwx = q["Himg"] // q["wh"], q["Wimg"] // q["ww"]
    m = (mask != 0).view(nwy, nwx, q["wh"], q["ww"], k["wh"], k["ww"])
    nrc = k["wh"] // RROWS
    skipped = 0
    for wx in range(nwx):
        for wg in _visit(shape, nwy - 1):
            hqa, hqb = wg["rows"]
            for c in range(wg["nch"]):
                sk, rc = divmod(c, nrc)
                blk = m[nwy - 1, wx, hqa:hqb + 1, 32 * wg["segs"][0]:32 * wg["segs"][1] + 32, RROWS * rc:RROWS * rc + RROWS, 32 * sk:32 * sk + 32]
                if (sk, rc) not in wg["chunks"]:
                    assert blk.all(), (shape, wx, wg["rows"], sk, rc)
                    skipped += 1
                elif wg["skip"] and not wg["mixed"] and wx < nwx - 1:
                    assert not blk.any(), (shape, wx, wg["rows"], sk, rc)
    assert (skipped > 0) == (shape != "a2w_straddle")


def test_trip_model_follows_the_same_order():
    """tools/attn_trip_model.py replays the kernel's visiting order: its visit_order agrees with this file's mirror."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "attn_trip_model.py")
    spec = importlib.util.spec_from_file_location("attn_trip_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for shape in [s for s in ALL if not SHAPES[s][7]] + sorted(BENCH):
        q, k = _kgeom(shape)
        nwy = q["Himg"] // q["wh"]
        for wy in (0, nwy - 1):
            got = mod.visit_order((q["wh"], q["ww"]), (k["wh"], k["ww"]), "own", bottom=wy == nwy - 1, qshy=q["shy"], kshy=k["shy"])
            want = _visit(shape, wy)
            assert [c for _, c in got] == [w["chunks"] for w in want] and [u for u, _ in got] == [w["waves"] for w in want], (shape, wy)


# ---- the float64 reference ----
@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", ALL)
def test_against_float64(shape, scale):
    sc, qn, kn, vf, bias = _random_operands(shape, scale)
    ref, lse_ref = _random_reference(shape, scale)
    got, lse = _launch(shape, qn * (sc * LOG2E).view(1, -1, 1), kn, vf, bias, sc)
    _compare(shape, got, lse, ref, lse_ref, hi=scale > 50)


# ---- aimed cases: the bottom-border (and every other) window of "win", scale 100 ----
@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("shape", ["win", "win_d32", "win_unaligned"])
def test_peak_in_visited_chunk(shape, where):
    """Per window, workgroup and wave a key of the aimed chunk copies the direction of one of the wave's queries (cos = 1): in the
    chunk the workgroup visits first (the prime pass sees it) and in the one it visits LAST -- in a bottom-border window that is the
    chunk before the start chunk inside the restricted range, reached after the wrap; every offset set before it is too low."""
    nh = SHAPES[shape][5]
    qg, kg = _grids(shape)
    q, _ = _kgeom(shape)
    sc, qn, kn, vf, bias = _random_operands(shape, 100.0)
    qv, kv = _kview(shape, qn, qg), _kview(shape, kn, kg)
    for wy in range(q["Himg"] // q["wh"]):
        for qs, wg in enumerate(_visit(shape, wy)):
            sk, rc = wg["chunks"][0 if where == "first" else -1]
            for w, (r0, c0) in enumerate(wg["waves"]):
                hq, wq = r0 + (w & 1), c0 + (5 + 7 * w + 3 * qs) % 32
                hk, wk = RROWS * rc + (w + qs) % RROWS, 32 * sk + (11 * qs + 3 * w) % 32
                kv[wy, :, :, hk, wk] = qv[wy, :, :, hq, wq]
    kn2 = _unkview(shape, kv, kg)
    qf = qn * (sc * LOG2E).view(1, nh, 1)
    got, lse = _launch(shape, qf, kn2, vf, bias, sc)
    _compare(shape, got, lse, *_reference(shape, qf, kn2, vf, bias), hi=True)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["win", "win_d32", "win_unaligned"])
def test_staircase_every_visited_chunk_trips(shape):
    """q.k = 20 binades x (place of the chunk in the workgroup's visiting order), exactly (query direction 16 x e_workgroup, key
    component `workgroup` = M / 16, multiples of 1.25: exact in fp16); chunks that are stepped over hold 0.  Every visited chunk's
    maximum lies more than the full headroom above the previous one's (tests/test_gpu_attention_trips.py)."""
    nh, d = SHAPES[shape][5], SHAPES[shape][6]
    qg, kg = _grids(shape)
    q, k = _kgeom(shape)
    _, _, _, vf, bias = _random_operands(shape, 100.0)
    nwy, nrc = q["Himg"] // q["wh"], k["wh"] // RROWS
    r = len(_visit(shape, 0))
    qfac = 16.0 * torch.eye(r)
    wgmap = torch.empty(q["wh"], q["ww"], dtype=torch.long)
    for qs, wg in enumerate(_visit(shape, 0)):
        for r0, c0 in wg["waves"]:
            wgmap[r0:r0 + 2, c0:c0 + 32] = qs
    qv = torch.zeros(*_kview(shape, torch.zeros(qg[0] * qg[1], nh, 1), qg).shape[:-1], d)
    kv = torch.zeros(*_kview(shape, torch.zeros(kg[0] * kg[1], nh, 1), kg).shape[:-1], d)
    qv[..., :r] = qfac[wgmap]
    cidx = (torch.arange(k["ww"]) // 32).view(1, -1) * nrc + (torch.arange(k["wh"]) // RROWS).view(-1, 1)
    top = 0.0
    for wy in range(nwy):
        M = torch.zeros(r, (k["ww"] // 32) * nrc)
        for qs, wg in enumerate(_visit(shape, wy)):
            for i, (sk, rc) in enumerate(wg["chunks"]):
                M[qs, sk * nrc + rc] = 20.0 * i
        kfac = M.t() / 16.0
        assert (qfac.half().double() @ kfac.half().double().t() == M.double()).all()
        kv[wy, ..., :r] = kfac[cidx]
        top = max(top, float(M.max()))
    qf, kf = _unkview(shape, qv, qg), _unkview(shape, kv, kg)
    bound = torch.full((nh,), top / LOG2E + 1.0)
    got, lse = _launch(shape, qf, kf, vf, bias / 8.0, bound)
    _compare(shape, got, lse, *_reference(shape, qf, kf, vf, bias / 8.0), hi=True)


# ---- invariance ----
@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", ALL)
def test_other_row_region_does_not_reach_the_output(shape, scale):
    """Bottom-border and corner windows (stripes), for the queries of row region 1 and of row region 2 in turn: the K and V rows
    of the OTHER row region hold large finite values (K: the direction of one of those queries, cos = 1; V: +-6e4) in run A and
    zeros in run B.  Outputs and log-sum-exp of those queries are equal bit for bit."""
    nh = SHAPES[shape][5]
    qg, kg = _grids(shape)
    q, k = _kgeom(shape)
    sc, qn, kn, vf, bias = _random_operands(shape, scale)
    qf = qn * (sc * LOG2E).view(1, nh, 1)
    wy = q["Himg"] // q["wh"] - 1
    qsplit, ksplit = q["wh"] - q["shy"], k["wh"] - k["shy"]       # first row of region 2 inside a bottom-border window
    sign = 1.0 - 2.0 * ((torch.arange(k["wh"]).view(-1, 1) + torch.arange(k["ww"]).view(1, -1)) % 2)
    for region in (1, 2):
        qrows = slice(0, qsplit) if region == 1 else slice(qsplit, q["wh"])
        krows = slice(ksplit, k["wh"]) if region == 1 else slice(0, ksplit)     # the other region's key rows
        runs = []
        for big in (True, False):
            kv, vv = _kview(shape, kn, kg), _kview(shape, vf, kg)
            if big:
                qdir = _kview(shape, qn, qg)[wy, :, :, qrows.start, :, :]                       # (window column, nh, q columns, d)
                kv[wy, :, :, krows] = qdir[:, :, torch.arange(k["ww"]) % q["ww"]].unsqueeze(2)
                vv[wy, :, :, krows] = (6.0e4 * sign[krows]).view(1, 1, -1, k["ww"], 1)
            else:
                kv[wy, :, :, krows] = 0.0
                vv[wy, :, :, krows] = 0.0
            got, lse = _launch(shape, qf, _unkview(shape, kv, kg), _unkview(shape, vv, kg), bias, sc)
            assert torch.isfinite(got).all()
            runs.append((_kview(shape, got, qg)[wy, :, :, qrows], _kview(shape, lse.unsqueeze(-1), qg)[wy, :, :, qrows]))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (shape, scale, region)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in ALL if s != "a2w_straddle"])
def test_stepped_over_rows_are_not_read(shape):
    """That the rule is in force on the GPU, not only in the mirror: V holds NaN in the key rows of the chunks that the workgroups of
    one row region step over (a non-finite K or V there no longer reaches the output; a kernel that still
    visits those chunks multiplies the NaN by its zero weights).  The outputs of those workgroups' queries are finite and equal
    to the run with zeros in the same rows."""
    nh = SHAPES[shape][5]
    qg, kg = _grids(shape)
    q, k = _kgeom(shape)
    sc, qn, kn, vf, bias = _random_operands(shape, 100.0)
    qf = qn * (sc * LOG2E).view(1, nh, 1)
    wy = q["Himg"] // q["wh"] - 1
    qsplit = q["wh"] - q["shy"]
    for region in (1, 2):
        wgs = [w for w in _visit(shape, wy) if w["skip"] and (w["rows"][1] < qsplit if region == 1 else w["rows"][0] >= qsplit)]
        assert wgs
        gone = set(range(k["wh"] // RROWS)).difference(*[{rc for _, rc in w["chunks"]} for w in wgs])   # stepped over by all of them
        assert gone
        rows = torch.tensor([RROWS * rc + r for rc in sorted(gone) for r in range(RROWS)])
        qrows = torch.tensor([h for w in wgs for h in range(w["rows"][0], w["rows"][1] + 1)])
        runs = []
        for fill in (float("nan"), 0.0):
            vv = _kview(shape, vf, kg)
            vv[wy, :, :, rows] = fill
            got, lse = _launch(shape, qf, kn, _unkview(shape, vv, kg), bias, sc)
            runs.append((_kview(shape, got, qg)[wy][:, :, qrows], _kview(shape, lse.unsqueeze(-1), qg)[wy][:, :, qrows]))
        assert torch.isfinite(runs[0][0]).all(), (shape, region)
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), (shape, region)
