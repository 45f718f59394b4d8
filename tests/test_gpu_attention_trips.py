"""Row-streaming attention kernel at the places where its lazy softmax offset moves (csrc/attention_rows.hip): peaks in
the chunk a workgroup visits first / last / for one query of a wave, a staircase that trips in every chunk, weights that
are fp16 sub-normals, and the low-scale regime that never trips.

Every case is checked against the float64 softmax of the same fp16-rounded operands, built as in
tests/test_gpu_kernels.py::_attention_case, with that function's tolerances: 1.5e-3 (x 3 at high scale) x max(1, |ref|max)
on the output and 2e-3 on the log2-sum-exp2.

`_visit_order` mirrors the kernel's work decomposition (rows_geom / rows_span / the start chunk) so that the cases can
aim at a chunk by its place in a workgroup's visiting order.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import grl_oracle as O
from tests.test_gpu_kernels import _dev, _slots, _windows

LOG2E = 1.4426950408889634
RW, RROWS = 4, 4     # waves per workgroup (2 query rows x 32 queries each), key rows per chunk

SHAPES = {
    # name: mode, (H, W), window / stripe, shift, df, nh, d, transposed
    "win32": ("w", (32, 32), (32, 32), (0, 0), 1, 2, 30, False),
    "win32_border": ("w", (64, 64), (32, 32), (16, 16), 1, 1, 30, False),       # shifted: the BORDER instance
    "a2w": ("a2w", (64, 64), (64, 64), (0, 0), 2, 2, 30, False),                 # anchors 32x32 -> stripe 64x64
    "w2a": ("w2a", (64, 64), (64, 64), (0, 0), 2, 1, 30, False),                 # stripe 64x64 -> anchors 32x32
    "w2a_T": ("w2a", (64, 64), (64, 64), (0, 0), 2, 1, 30, True),                # the same on the transposed view
    "win32_d32": ("w", (32, 32), (32, 32), (0, 0), 1, 3, 32, False),             # head_dim 32: attn_rows_kernel<true>
}
ALL = sorted(SHAPES)


def _grids(shape):
    mode, (H, W), win, shift, df, nh, d, tr = SHAPES[shape]
    awin, ashift = (win[0] // df, win[1] // df), (shift[0] // df, shift[1] // df)
    if mode == "w":
        qg = kg = (H, W, win, shift)
    elif mode == "a2w":
        qg, kg = (H // df, W // df, awin, ashift), (H, W, win, shift)
    else:
        qg, kg = (H, W, win, shift), (H // df, W // df, awin, ashift)
    return qg, kg


def _visit_order(shape):
    """(wg[hq, wq], order[wg] = list of (sk, chunk row), units[wg] = list of (first row, first column) of its waves) in the
    KERNEL's frame (the transposed view swaps rows and columns)."""
    qg, kg = _grids(shape)
    tr = SHAPES[shape][7]
    (qwh, qww), (kwh, kww) = (qg[2][::-1], kg[2][::-1]) if tr else (qg[2], kg[2])
    qseg, nks, nrc = qww // 32, kww // 32, kwh // RROWS
    units = (qwh // 2) * qseg
    upw = min(RW, units)
    wg = torch.empty(qwh, qww, dtype=torch.long)
    order, waves = [], []
    for qs in range((units + upw - 1) // upw):
        u0, u1 = qs * upw, min(qs * upw + upw, units) - 1
        hqa, hqb = 2 * (u0 // qseg), 2 * (u1 // qseg) + 1
        sga, sgb = (u0 % qseg, u1 % qseg) if u0 // qseg == u1 // qseg else (0, qseg - 1)
        rc = min(((hqa + hqb + 1) * kwh) // (2 * qwh * RROWS), nrc - 1)
        sc = min(((sga + sgb + 1) * kww) // (2 * qww), nks - 1)
        c0 = sc * nrc + rc
        order.append([divmod((c0 + i) % (nks * nrc), nrc) for i in range(nks * nrc)])
        for u in range(u0, u1 + 1):
            wg[2 * (u // qseg): 2 * (u // qseg) + 2, 32 * (u % qseg): 32 * (u % qseg) + 32] = qs
        waves.append([(2 * (u // qseg), 32 * (u % qseg)) for u in range(u0, u1 + 1)])
    return wg, order, waves


def _to_ref(shape, t):
    """(nW, nh, wh_kernel, ww_kernel, c) in the kernel's frame -> (nW, nh, N, c) in the reference's window order."""
    if SHAPES[shape][7]:
        t = t.transpose(2, 3)
    return t.reshape(t.shape[0], t.shape[1], -1, t.shape[-1])


def _from_windows(t, grid, nh):
    """(nW, nh, N, c) window order -> (tokens, nh, c): the inverse of test_gpu_kernels._windows (B = 1)."""
    Hh, Ww, win, shift = grid
    x = t.permute(0, 2, 1, 3).reshape(-1, win[0], win[1], nh * t.shape[-1])
    x = O.unpartition(x, win, (Hh, Ww))
    if shift[0] or shift[1]:
        x = torch.roll(x, shifts=(shift[0], shift[1]), dims=(1, 2))
    return x.reshape(Hh * Ww, nh, t.shape[-1])


def _check(shape, qf, kf, vf, bias, bound, hi):
    """qf (already scaled, log2 domain) / kf / vf: (tokens, nh, d) float; bias: (rows, nh), natural-log domain; bound: per-head
    bound of |q.k| / log2e (what the lazy floor and ceiling are derived from).  Launches the lazy-offset path, checks output and lse."""
    from grl_image_restoration_amd import ops, tables

    mode, (H, W), win, shift, df, nh, d, tr = SHAPES[shape]
    qg, kg = _grids(shape)
    B = 1
    ones, one31 = d < 32, d <= 30
    qs, ks, vs = _slots(qf, d), _slots(kf, d, one31=one31), _slots(vf, d, ones)
    rows = (qg[2][0] + kg[2][0] - 1) * (qg[2][1] + kg[2][1] - 1)
    assert bias.shape == (rows, nh)
    tab_k = tables.kernel_table(bias)
    tab = torch.flip(tab_k[:, : tab_k.shape[1] - (-rows) % 4], dims=(1,))
    if tr:
        tab_k = tables.kernel_table(ops.transpose_table(bias, qg[2], kg[2]))
    masked = shift[0] > 0 or shift[1] > 0
    if mode == "w":
        index = O.rel_index(win)
        mask = O.shift_mask((H, W), win, shift, mode="w") if masked else None
    else:
        index = O.rel_index(win, df, mode == "w2a")
        mask = O.shift_mask((H, W), win, shift, df, mode) if masked else None
    qw, kw, vw = (_windows(t, B, g_[0], g_[1], g_[2], g_[3], nh) for t, g_ in ((qs, qg), (ks, kg), (vs, kg)))
    s = qw[..., :d].double() @ kw[..., :d].double().transpose(-1, -2)
    s = s + tab.double()[:, index.reshape(-1)].view(nh, *index.shape).unsqueeze(0)
    if mask is not None:
        s = (s.view(B, mask.shape[0], nh, *index.shape) + (mask.double() * LOG2E).unsqueeze(1).unsqueeze(0)).view(-1, nh, *index.shape)
    smax = s.max(dim=-1, keepdim=True).values
    p = torch.exp2(s - smax)
    lse_ref = torch.log2(p.sum(-1)) + smax[..., 0]
    ref = (p @ vw.double()) / p.sum(-1, keepdim=True)
    ref = _from_windows(ref, qg, nh)[..., :d]
    lse_ref = _from_windows(lse_ref.unsqueeze(-1), qg, nh)[..., 0]

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
    ops.attention(*grids, B=B, nh=nh, table=tab_k.to(dev), masked=masked, ones_col=d if ones else -1, head_dim=d, k_one31=one31,
                  lazy_floor=tables.lazy_floor(bound).to(dev), lse=lse, lazy_ceil=tables.lazy_ceil(bound, tab_k).to(dev))
    torch.cuda.synchronize()
    got = out.permute(1, 0, 2).float().cpu()[..., :d]
    assert torch.isfinite(got).all(), "non-finite output: the poison path fired"
    err = (got.double() - ref).abs().max().item()
    e2 = (lse.t().cpu().double() - lse_ref).abs().max().item()
    print(f"{shape}: max|err| = {err:.3e} (ref max {ref.abs().max().item():.2f}), lse {e2:.3e}")
    assert err < 1.5e-3 * (3.0 if hi else 1.0) * max(1.0, ref.abs().max().item()), err
    assert e2 < 2e-3, e2


@functools.lru_cache(maxsize=None)
def _random_operands(shape, scale_lo, scale_hi):
    """Unit q / k directions, v and a bias in 0 .. 16 as in _attention_case; scale per head uniform in [lo, hi]."""
    mode, _, _, _, _, nh, d, _ = SHAPES[shape]
    qg, kg = _grids(shape)
    g = torch.Generator().manual_seed(11 + ALL.index(shape))
    scale = scale_lo + (scale_hi - scale_lo) * torch.rand(nh, generator=g)
    qn = F.normalize(torch.randn(qg[0] * qg[1], nh, d, generator=g), dim=-1)
    kn = F.normalize(torch.randn(kg[0] * kg[1], nh, d, generator=g), dim=-1)
    vf = torch.randn(kg[0] * kg[1], nh, d, generator=g)
    rows = (qg[2][0] + kg[2][0] - 1) * (qg[2][1] + kg[2][1] - 1)
    bias = torch.rand(rows, nh, generator=g) * 16
    return scale, qn, kn, vf, bias


def _window_view(t, grid, nh):
    """(tokens, nh, c) -> (nW, nh, wh, ww, c) window view (a copy) in the reference's frame."""
    Hh, Ww, win, shift = grid
    c = t.shape[-1]
    x = t.reshape(1, Hh, Ww, nh * c)
    if shift[0] or shift[1]:
        x = torch.roll(x, shifts=(-shift[0], -shift[1]), dims=(1, 2))
    x = O.partition(x, win).reshape(-1, win[0], win[1], nh, c)
    return x.permute(0, 3, 1, 2, 4).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "last", "one_query"])
@pytest.mark.parametrize("shape", ALL)
def test_peak_placement(shape, where):
    """Scale 100; per workgroup and wave, a key of the aimed chunk copies the direction of one of the wave's queries (cos = 1, 58
    binades above what random directions reach): in the chunk the workgroup visits first (the prime pass sees it), in the one it
    visits last (every offset set before is too low), and -- `one_query` -- in a middle chunk for the workgroup's first wave only."""
    mode, _, _, _, _, nh, d, tr = SHAPES[shape]
    qg, kg = _grids(shape)
    scale, qn, kn, vf, bias = _random_operands(shape, 100.0, 100.0)
    wg, order, waves = _visit_order(shape)
    qv = _window_view(qn, qg, nh)                 # (nW, nh, wh, ww, d), reference frame
    kv = _window_view(kn, kg, nh)
    if tr:
        qv, kv = qv.transpose(2, 3), kv.transpose(2, 3)   # kernel frame (views of the copies)
    for qs, visits in enumerate(order):
        sk, rc = {"first": visits[0], "last": visits[-1], "one_query": visits[len(visits) // 2]}[where]
        for w, (r0, c0) in enumerate(waves[qs][:1] if where == "one_query" else waves[qs]):
            hq, wq = r0 + (w & 1), c0 + (5 + 7 * w + 3 * qs) % 32                          # one query of the wave (2 rows x 32 columns)
            hk, wk = RROWS * rc + (w + qs) % RROWS, 32 * sk + (11 * qs + 3 * w) % 32      # distinct keys for distinct (qs, w) of a chunk
            kv[:, :, hk, wk] = qv[:, :, hq, wq]
    kn2 = _from_windows(_to_ref(shape, kv), kg, nh)
    _check(shape, qn * (scale * LOG2E).view(1, nh, 1), kn2, vf, bias, scale, hi=True)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALL)
def test_staircase_every_chunk_trips(shape):
    """q.k = M[workgroup, chunk] = 20 binades x (place of the chunk in the workgroup's visiting order), exactly: query direction
    16 x e_workgroup, key component `workgroup` = M / 16 (multiples of 1.25 up to 38.75: exact in fp16).  Every chunk's maximum lies
    more than the full headroom (at most 17 binades between the resting level and the trip, + the bias spread) above the previous
    one's, so every wave of an unmasked window trips in every chunk (in a shifted border window the region mask, -144, hides part
    of the stairs from a query).  The bias spreads the weights inside the last chunk."""
    mode, _, _, _, _, nh, d, tr = SHAPES[shape]
    qg, kg = _grids(shape)
    _, _, _, vf, bias = _random_operands(shape, 100.0, 100.0)
    wg, order, _ = _visit_order(shape)
    nch = len(order[0])
    nrc = nch // (max(s for s, _ in order[0]) + 1)
    r = len(order)
    assert r <= 28 and nch <= 32
    M = torch.zeros(r, nch)
    for qs, visits in enumerate(order):
        for i, (sk, rc) in enumerate(visits):
            M[qs, sk * nrc + rc] = 20.0 * i
    qfac, kfac = 16.0 * torch.eye(r), M.t() / 16.0                                          # M = qfac @ kfac^T
    Mr = qfac.half().double() @ kfac.half().double().t()
    assert (Mr == M.double()).all()
    qv = torch.zeros(*_window_view(torch.zeros(qg[0] * qg[1], nh, 1), qg, nh).shape[:-1], d)
    kv = torch.zeros(*_window_view(torch.zeros(kg[0] * kg[1], nh, 1), kg, nh).shape[:-1], d)
    if tr:
        qv, kv = qv.transpose(2, 3), kv.transpose(2, 3)
    qv[..., :r] = qfac[wg]                                        # (wh, ww, r) broadcast over windows and heads
    kwh, kww = kv.shape[2], kv.shape[3]
    cidx = (torch.arange(kww) // 32).view(1, -1) * nrc + (torch.arange(kwh) // RROWS).view(-1, 1)
    kv[..., :r] = kfac[cidx]
    qf, kf = _from_windows(_to_ref(shape, qv), qg, nh), _from_windows(_to_ref(shape, kv), kg, nh)
    # (_attention_case's bias, 0 .. 16 nats = 23 binades, would level the steps: an eighth of it here, 20 - 2.9 > 17)
    bound = torch.full((nh,), float(Mr.abs().max()) / LOG2E + 1.0)
    _check(shape, qf, kf, vf, bias / 8.0, bound, hi=True)


def _denormal_case(shape):
    mode, _, win, _, _, nh, d, _ = SHAPES[shape]
    qg, kg = _grids(shape)
    g = torch.Generator().manual_seed(5)
    vf = torch.randn(kg[0] * kg[1], nh, d, generator=g)
    rows = (2 * win[0] - 1) * (2 * win[1] - 1)
    bias = torch.zeros(rows, nh)
    bias[int(O.rel_index(win)[0, 0])] = torch.linspace(15.2, 15.8, nh) / LOG2E          # relative position (0, 0): each query's own key
    return vf, bias


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["win32", "win32_d32"])
def test_denormal_weights(shape):
    """q = 0: the logits are the bias table, 0 everywhere except 15.2 .. 15.8 (log2) at relative position (0, 0).  The 1023 other
    keys of a query carry 1023 x 2^-15.5 = 2 % of its softmax mass, 15 - 16 binades under its own key: wherever the own key rests
    under 2^2 they are fp16 sub-normals, and a kernel that flushes them is off by 2 % of |v| -- ten times the tolerance."""
    mode, _, _, _, _, nh, d, _ = SHAPES[shape]
    qg, kg = _grids(shape)
    vf, bias = _denormal_case(shape)
    z = torch.zeros(qg[0] * qg[1], nh, d)
    _check(shape, z, torch.zeros(kg[0] * kg[1], nh, d), vf, bias, torch.full((nh,), 100.0), hi=True)


def test_denormal_case_separates_flushing_from_rounding():
    """CPU: the denormal case with the weights rounded to fp16 relative to an offset that rests the own key in (2^-3, 2^-2] (the
    kernel's resting level) and one binade lower (the lowest it lets a row maximum rest).  With sub-normals kept the float64 result stays well inside the tolerance; with
    them flushed it misses it by an order of magnitude -- so the GPU test above decides which of the two the hardware does."""
    nh, d = 2, 30
    vf, bias = _denormal_case("win32")
    own = bias.max(dim=0).values * LOG2E                           # (nh,) log2 logit of the own key; the others are 0
    v = vf.half().double().permute(1, 0, 2)                        # (nh, N, d)
    n = v.shape[1]
    for rest in (-2.0, -3.0):
        m = torch.ceil(own) - rest
        w_own, w_oth = torch.exp2(own - m).half(), torch.exp2(-m).half()          # .half() keeps sub-normals
        assert (w_oth.float() < 2.0 ** -14).all() and (w_oth > 0).all()
        for flush in (False, True):
            wo = torch.zeros_like(w_oth) if flush else w_oth
            den = w_own.double() + (n - 1) * wo.double()
            tot = v.sum(1)                                         # (nh, d)
            got = (w_own.double().view(nh, 1, 1) * v + wo.double().view(nh, 1, 1) * (tot.unsqueeze(1) - v)) / den.view(nh, 1, 1)
            e_own, e_oth = torch.exp2(own).double(), 1.0
            ref = (e_own.view(nh, 1, 1) * v + (tot.unsqueeze(1) - v)) / (e_own + (n - 1)).view(nh, 1, 1)
            err = (got - ref).abs().max().item()
            lse_err = (torch.log2(den) + m - torch.log2(e_own + (n - 1))).abs().max().item()
            tol = 1.5e-3 * 3.0 * max(1.0, ref.abs().max().item())
            print(f"rest {rest} flush {flush}: err {err:.3e} (tol {tol:.3e}) lse {lse_err:.3e}")
            if flush:
                assert err > 5 * tol and lse_err > 5 * 2e-3
            else:
                assert err < 0.5 * tol and lse_err < 0.5 * 2e-3


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["win32_border", "w2a"])
def test_random_init_regime(shape):
    """Scales 4 .. 16: the offsets reach the test-free level with the prime pass (`nochk` from the first chunk on) and nothing trips."""
    mode, _, _, _, _, nh, d, _ = SHAPES[shape]
    scale, qn, kn, vf, bias = _random_operands(shape, 4.0, 16.0)
    _check(shape, qn * (scale * LOG2E).view(1, nh, 1), kn, vf, bias, scale, hi=False)
