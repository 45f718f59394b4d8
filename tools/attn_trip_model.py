#!/usr/bin/env python3
"""CPU model of the lazy softmax offset of csrc/attention_rows.hip: how often does a wave leave the key-row statement
("trip") at a given resting level and chunk order, and what do fp16 weights relative to the final offsets cost?

The bench's own network (baseline_config(3), constructor seed 0, checkpoint-like logit scales from seed 7 as bench.py
draws them, uniform-random pixels, one tile) runs through the torch oracle; every attention call of its blocks is cut into
the kernel's waves (2 query rows x 32 queries) and chunks (4 key rows x 32 keys) and replayed:
  * the first chunk a wave visits primes the offsets: exact maxima of the chunk, offset = ceil(max) - REST;
  * in later chunks a key row whose logit - offset reaches 14 for any of the wave's 64 queries trips the wave: exact maxima
    of that row and the rest of the chunk, offsets of the queries raised to ceil(max) - REST (never lowered);
  * offsets within EXTRA under msafe = ceil(lazy_ceil - 13.5) go straight there; once every query of the wave is at
    msafe the wave stops testing (no trips any more);
  * round 8: in a bottom-border window (stripe) of a shifted block a workgroup whose query rows carry one row label steps over
    the chunks of the other row region (rows_visit of the kernel); the order is the same, minus those chunks, and the share of
    chunks a wave visits is printed per launch.  Against offsets set from visible keys such a chunk never trips (144 binades under);
    it could trip in a CORNER window, for a wave with queries whose start chunk lies wholly in the other column region: their offsets
    sit at the masked level until the first visible chunk arrives.  Those trips go with the chunks (anchors->tokens at side 64, where
    the only stripe is a corner stripe: 3.01 -> 2.69 trips per wave); the final offsets are the same.
Not modelled: transposed grid views (the bench geometry has none) and the 2^-12 by which the packed fp16 weight
reaches 2^14 before the logit reaches 14.

    python tools/attn_trip_model.py --side 64 --rest 4 0 -2 --order top own
prints, for every (rest, order) pair asked for (one pass of the network serves them all), trips per wave per launch kind and the worst relative output error of fp16 weights (sub-normals kept) x fp16 V,
fp32 accumulation, against the float64 softmax.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

LOG2E = 1.4426950408889634
RW, RROWS = 4, 4


def region1d(p, n, s, sh):
    """csrc/attn_common.h: labels 0 | 1 | 2 split at n - s and n - sh; a zero shift labels the whole axis alike."""
    if sh == 0:
        return 0
    return 0 if p < n - s else (1 if p < n - sh else 2)


def rows_visit(qwh, kwh, qshy, kshy, hqa, hqb, hk_s):
    """rows_visit of csrc/attention_rows.hip for a window in the LAST window row of a masked launch (the image height drops out:
    rows qwh - qshy .. of such a window carry label 2, the rows above label 1): first key rows [lo, hi) of the chunks visited."""
    def lab(h, wh, sh):
        return region1d(h, wh, wh, sh)

    def skippable(hk0, rq):
        return all(lab(hk0 + r, kwh, kshy) != rq for r in range(RROWS))

    if qshy <= 0:
        return 0, kwh
    rq = lab(hqa, qwh, qshy)
    if rq != lab(hqb, qwh, qshy) or skippable(hk_s, rq):
        return 0, kwh
    lo, hi = hk_s, hk_s + RROWS
    while lo > 0 and not skippable(lo - RROWS, rq):
        lo -= RROWS
    while hi < kwh and not skippable(hi, rq):
        hi += RROWS
    return lo, hi


def visit_order(qwin, kwin, order="own", bottom=False, qshy=0, kshy=0):
    """Per workgroup: (units = [(first query row, first query column)], chunks = [(sk, chunk row)] in visiting order).
    Mirrors rows_geom / rows_span, the start chunk and rows_visit of attn_rows_kernel.  bottom: the window lies in the last window
    row of a launch whose rows are shifted by qshy (queries) / kshy (keys)."""
    (qwh, qww), (kwh, kww) = qwin, kwin
    qseg, nks, nrc = qww // 32, kww // 32, kwh // RROWS
    units = (qwh // 2) * qseg
    upw = min(RW, units)
    out = []
    for qs in range((units + upw - 1) // upw):
        u0, u1 = qs * upw, min(qs * upw + upw, units) - 1
        hqa, hqb = 2 * (u0 // qseg), 2 * (u1 // qseg) + 1
        sga, sgb = (u0 % qseg, u1 % qseg) if u0 // qseg == u1 // qseg else (0, qseg - 1)
        c0 = 0
        if order in ("own", "alt"):
            rc = min(((hqa + hqb + 1) * kwh) // (2 * qwh * RROWS), nrc - 1)
            sc = min(((sga + sgb + 1) * kww) // (2 * qww), nks - 1)
            c0 = sc * nrc + rc
        n = nks * nrc
        if order == "alt":     # nearest chunk first, alternating outwards (by linear chunk index)
            seq, lo, hi = [c0], c0 - 1, c0 + 1
            while len(seq) < n:
                if hi < n:
                    seq.append(hi); hi += 1
                if lo >= 0:
                    seq.append(lo); lo -= 1
        else:
            seq = [(c0 + i) % n for i in range(n)]
        if bottom:
            lo, hi = rows_visit(qwh, kwh, qshy, kshy, hqa, hqb, RROWS * (c0 % nrc))
            seq = [c for c in seq if lo <= RROWS * (c % nrc) < hi]
        out.append(([(2 * (u // qseg), 32 * (u % qseg)) for u in range(u0, u1 + 1)], [divmod(c, nrc) for c in seq]))
    return out


def simulate(S, qwin, kwin, floor, ceil_, rest, extra, order="own", bottom=None, shy=(0, 0)):
    """S: (n, qwh, qww, kwh, kww) log2-domain logits (bias and mask included) of n (window, head) pairs; floor / ceil_: (n,)
    lazy_floor / lazy_ceil of each pair's head; bottom: (n,) bool, the pair's window lies in the last window row of a launch
    shifted by shy = (query rows, key rows).  Returns (trips (n, waves) int, final offsets (n, qwh, qww), chunks visited (n, waves))."""
    if bottom is not None and bottom.any() and not bottom.all():
        parts = [(sel, simulate(S[sel], qwin, kwin, floor[sel], ceil_[sel], rest, extra, order, bottom[sel], shy)) for sel in (bottom, ~bottom)]
        outs = []
        for j in range(3):
            t = torch.empty(S.shape[0], *parts[0][1][j].shape[1:], dtype=parts[0][1][j].dtype)
            for sel, res in parts:
                t[sel] = res[j]
            outs.append(t)
        return tuple(outs)
    is_bottom = bottom is not None and bool(bottom.all())
    n = S.shape[0]
    msafe = torch.ceil(ceil_ - 13.5).view(n, 1)
    m_all = floor.view(n, 1, 1).expand(n, qwin[0], qwin[1]).clone()
    trips, visited = [], []
    for units, chunks in visit_order(qwin, kwin, order, is_bottom, shy[0], shy[1]):
        for (r0, c0) in units:
            Sw = S[:, r0:r0 + 2, c0:c0 + 32].reshape(n, 64, kwin[0], kwin[1])
            m = m_all[:, r0:r0 + 2, c0:c0 + 32].reshape(n, 64).clone()
            nochk = torch.zeros(n, dtype=torch.bool)
            t = torch.zeros(n, dtype=torch.long)

            def repair(mx, sel):
                nonlocal m, nochk
                d = (torch.ceil(mx - m) - rest).clamp_min(0.0)
                mn = m + d
                mn = torch.where((mn < msafe) & (mn >= msafe - extra), msafe.expand_as(mn), mn)
                m = torch.where(sel.view(n, 1), mn, m)
                nochk = torch.where(sel, (mn >= msafe).all(dim=1), nochk)

            for i, (sk, rc) in enumerate(chunks):
                C = Sw[:, :, RROWS * rc:RROWS * rc + RROWS, 32 * sk:32 * sk + 32]       # (n, 64, 4, 32)
                if i == 0:
                    repair(C.amax(dim=(2, 3)), torch.ones(n, dtype=torch.bool))
                    continue
                rowmax = C.amax(dim=3)                                                   # (n, 64, 4)
                over = ((rowmax - m.unsqueeze(2)) >= 14.0).any(dim=1) & ~nochk.view(n, 1)  # (n, 4): row trips the wave
                trip = over.any(dim=1)
                first = torch.where(trip, over.float().argmax(dim=1), torch.full((n,), RROWS, dtype=torch.long))
                rest_rows = torch.arange(RROWS).view(1, 1, RROWS) >= first.view(n, 1, 1)
                mx = torch.where(rest_rows, rowmax, torch.full_like(rowmax, -1e30)).amax(dim=2)
                repair(mx, trip)
                t += trip.long()
            trips.append(t)
            visited.append(torch.full((n,), len(chunks), dtype=torch.long))
            m_all[:, r0:r0 + 2, c0:c0 + 32] = m.view(n, 2, 32)
    return torch.stack(trips, dim=1), m_all, torch.stack(visited, dim=1)


def fp16_weight_error(S, V, m):
    """S (n, Nq, Nk) log2 logits, V (n, Nk, d), m (n, Nq) offsets: worst |out - ref| / max|ref| of fp16 weights (sub-normals kept)
    x fp16 V with fp32 accumulation against the float64 softmax."""
    w = torch.exp2(S.double() - m.double().unsqueeze(-1)).to(torch.float16).float()
    v16 = V.to(torch.float16).float()
    got = (w @ v16) / w.sum(-1, keepdim=True)
    p = torch.softmax(S.double() * math.log(2.0), dim=-1)
    ref = p @ V.double()
    return ((got.double() - ref).abs().amax() / ref.abs().amax()).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=64, help="tile side in LQ pixels")
    ap.add_argument("--rest", type=float, nargs="+", default=[-2.0], help="resting level ROWS_REST (the row maximum rests in (2^(rest-1), 2^rest])")
    ap.add_argument("--extra", type=float, default=None, help="ROWS_EXTRA (default: min(3, rest + 3), the kernel's rule)")
    ap.add_argument("--order", choices=["top", "own", "alt"], nargs="+", default=["own"], help="chunk order: (0, 0) upward / own chunk first, cyclic / own chunk first, alternating outwards")
    ap.add_argument("--random-init-scales", action="store_true")
    a = ap.parse_args()
    combos = [(r, a.extra if a.extra is not None else min(3.0, r + 3.0), o) for o in a.order for r in a.rest]

    from grl_image_restoration_amd import GRL, baseline_config, tables
    from oracle import grl_oracle as O

    cfg = baseline_config(3)
    cfg["img_size"] = a.side
    torch.manual_seed(0)
    model = GRL(**cfg).eval()
    if not a.random_init_scales:
        gs = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for name, p_ in model.named_parameters():
                if name.endswith("logit_scale"):
                    p_.copy_(math.log(100.0) + 0.3 * torch.randn(p_.shape, generator=gs))
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    x = torch.rand(1, 3, a.side, a.side, generator=torch.Generator().manual_seed(1))

    geom = {}
    stats = {}     # kind -> [trips, waves, worst error]
    win_attn, stripe_attn, cos_attn = O.window_attention, O.anchor_stripe_attention, O.cosine_attention

    def window_attention(qkv, x_size, window, shift, nh, p, prefix):
        geom["w"] = (tuple(window), tuple(window))
        geom["kinds"] = ["window"]
        geom["nw"], geom["shy"] = (x_size[0] // window[0], x_size[1] // window[1]), {"window": (shift, shift)}
        return win_attn(qkv, x_size, window, shift, nh, p, prefix)

    def anchor_stripe_attention(qkv, anchor, x_size, stripe, shift, do_shift, df, nh, p, prefix):
        astripe = tuple(s // df for s in stripe)
        geom["kinds"] = ["anchors->tokens", "tokens->anchors"]
        geom["anchors->tokens"], geom["tokens->anchors"] = (astripe, tuple(stripe)), (tuple(stripe), astripe)
        sy = shift[0] if do_shift else 0
        geom["nw"], geom["shy"] = (x_size[0] // stripe[0], x_size[1] // stripe[1]), {"anchors->tokens": (sy // df, sy), "tokens->anchors": (sy, sy // df)}
        return stripe_attn(qkv, anchor, x_size, stripe, shift, do_shift, df, nh, p, prefix)

    def cosine_attention(q, k, v, p, prefix, table, index, mask):
        kind = geom["kinds"].pop(0)
        qwin, kwin = geom["w"] if kind == "window" else geom[kind]
        B_, nh, Nq, _ = q.shape
        Nk = k.shape[2]
        scale = O.logit_scale(p, prefix).reshape(-1)
        s = torch.nn.functional.normalize(q, dim=-1) @ torch.nn.functional.normalize(k, dim=-1).transpose(-2, -1) * scale.view(1, nh, 1, 1)
        bt = O.bias_table(p, prefix, table)
        s = s + bt[index.reshape(-1)].view(Nq, Nk, nh).permute(2, 0, 1).unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            s = (s.view(B_ // nW, nW, nh, Nq, Nk) + mask.unsqueeze(1).unsqueeze(0)).view(-1, nh, Nq, Nk)
        S = (s * LOG2E).reshape(B_ * nh, Nq, Nk).float()
        floor = tables.lazy_floor(scale).repeat(B_)
        ceil_ = tables.lazy_ceil(scale, tables.kernel_table(bt)).repeat(B_)
        nwy, nwx = geom["nw"]
        bottom = ((torch.arange(B_) % (nwy * nwx)) // nwx == nwy - 1).repeat_interleave(nh) if mask is not None else None
        for rest, extra, order in combos:
            trips, m, vis = simulate(S.view(-1, *qwin, *kwin), qwin, kwin, floor, ceil_, rest, extra, order, bottom, geom["shy"][kind])
            err = fp16_weight_error(S, v.reshape(B_ * nh, Nk, -1), m.reshape(B_ * nh, Nq))
            st = stats.setdefault((rest, order, kind), [0, 0, 0.0, kwin[0] * kwin[1] // (RROWS * 32), 0])
            st[0] += int(trips.sum()); st[1] += trips.numel(); st[2] = max(st[2], err); st[4] += int(vis.sum())
        return cos_attn(q, k, v, p, prefix, table, index, mask)

    O.window_attention, O.anchor_stripe_attention, O.cosine_attention = window_attention, anchor_stripe_attention, cosine_attention
    with torch.no_grad():
        O.grl_forward(x, cfg, sd)
    for rest, extra, order in combos:
        print(f"# side {a.side}  rest {rest:g}  extra {extra:g}  order {order}  scales {'random-init' if a.random_init_scales else 'checkpoint-like (seed 7)'}")
        print(f"{'launch (chunks per wave)':28s} {'trips/wave':>10s} {'waves':>8s} {'fp16-weight rel. error':>24s} {'chunks visited':>15s}")
        for kind in ("window", "tokens->anchors", "anchors->tokens"):
            if (rest, order, kind) in stats:
                t, w, e, nch, v = stats[(rest, order, kind)]
                print(f"{kind + ' (' + str(nch) + ')':28s} {t / w:10.3f} {w:8d} {e:24.3e} {v / (w * nch):15.3f}")


if __name__ == "__main__":
    main()
