"""The training path of ``GRL`` (BASELINE config 5; reference: engines/base.py:221-236 = autograd through grl.py / efficient.py):
GRL.forward (grl.py:506-551) as a differentiable graph over the HIP kernels of autograd.py -- and, on CPU tensors, over the composite
torch contractions (composite.py).  Every function takes the model as its first argument.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import autograd as AG
from . import ops, tables
from . import switches as SW
from .geometry import BlockGeo, block_schedule

LOG2E = tables.LOG2E


def _const(model, key, make):
    """A constant tensor (or tuple of them) per geometry / device, built once by ``make()`` and kept on the model: a dozen tiny
    launches per call otherwise."""
    cache = model.__dict__.setdefault("_coords_cache", {})
    x = cache.get(key)
    if x is None:
        x = cache[key] = make()
    return x


def _scale(logit_scale):
    """exp(min(logit_scale, ln 100)) * log2e (efficient.py:39, exp2 domain), differentiable below the clamp."""
    return torch.clamp(logit_scale, max=math.log(1.0 / 0.01)).exp() * LOG2E


def _floor(sc):
    """tables.lazy_floor from the already scaled value ``sc`` = clamped scale * log2e (no gradient)."""
    return -1.0 - torch.ceil(sc.detach())


def _revidx(model, rows: int, dev):
    """Gather index of tables.kernel_table's row order: reversed, padded to a multiple of 4 with entries that repeat row 0 instead of
    being zero (no valid (query, key) pair addresses them)."""
    return _const(model, ("revidx", rows, str(dev)), lambda: torch.cat([torch.arange(rows - 1, -1, -1, device=dev),
                                                                        torch.zeros((-rows) % 4, dtype=torch.long, device=dev)]))


def _ones_nh(model, nh: int, dev):
    return _const(model, ("ones_nh", nh, str(dev)), lambda: torch.ones(nh, dtype=torch.float32, device=dev))


def _value_masks(model, d: int, v1: int, dev):
    """(dmask, onev): 1.0 on the real head dims / on the constant-1 column ``v1`` of a 32-wide value plane."""
    return (_const(model, ("dmask", d, str(dev)), lambda: (torch.arange(32, device=dev) < d).float()),
            _const(model, ("onev", d, str(dev)), lambda: (torch.arange(32, device=dev) == v1).float()))


def to_planes(model, t, one_col: int = -1, extra: int = 32):
    """[tokens, nh, d] -> fp32 head planes [nh, tokens, 32] in ONE launch: a cat with a cached constant block for the pad
    columns (F.pad is a fill plus a strided copy) -- zeros, and 1.0 in plane column ``one_col`` where the attention kernel
    wants a constant (k: slot 31, the partner of the running softmax offset; v: column d, the softmax denominator), so that
    the attention op needs no index fills (``prepared`` operands)."""
    M, nh, d = t.shape
    if d == extra:
        return t.permute(1, 0, 2).contiguous()

    def make():
        blk = torch.zeros(nh, M, extra - d, dtype=torch.float32, device=t.device)
        if one_col >= d:
            blk[..., one_col - d] = 1.0
        return blk

    return torch.cat([t.permute(1, 0, 2), _const(model, ("padblk", nh, M, extra - d, one_col, str(t.device)), make)], dim=2)


def block_planes(model, x, scales, one_cols, sc=None):
    """All head planes of a block's projection in ONE chain: ``x`` [tokens, S, nh, d] (S slots: q / k / v of the window branch and of
    the stripe branch; or the anchors, used twice) -> fp32 planes [S, nh, tokens, 32] plus their fp16 copy (the kernels' operands).
    ``scales[j]``: None = slot j is taken as it is (values), a tensor [nh] = L2-normalise over d and multiply (q: the clamped
    logit scale * log2e, k: ones); ``one_cols[j]``: plane column of slot j that holds 1.0 (-1: none).  The per-slot chain of
    round 4 (normalize, scale, permute + cat, fp16 copy -- and in the backward a strided [tokens, nh, d] -> [nh] reduction per
    logit scale) was ~35 launches forward and ~80 backward per block; here the scale rides on the per-token inverse norm
    (a tensor 1/d the size, so its gradient is a last-dim reduction plus a small column sum): 6 + ~12 launches."""
    T, S, nh, d = x.shape
    dev = x.device
    if ops.head_planes_ok(x, S) and SW.on("GRL_PLANES_KERNEL") and not ops.deterministic():
        # round 6: one launch forward (normalise, scale, pad constants, permute, fp16 copy), one backward (csrc/planes.hip).
        # An expanded input (the anchors, used as scaled queries and as keys) is passed once: both slots read input slot 0.
        expanded = x.stride(1) == 0
        xin = x[:, :1] if expanded else x
        ones = _ones_nh(model, nh, dev)
        if sc is None:                                                                   # (else: prebuilt for all blocks, train_tables)
            sc = torch.stack([ones if s is None else s for s in scales])                 # [S, nh] (differentiable in the q scales)
        # (the fp32 planes are autograd's handle on the operands only -- every consumer takes the fp16 copies, f16= of the attention
        # op -- so the kernel does not write them: GRL_PLANES_WRITE32=1 restores the values)
        outs = AG.HeadPlanesFn.apply(xin, sc, tuple(0 if expanded else j for j in range(S)), tuple(s is None for s in scales),
                                     tuple(int(c) for c in one_cols), SW.on("GRL_PLANES_WRITE32"))
        return outs[:S], outs[S:]

    def make():
        blk = torch.zeros(S, nh, T, 32 - d, dtype=torch.float32, device=dev)
        for j, c in enumerate(one_cols):
            if c >= d:
                blk[j, :, :, c - d] = 1.0
        raw = torch.tensor([s is None for s in scales], device=dev).view(1, S, 1, 1)
        return blk, raw, torch.ones(nh, dtype=torch.float32, device=dev)

    blk, raw, ones = _const(model, ("planes_const", T, S, nh, d, tuple(s is None for s in scales), tuple(one_cols), str(dev)), make)
    sc = torch.stack([ones if s is None else s for s in scales]).view(1, S, nh, 1)
    nrm = torch.linalg.vector_norm(x, dim=-1, keepdim=True)                      # F.normalize: v / max(|v|, 1e-12)
    inv = torch.where(raw, ones.view(1, 1, nh, 1), sc / nrm.clamp_min(1e-12))
    y = x * inv
    planes = torch.cat([y.permute(1, 2, 0, 3), blk], dim=3) if d < 32 else y.permute(1, 2, 0, 3).contiguous()
    return planes.unbind(0), planes.detach().to(ops.PLANE_DTYPE).unbind(0)


def train_tables(model, sched, dev):
    """The relative-position bias tables and clamped logit scales of EVERY block in a few batched chains (training path).
    The tables depend on the CPB-MLP weights only, not on activations, so nothing forces them to be built block by block:
    per geometry class (same coordinate table and head count) the 2 -> 512 -> nh MLPs of all blocks run as one broadcast
    layer and one bmm -- per block they were 3 x (7 launches forward, ~12 backward) with a K = 2 GEMM that the BLAS library
    takes 45-50 us for (16 ms of a 182 ms step).  Returns {(stage, block): ((table_w, table_a2w, table_w2a), scales [3, nh],
    floors [3, nh])}; only for blocks whose two branches have the same head count (the batched plane path)."""
    groups, blocks = {}, []
    for si, stage in enumerate(model.layers):
        for bi, blk in enumerate(stage.blocks):
            geo, a = sched[si][bi], blk.attn
            if geo.nh_w != geo.nh_s:
                continue
            ts = (a.window_attn.attn_transform, a.stripe_attn.attn_transform1, a.stripe_attn.attn_transform2)
            blocks.append(((si, bi), ts))
            for slot, (m, win, df) in enumerate(zip(ts, (geo.window, geo.stripe, geo.stripe), (1, geo.df, geo.df))):
                key = (tuple(win), df, tuple(m.cpb_mlp[2].weight.shape))
                groups.setdefault(key, []).append(((si, bi, slot), m))
    tabs = {}
    for (win, df, _), items in groups.items():
        coords = _const(model, (win, df, str(dev)), lambda: tables.coords_table(win, df, device=dev))
        idx = _revidx(model, coords.shape[0], dev)
        W1 = torch.stack([m.cpb_mlp[0].weight for _, m in items])            # [G, 512, 2]
        b1 = torch.stack([m.cpb_mlp[0].bias for _, m in items])              # [G, 512]
        W2 = torch.stack([m.cpb_mlp[2].weight for _, m in items])            # [G, nh, 512]
        # round 6: one launch forward, one backward, the [G, rows, 512] hidden layer (1.5 GB for the stripe transforms of GRL-Base)
        # never in memory (autograd.cpb_tables -> csrc/cpb.hip; CPU tensors: the torch expression)
        t = AG.cpb_tables(coords, W1, b1, W2, idx)                            # [G, nh, rows4], see attn_table
        for (key, _), tt in zip(items, t.unbind(0)):
            tabs[key] = tt
    out = {}
    if blocks:
        ls = torch.stack([m.logit_scale.reshape(-1) for _, ts in blocks for m in ts]).view(len(blocks), 3, -1)
        scales = _scale(ls)
        floors = _floor(scales)
        # the [slots, nh] scale matrices of the two plane launches of every block (q k v q k v | anchors as q, as k) from one cat
        # each and one unbind (per block: a stack forward, a stack backward)
        one = torch.ones(len(blocks), 1, scales.shape[2], dtype=scales.dtype, device=scales.device)
        sc6 = torch.cat([scales[:, 0:1], one, one, scales[:, 2:3], one, one], dim=1).unbind(0)
        sc2 = torch.cat([scales[:, 1:2], one], dim=1).unbind(0)
        for i, ((key, _), sc, fl) in enumerate(zip(blocks, scales.unbind(0), floors.unbind(0))):
            out[key] = (tuple(tabs[key + (slot,)] for slot in range(3)), sc, fl, sc6[i], sc2[i])
    return out


def attn_table(model, m, win, df, dev):
    """tables.kernel_table(16 * sigmoid(cpb_mlp(coords))) of one transform -- transpose, exp2 domain, reversed rows, padded to 4
    (_revidx) -- with autograd."""
    coords = _const(model, (tuple(win), df, str(dev)), lambda: tables.coords_table(win, df, device=dev))
    idx = _revidx(model, coords.shape[0], dev)
    return AG.cpb_tables(coords, m.cpb_mlp[0].weight.unsqueeze(0), m.cpb_mlp[0].bias.unsqueeze(0), m.cpb_mlp[2].weight.unsqueeze(0), idx)[0]


def block_train(model, r, blk, geo: BlockGeo, B, H, W, dp: float, pre=None):
    """EfficientMixAttnTransformerBlock.forward (efficient.py:539-556) on the token matrix r [B*H*W, C] with autograd."""
    C = model.embed_dim
    M = B * H * W
    nh_w, nh_s, df = geo.nh_w, geo.nh_s, geo.df
    d_w, d_s = C // 2 // nh_w, C // 2 // nh_s
    Ha, Wa = H // df, W // df
    a = blk.attn
    dev = r.device
    # (r has four consumers -- QKV projection, anchor pooling, the CAB, the residual: their gradients are added in one launch)
    r_q, r_p, r_c, r = AG.fan_out(r, 4)
    qkv = AG.linear(r_q, a.qkv.body.weight, a.qkv.body.bias)                               # QKVProjection (mixed_attn_block.py:669-676)
    pooled = r_p.view(B, Ha, df, Wa, df, C).mean(dim=(2, 4)).reshape(B * Ha * Wa, C)        # AnchorLinear avg-pool (:727-736)
    anc = AG.linear(pooled, a.anchor.body[0].reduction.weight, a.anchor.body[0].reduction.bias).view(-1, nh_s, d_s)
    same = (nh_w, d_w) == (nh_s, d_s) and SW.on("GRL_TRAIN_BATCHED_PLANES")
    if same:
        att = attention_train_batched(model, qkv, anc, a, geo, B, H, W, pre)
        return block_train_tail(model, r, att, blk, B, H, W, dp, r_c)
    if (nh_w, d_w) == (nh_s, d_s):   # one view, one unbind: the backward is a single stack instead of two slice-backwards (zeros + copy) and an add
        qw, kw, vw, qs, ks, vs = qkv.view(M, 6, nh_w, d_w).unbind(1)
    else:
        qw, kw, vw = qkv[:, : 3 * C // 2].reshape(M, 3, nh_w, d_w).unbind(1)
        qs, ks, vs = qkv[:, 3 * C // 2 :].reshape(M, 3, nh_s, d_s).unbind(1)
    P = lambda t, one_col=-1: to_planes(model, t, one_col)
    k1_w, k1_s = (31 if d_w <= 30 else -1), (31 if d_s <= 30 else -1)     # plane columns that hold a constant 1.0 (see to_planes)
    v1_w, v1_s = (d_w if d_w < 32 else -1), (d_s if d_s < 32 else -1)
    g_tok_w, g_tok_s, g_anc = geo.grids(H, W)
    # window attention (efficient.py:128-165)
    tw = a.window_attn.attn_transform
    sw = _scale(tw.logit_scale.reshape(-1))
    ow = AG.AttentionFn.apply(P(F.normalize(qw, dim=-1) * sw.view(1, nh_w, 1)), P(F.normalize(kw, dim=-1), k1_w), P(vw, v1_w),
                              attn_table(model, tw, geo.window, 1, dev),
                              dict(q=g_tok_w, k=g_tok_w, B=B, nh=nh_w, d=d_w, masked=geo.window_shift > 0, floor=_floor(sw), prepared=True))
    # anchored stripe attention (efficient.py:215-270): anchors -> stripe tokens, then stripe tokens -> anchors
    t1, t2 = a.stripe_attn.attn_transform1, a.stripe_attn.attn_transform2
    an = F.normalize(anc, dim=-1)
    s1, s2 = _scale(t1.logit_scale.reshape(-1)), _scale(t2.logit_scale.reshape(-1))
    y = AG.AttentionFn.apply(P(an * s1.view(1, nh_s, 1)), P(F.normalize(ks, dim=-1), k1_s), P(vs, v1_s),
                             attn_table(model, t1, geo.stripe, df, dev),
                             dict(q=g_anc, k=g_tok_s, B=B, nh=nh_s, d=d_s, masked=geo.stripe_shift, floor=_floor(s1), prepared=True))
    dmask, onev = _value_masks(model, d_s, v1_s, dev)
    yv = torch.addcmul(onev, y, dmask)                              # real head dims only, and the constant 1.0 in column d again
    os_ = AG.AttentionFn.apply(P(F.normalize(qs, dim=-1) * s2.view(1, nh_s, 1)), P(an, k1_s), yv,
                               attn_table(model, t2, geo.stripe, df, dev),
                               dict(q=g_tok_s, k=g_anc, B=B, nh=nh_s, d=d_s, masked=geo.stripe_shift, floor=_floor(s2), prepared=True))
    if d_w == d_s:                    # one cat of the planes, one slice (its backward: one zeros + copy instead of two)
        att = torch.cat([ow, os_], dim=0).permute(1, 0, 2)[..., :d_w].reshape(M, C)
    else:
        att = torch.cat([ow.permute(1, 0, 2)[..., :d_w].reshape(M, C // 2), os_.permute(1, 0, 2)[..., :d_s].reshape(M, C // 2)], dim=1)
    return block_train_tail(model, r, att, blk, B, H, W, dp)


def attention_train_batched(model, qkv, anc, a, geo: BlockGeo, B, H, W, pre=None):
    """The three attention calls of a block (as in block_train) with all head planes built by two block_planes chains."""
    C = model.embed_dim
    M = B * H * W
    nh, df = geo.nh_w, geo.df
    d = C // 2 // nh
    dev = qkv.device
    k1, v1 = (31 if d <= 30 else -1), (d if d < 32 else -1)
    tw, t1, t2 = a.window_attn.attn_transform, a.stripe_attn.attn_transform1, a.stripe_attn.attn_transform2
    # the three clamped logit scales (efficient.py:39) and their lazy-offset floors in one chain each instead of three
    if pre is None:
        scales = _scale(torch.stack([tw.logit_scale.reshape(-1), t1.logit_scale.reshape(-1), t2.logit_scale.reshape(-1)]))
        floors = _floor(scales)
        tabs = (attn_table(model, tw, geo.window, 1, dev), attn_table(model, t1, geo.stripe, df, dev),
                attn_table(model, t2, geo.stripe, df, dev))
    sc6 = sc2 = None
    if pre is not None:                                                  # (built for all blocks at once: train_tables)
        tabs, scales, floors, sc6, sc2 = pre
    sw, s1, s2 = scales.unbind(0)
    fw, f1, f2 = floors.unbind(0)
    ones = _ones_nh(model, nh, dev)
    # slots of the projection: q k v (window branch), q k v (stripe branch); the anchors serve as queries (scaled) and as keys
    (qw, kw, vw, qs, ks, vs), (qw16, kw16, vw16, qs16, ks16, vs16) = block_planes(
        model, qkv.view(M, 6, nh, d), (sw, ones, None, s2, ones, None), (-1, k1, v1, -1, k1, v1), sc=sc6)
    (aq, ak), (aq16, ak16) = block_planes(model, anc.view(-1, 1, nh, d).expand(-1, 2, nh, d), (s1, ones), (-1, k1), sc=sc2)

    g_tok_w, g_tok_s, g_anc = geo.grids(H, W)
    # (round 6: the two branch outputs as token matrices [M, nh * 32]: one cat along the channels gives the projection's input --
    # block_train_tail places the weight columns accordingly -- and the cat's backward hands each attention backward its column
    # block of the gradient in place; before: cat of the planes, permute, slice, copy, and zeros + copy + two copies back)
    ow = AG.AttentionFn.apply(qw, kw, vw, tabs[0],
                              dict(q=g_tok_w, k=g_tok_w, B=B, nh=nh, d=d, masked=geo.window_shift > 0, floor=fw, prepared=True,
                                   f16=(qw16, kw16, vw16), token_major=True))
    y = AG.AttentionFn.apply(aq, ks, vs, tabs[1],
                             dict(q=g_anc, k=g_tok_s, B=B, nh=nh, d=d, masked=geo.stripe_shift, floor=f1, prepared=True,
                                  f16=(aq16, ks16, vs16)))
    dmask, onev = _value_masks(model, d, v1, dev)
    if y.is_cuda and d < 31:
        # the kernel's output already IS the prepared value operand: column d = the softmax denominator over itself (1.0, exact
        # once rounded to fp16), column 31 = 0.  Only the gradient of the pad columns has to go (round 6: an addcmul forward and
        # three multiplies backward before).
        yv = AG.PadGradMask.apply(y, dmask)
    else:
        yv = torch.addcmul(onev, y, dmask)                          # real head dims only, and the constant 1.0 in column d again
    os_ = AG.AttentionFn.apply(qs, ak, yv, tabs[2],
                               dict(q=g_tok_s, k=g_anc, B=B, nh=nh, d=d, masked=geo.stripe_shift, floor=f2, prepared=True,
                                    f16=(qs16, ak16, None), token_major=True))
    return torch.cat([ow, os_], dim=1)                              # [M, 2 * nh * 32]


def block_train_tail(model, r, att, blk, B, H, W, dp: float, r_conv=None):
    """proj + norm1 + residual, CAB, MLP + norm2 + residual of a block (efficient.py:543-556) on token matrices."""
    C = model.embed_dim
    a = blk.attn
    if att.shape[1] != C:
        # att = [M, heads * 32]: head h's d channels at columns 32 h .. 32 h + d - 1 (the attention kernels' own layout); the weight
        # columns go where their channels are, zero elsewhere.  Column d of a head holds the softmax denominator over itself = 1.0
        # (v's ones column through the PV product): the bias gradient's ones column.
        nht = att.shape[1] // 32
        dh = C // nht
        zb = _const(model, ("wzero", C, nht, 32 - dh, str(att.device)),
                    lambda: torch.zeros(C, nht, 32 - dh, dtype=torch.float32, device=att.device))
        wpad = torch.cat([a.proj.weight.view(C, nht, dh), zb], dim=2).view(C, nht * 32)
        x1 = AG.linear(att, wpad, a.proj.bias, one_col=dh if dh < 32 else -1)
    else:
        x1 = AG.linear(att, a.proj.weight, a.proj.bias)
    x1 = norm_residual(model, r, x1, blk.norm1, H * W, dp)
    if model.local_connection:   # CAB + ChannelAttention (mixed_attn_block.py:948-983)
        c0, c2, se = blk.conv.cab[0], blk.conv.cab[2], blk.conv.cab[3].attention
        u = AG.conv3x3(F.gelu(AG.conv3x3(r if r_conv is None else r_conv, c0.weight, c0.bias, B, H, W)), c2.weight, c2.bias, B, H, W)
        # x1 + u * gate(u): pool, squeeze-excite MLP and the gated residual as three launches each way (autograd.se_residual)
        x1 = AG.se_residual(x1, u, se[1].weight.flatten(1), se[1].bias, se[3].weight.flatten(1), se[3].bias, H * W)
    # Mlp (swin_v1_block.py:37-43): the GELU between fc1 and fc2 is taken by fc2's loader, its adjoint by the epilogue of fc2's
    # data-gradient launch (autograd.linear gelu_in)
    h1 = AG.linear(x1, blk.mlp.fc1.weight, blk.mlp.fc1.bias)
    m = AG.linear(h1, blk.mlp.fc2.weight, blk.mlp.fc2.bias, gelu_in=True)
    return norm_residual(model, x1, m, blk.norm2, H * W, dp)


def norm_residual(model, r, t, norm, rows_per_image: int, p: float):
    """r + res_scale * DropPath(norm(t)) (efficient.py:543-556; timm DropPath, scale_by_keep: one Bernoulli draw per image) inside the
    LayerNorm launches (autograd.layer_norm_residual)."""
    if p == 0.0 or not model.training:
        return AG.layer_norm_residual(r, t, norm.weight, norm.bias, 1e-5, None, rows_per_image, model.res_scale)
    keep = 1.0 - p
    m = t.new_empty(t.shape[0] // rows_per_image).bernoulli_(keep)
    return AG.layer_norm_residual(r, t, norm.weight, norm.bias, 1e-5, m, rows_per_image, model.res_scale / keep)


def forward(model, x):
    """GRL.forward (grl.py:506-551) as a differentiable graph over the HIP kernels (autograd.py)."""
    H0, W0 = x.shape[2:]
    first = model.conv_first.weight
    if x.is_cuda and getattr(model, "_ag_registered", None) != (first.data_ptr(), first.device):   # (re)register after .to() / load
        AG.register_parameters(model)
        model._ag_registered = (first.data_ptr(), first.device)
    # (a float64 model on the composite path computes in float64; every other input is cast to float32, whatever it came as)
    x = model.check_image_size(x.to(first.dtype) if (first.dtype == torch.float64 and not x.is_cuda) else x.float())
    mean = model._mean.to(x.device, x.dtype)
    x = (x - mean) * model.img_range
    B, Cin, H, W = x.shape
    s = model.upscale
    sched = block_schedule(model.depths, model.num_heads_window, model.num_heads_stripe, model.window_size, model.stripe_size,
                           model.stripe_groups, model.stripe_shift, model.df, (H, W))

    def conv(t, m, b=B, h=H, w=W):
        return AG.conv3x3(t, m.weight, m.bias, b, h, w)

    def shuffle(t, b, h, w, r):   # PixelShuffle(r) on a token matrix [b*h*w, c*r*r] -> [b*h*r*w*r, c]
        c = t.shape[1] // (r * r)
        return t.view(b, h, w, c, r, r).permute(0, 1, 4, 2, 5, 3).reshape(b * h * r * w * r, c)

    def image(t, h, w):
        return t.view(B, h, w, -1).permute(0, 3, 1, 2)

    f = conv(x.permute(0, 2, 3, 1).reshape(B * H * W, Cin), model.conv_first)
    z = AG.layer_norm(f, model.norm_start.weight, model.norm_start.bias, 1e-5)
    pre = train_tables(model, sched, x.device) if SW.on("GRL_TRAIN_BATCHED_PLANES") else {}
    j = 0
    for si, stage in enumerate(model.layers):
        r = z
        for bi, blk in enumerate(stage.blocks):
            r = block_train(model, r, blk, sched[si][bi], B, H, W, model._dpr[j], pre.get((si, bi)))
            j += 1
        z = conv(r, stage.conv) + z
    z = AG.layer_norm(z, model.norm_end.weight, model.norm_end.bias, 1e-5)
    body = conv(z, model.conv_after_body) + f
    if model.upsampler == "pixelshuffle":
        y = F.leaky_relu(conv(body, model.conv_before_upsample[0]), 0.01)
        h, w = H, W
        r = 3 if model.upscale == 3 else 2
        for m in model.upsample.up:
            if isinstance(m, nn.Conv2d):
                y = shuffle(conv(y, m, B, h, w), B, h, w, r)
                h, w = h * r, w * r
        y = image(conv(y, model.conv_last, B, h, w), h, w)
    elif model.upsampler == "pixelshuffledirect":
        y = image(shuffle(conv(body, model.upsample.up[0]), B, H, W, s), H * s, W * s)
    elif model.upsampler == "nearest+conv":
        def up2(t, h, w):
            return t.view(B, h, 1, w, 1, -1).expand(B, h, 2, w, 2, t.shape[1]).reshape(B * 4 * h * w, -1)

        y = F.leaky_relu(conv(body, model.conv_before_upsample[0]), 0.01)
        y = F.leaky_relu(conv(up2(y, H, W), model.conv_up1, B, 2 * H, 2 * W), 0.2)
        y = F.leaky_relu(conv(up2(y, 2 * H, 2 * W), model.conv_up2, B, 4 * H, 4 * W), 0.2)
        y = F.leaky_relu(conv(y, model.conv_hr, B, 4 * H, 4 * W), 0.2)
        y = image(conv(y, model.conv_last, B, 4 * H, 4 * W), 4 * H, 4 * W)
    else:
        y = image(conv(body, model.conv_last), H, W)
        if model.in_channels == model.out_channels:
            y = x + y
    y = y / model.img_range + mean
    y = y[:, :, : H0 * s, : W0 * s].contiguous()
    return AG.GradScaleTop.apply(y) if y.is_cuda else y      # (the gradient operand scale belongs to the fp16 HIP contractions)
