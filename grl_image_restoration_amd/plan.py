"""Packing the weights and tables of a ``GRL`` into a *plan*: what the inference launch sequence (forward_infer.py) hands to the kernels.

A plan belongs to one input size, one device and one state of the parameters (``GRL._plan`` caches it).  Which kernel a block runs
is decided HERE, by which optional field of its ``BlockPlan`` is packed; forward_infer.py only tests ``is not None``.  The plans are
dataclasses, so a field that is not declared fails when the plan is built instead of quietly selecting the generic kernel.

Every function takes the model as its first argument; nothing here launches a forward except the calibration probe.
"""
import dataclasses
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, tables
from . import switches as SW
from .geometry import BlockGeo, block_schedule, table_rows

LOG2E = tables.LOG2E
Tensor = torch.Tensor


def _pad32(n: int) -> int:
    return (n + 31) // 32 * 32


def _padv(v, n: int, dev):
    """Vector ``v`` as fp32 on ``dev``, zero padded to ``n`` entries."""
    out = torch.zeros(n, dtype=torch.float32, device=dev)
    out[: v.numel()] = v.detach().float()
    return out


@dataclass
class BlockPlan:
    """Packed weights / tables of one block.  Fields without a default are packed on every route."""

    hi: bool                       # the block runs on split operands (forward_infer.block_high)
    one_w: bool                    # K planes carry 1.0 in head-dim slot 31 (window branch / stripe branch): partner of the
    one_s: bool                    # attention kernel's running softmax offset
    qkv_w: Any                     # [G*32, CP] fp16, or the split3 image when hi
    qkv_b: Tensor
    qkv_gs: Tensor                 # per-slot group scale of the EPI_GROUPNORM epilogue (clamped logit scale * log2e for q)
    anc_w: Any
    anc_b: Tensor
    anc_gs: Tensor
    proj_w: Any
    proj_b: Tensor
    n1_g: Tensor
    n1_b: Tensor
    fc1_w: Any
    fc1_b: Tensor
    fc2_w: Any
    fc2_b: Tensor
    n2_g: Tensor
    n2_b: Tensor
    tab_w: Tensor                  # relative-position bias tables in the kernel's exp2 domain
    tab_a2w: Tensor
    tab_w2a: Tensor
    tr_w: bool                     # the table (and the launch) is on the transposed view of the grids: ops.attention, row kernel
    tr_a2w: bool
    tr_w2a: bool
    floor_w: Tensor                # lazy softmax offsets of ops.attention
    floor_a2w: Tensor
    floor_w2a: Tensor
    ceil_w: Any
    ceil_a2w: Any
    ceil_w2a: Any
    hi_c: bool = False             # the CAB convolutions on split operands too (conv3x3 x_split=3, fp32 mid tensor)
    hiq: bool = False              # fast block above hiq_scale: q / k / anchor planes from the split-operand projection
    qkv_w3: Any = None             # hiq: split3 QKV weights -- ops.linear a_split=3 (linear_split kernels)
    qkv_w3r: Any = None            # hiq: their register image -- ops.linear w_regs (csrc/linear_split.hip)
    anc_w3: Any = None             # hiq: split3 anchor weights -- ops.linear a_split=3
    qkv_blob: Any = None           # ops.qkv: one-pass streaming QKV kernel (csrc/qkv.hip)
    qkv_slots: Optional[int] = None            # ops.qkv: number of 32-wide plane slots
    qa_blob: Any = None            # ops.qkv_anchor: q/k/v + pooled anchors in one pass (csrc/qkv_anchor.hip)
    qa_slots: Optional[Tuple[int, int]] = None  # ops.qkv_anchor: (qkv slots, anchor slots)
    qa_lo: Any = None              # ops.qkv_anchor lo_blob: the same pass on split operands (qkv_split_kernel)
    qkv_wr: Any = None             # hi: register images for ops.linear w_regs (csrc/linear_split.hip; None: generic kernel)
    anc_wr: Any = None             # hi: ... and the pooled-anchor route of block_high
    proj_wr: Any = None            # hi: ... with fc2_wr, the fused-LN epilogue of block_high
    fc1_wr: Any = None             # hi: ops.linear w_regs
    fc2_wr: Any = None             # hi: ops.linear w_regs
    proj_blob: Any = None          # ops.block_tail: proj + norm1 + CAB + MLP in one kernel (csrc/tail.hip)
    tail_rblob: Any = None         # ops.block_tail rblob: weights stationary in registers (csrc/tail_regs.hip)
    mlp_blob: Any = None           # ops.mlp / ops.block_tail: fused fc1 -> GELU -> fc2 -> norm2 -> residual (csrc/mlp.hip)
    mlp_hp: Optional[int] = None   # ops.mlp / ops.block_tail: padded hidden width
    cab0_split: Optional[int] = None   # ops.conv3x3 x_split of the CAB's first convolution (1 | 2 | 3)
    cab0_w: Any = None             # ops.conv3x3 (CAB conv1, GELU)
    cab0_b: Any = None
    cab2_w: Any = None             # ops.conv3x3 want_pool (CAB conv2, generic route)
    cab2_b: Any = None
    cab_mid: Optional[int] = None  # padded channel count of the tensor between the two CAB convolutions
    se1_w: Any = None              # ops.se_scale: squeeze-excite gate
    se1_b: Any = None
    se3_w: Any = None
    se3_b: Any = None
    cab2_blob: Any = None          # ops.cab_conv2: filters-in-registers conv2 + pool (csrc/cab_conv2.hip)
    cab2_bias: Any = None          # ops.cab_conv2


@dataclass
class StagePlan:
    blocks: List[BlockPlan]
    conv_w: Any                    # ops.conv3x3 of the stage (x_split = Plan.xs["stage_conv"])
    conv_b: Any


@dataclass
class Plan:
    """Packed weights / tables of the whole network for one input size.  ``first`` .. ``last`` are (weight, bias) pairs of ops.conv3x3."""

    sched: List[List[BlockGeo]]
    stages: List[StagePlan]
    split: int                     # x_split of the tail convolutions: 3 (high) | 1
    xs: Dict[str, int]             # x_split of the sites named in GRL_SPLIT_SITES: stage_conv, after, last
    ns_g: Tensor                   # ops.layernorm (norm_start / norm_end)
    ns_b: Tensor
    ne_g: Tensor
    ne_b: Tensor
    first: Tuple                   # conv_first
    after: Tuple                   # conv_after_body
    cbu: Optional[Tuple] = None    # conv_before_upsample (pixelshuffle, nearest+conv)
    ups: Optional[List[Tuple]] = None   # pixelshuffle: conv + PixelShuffle steps (ops.conv3x3 shuffle_r)
    ups_r: Optional[int] = None
    upd: Optional[Tuple] = None    # pixelshuffledirect (ops.conv3x3 shuffle_r, shuffle_cg=upd_cg)
    upd_cg: Optional[int] = None
    up1: Optional[Tuple] = None    # nearest+conv
    up2: Optional[Tuple] = None
    hr: Optional[Tuple] = None
    last: Optional[Tuple] = None   # conv_last (every tail but pixelshuffledirect)


def _split_sites(spec: str) -> dict:
    """'stage_conv:x,after,last,cab0' -> {site: x_split}: 3 = activations and weights split (three MFMA terms), ':x' = 2 = only the
    activations (two terms; for sites where the rounding of x matters and that of W does not, tools/precision_sites.py combo)."""
    out = {}
    for item in spec.split(","):
        if item:
            name, _, mode = item.partition(":")
            out[name] = 2 if mode == "x" else 3
    return out


def predicted_split_count(var_desc, base_var: float, bar_rms: float, margin: float = 0.9) -> int:
    """How many blocks -- taken from the front of ``var_desc``, the per-block error variances in DESCENDING order -- must move to split
    operands so that the variance left (``base_var``: what remains with every block split, plus the variances of the blocks that stay on
    fp16 operands; independent rounding errors add in variance) stays within ``(margin * bar_rms)^2``.  The calibration verifies the
    prediction on the probe and raises the count until it passes (calibrated_plan)."""
    k, acc = len(var_desc), base_var
    for j in range(len(var_desc) - 1, -1, -1):        # blocks that may stay on fp16 operands, cheapest first
        if acc + var_desc[j] > (margin * bar_rms) ** 2:
            break
        acc += var_desc[j]
        k = j
    return k


def pack_block(model, blk, geo: BlockGeo, dev, hi: Optional[bool] = None, cab_split: Optional[bool] = None,
               allow_hiq: bool = True) -> BlockPlan:
    """Packed weights / tables of one block.  ``hi``: this block runs on split operands (None: as the model's precision says;
    `auto` may choose it block by block, see calibrated_plan); ``cab_split``: the CAB convolutions of a split block on split
    operands too (None: high_cab_fp16 decides)."""
    C = model.embed_dim
    CP = _pad32(C)
    nh_w, nh_s = geo.nh_w, geo.nh_s
    d_w, d_s = C // 2 // nh_w, C // 2 // nh_s
    a = blk.attn
    f32 = dict(dtype=torch.float32, device=dev)

    def aff(m):
        return tables.clamped_scale(m.logit_scale).to(dev)

    sc_w, sc_1, sc_2 = aff(a.window_attn.attn_transform), aff(a.stripe_attn.attn_transform1), aff(a.stripe_attn.attn_transform2)
    # K planes carry 1.0 in the spare head-dim slot 31 (negative gscale): partner of the attention kernel's running
    # softmax offset, which lives in slot 31 of its Q fragments (include/grl_hip.h)
    one_w, one_s = d_w <= 30, d_s <= 30
    if hi is None:
        hi = model.precision == "high"
    fast_cp = not hi and CP in (64, 128, 192)          # the widths the one-pass fast-mode kernels are built for
    opt: Dict[str, Any] = {}                           # the optional fields of this block

    # --- QKV: one 32-wide slot per (branch, q|k|v, head); v slots carry a constant-1 column ---
    W = a.qkv.body.weight.detach().float()
    b = a.qkv.body.bias.detach().float()
    G = 3 * nh_w + 3 * nh_s
    Wp = torch.zeros(G * 32, CP, **f32)
    bp = torch.zeros(G * 32, **f32)
    gs = torch.zeros(G, **f32)
    for br, (nh, d, base_o, base_g) in enumerate(((nh_w, d_w, 0, 0), (nh_s, d_s, 3 * C // 2, 3 * nh_w))):
        for which in range(3):
            for h in range(nh):
                g = base_g + which * nh + h
                o0 = base_o + which * (C // 2) + h * d
                Wp[g * 32 : g * 32 + d, :C] = W[o0 : o0 + d]
                bp[g * 32 : g * 32 + d] = b[o0 : o0 + d]
                if which == 2 and d < 32:
                    bp[g * 32 + d] = 1.0
                if which == 0:
                    gs[g] = (sc_w[h] if br == 0 else sc_2[h]) * LOG2E
                elif which == 1:
                    one = one_w if br == 0 else one_s
                    gs[g] = (1.0 if br == 0 else sc_1[h] * LOG2E) * (-1.0 if one else 1.0)
    G16 = ops.GEMM_DTYPE
    qkv_w = ops.split3_weight(Wp) if hi else Wp.to(G16)
    # fast mode, logit scales beyond GRL_HIQ_SCALE (trained checkpoints sit at the clamp, 100): the q / k / anchor planes come from
    # the split-operand projection -- at scale 100 the fp16 rounding of x and W in this one GEMM is the largest single
    # contribution to the output error (tools/precision_sites.py: rms 8.9e-5 of 1.6e-4), amplified by the scale itself
    hiq = (not hi) and allow_hiq and float(max(sc_w.max(), sc_1.max(), sc_2.max())) > model.hiq_scale
    if hiq:
        opt.update(qkv_w3=ops.split3_weight(Wp))
        opt.update(qkv_w3r=ops.pack_linear_split(opt["qkv_w3"]))
    if fast_cp:  # one-pass streaming QKV kernel (csrc/qkv.hip)
        opt.update(qkv_blob=ops.pack_qkv(Wp, bp, gs), qkv_slots=G)

    # --- anchor projection (avg-pool fused in the kernel) ---
    Wa = a.anchor.body[0].reduction.weight.detach().float()
    ba = a.anchor.body[0].reduction.bias.detach().float()
    Wap = torch.zeros(nh_s * 32, CP, **f32)
    bap = torch.zeros(nh_s * 32, **f32)
    for h in range(nh_s):
        Wap[h * 32 : h * 32 + d_s, :C] = Wa[h * d_s : (h + 1) * d_s]
        bap[h * 32 : h * 32 + d_s] = ba[h * d_s : (h + 1) * d_s]
    anc_w = ops.split3_weight(Wap) if hi else Wap.to(G16)
    anc_gs = torch.full((nh_s,), -1.0 if one_s else 1.0, **f32)
    if hiq:
        opt.update(anc_w3=ops.split3_weight(Wap))
    if fast_cp:   # q/k/v + 2x2-pooled anchors in one pass over x (csrc/qkv_anchor.hip)
        opt.update(qa_blob=ops.pack_qkv_anchor(Wp, bp, gs, Wap, bap, anc_gs), qa_slots=(G, nh_s))
        if hiq and CP == 192 and (nh_w, nh_s) == (3, 3):   # the same pass on split operands (qkv_split_kernel, round 4)
            opt.update(qa_lo=ops.pack_qkv_anchor_lo(torch.cat([Wp, Wap]), torch.cat([gs, anc_gs])))

    # --- output projection over the slotted attention output + norm1 ---
    Wo = a.proj.weight.detach().float()
    KA = (nh_w + nh_s) * 32
    Wop = torch.zeros(CP, KA, **f32)
    for h in range(nh_w):
        Wop[:C, h * 32 : h * 32 + d_w] = Wo[:, h * d_w : (h + 1) * d_w]
    for h in range(nh_s):
        Wop[:C, (nh_w + h) * 32 : (nh_w + h) * 32 + d_s] = Wo[:, C // 2 + h * d_s : C // 2 + (h + 1) * d_s]
    proj_w = ops.split3_weight(Wop) if hi else Wop.to(G16)

    # --- MLP + norm2 ---
    Hd = blk.mlp.fc1.weight.shape[0]
    HP = _pad32(Hd)
    W1 = torch.zeros(HP, CP, **f32)
    W1[:Hd, :C] = blk.mlp.fc1.weight.detach().float()
    W2 = torch.zeros(CP, HP, **f32)
    W2[:C, :Hd] = blk.mlp.fc2.weight.detach().float()
    fc1_w = ops.split3_weight(W1) if hi else W1.to(G16)
    fc2_w = ops.split3_weight(W2) if hi else W2.to(G16)
    if hi:   # register images of the split weights for the weights-stationary kernel (csrc/linear_split.hip; None: generic kernel)
        opt.update(qkv_wr=ops.pack_linear_split(qkv_w), anc_wr=ops.pack_linear_split(anc_w), proj_wr=ops.pack_linear_split(proj_w),
                   fc1_wr=ops.pack_linear_split(fc1_w), fc2_wr=ops.pack_linear_split(fc2_w))
    if fast_cp and KA == CP and model.local_connection:   # + proj/norm1/CAB in front: one kernel per block tail
        opt.update(proj_blob=ops.pack_proj(Wop))
        # weights stationary in registers (csrc/tail_regs.hip, round 4): 255 against 290 us per 4 tiles.  Its register image is built for
        # the Base widths only (192 padded channels, 384 hidden, more than 160 real channels); every other width streams its weights
        if CP == 192 and HP == 384 and C > 160:
            opt.update(tail_rblob=ops.pack_tail_regs(Wop, blk.mlp.fc1.weight.to(dev), blk.mlp.fc1.bias.to(dev), blk.mlp.fc2.weight.to(dev)))
    if fast_cp:  # fused fc1 -> GELU -> fc2 -> norm2 -> residual kernel (csrc/mlp.hip)
        opt.update(mlp_blob=ops.pack_mlp(blk.mlp.fc1.weight.to(dev), blk.mlp.fc1.bias.to(dev), blk.mlp.fc2.weight.to(dev), CP, HP),
                   mlp_hp=HP)

    # --- relative-position bias tables in the kernel's exp2 domain ---
    # A (query window, key window) pair that is not 32-aligned as it stands but is so with the image axes swapped -- the
    # 128x64 stripes / 32x16 anchors of every other block of the dn geometry -- is launched on the transposed view of its
    # grids (GrlTokenGrid.transposed) with the transposed table: row-streaming kernel instead of the generic one.
    def table(m, win, df, q_win, k_win, q_sh, k_sh, masked, d):
        coords = tables.coords_table(win, df, device=dev)
        bias = tables.bias_rows(m.cpb_mlp[0].weight.to(dev), m.cpb_mlp[0].bias.to(dev), m.cpb_mlp[2].weight.to(dev), coords)
        sw = lambda t: (t[1], t[0])
        tr = (not hi
              and not ops.attention_rows_ok(q_win, k_win, q_sh, k_sh, masked, d)
              and ops.attention_rows_ok(sw(q_win), sw(k_win), sw(q_sh), sw(k_sh), masked, d))
        if tr:
            bias = ops.transpose_table(bias, q_win, k_win)
        return tables.kernel_table(bias), tr

    wsh = (geo.window_shift, geo.window_shift)
    tab_w, tr_w = table(a.window_attn.attn_transform, geo.window, 1, geo.window, geo.window, wsh, wsh, geo.window_shift > 0, d_w)
    tab_a2w, tr_a2w = table(a.stripe_attn.attn_transform1, geo.stripe, geo.df, geo.anchor_stripe, geo.stripe,
                            geo.anchor_shift_size, geo.stripe_shift_size, geo.stripe_shift, d_s)
    tab_w2a, tr_w2a = table(a.stripe_attn.attn_transform2, geo.stripe, geo.df, geo.stripe, geo.anchor_stripe,
                            geo.stripe_shift_size, geo.anchor_shift_size, geo.stripe_shift, d_s)
    assert tab_w.shape[1] == (table_rows(geo.window, geo.window) + 3) // 4 * 4
    assert tab_a2w.shape[1] == (table_rows(geo.anchor_stripe, geo.stripe) + 3) // 4 * 4

    # --- CAB: conv3x3 C->C/4 (GELU), conv3x3 C/4->C, squeeze-excite gate (mixed_attn_block.py:948-983) ---
    if model.local_connection:
        c0, c2 = blk.conv.cab[0], blk.conv.cab[2]
        se = blk.conv.cab[3].attention
        Cm = c0.weight.shape[0]
        CmO, CmI = (Cm + 15) // 16 * 16, _pad32(Cm)  # conv1 writes CmO channels of a zeroed CmI-wide matrix
        # (the CAB convs of an auto-resolved `high` Base-width model stay on fp16 operands)
        hi_c = hi and (cab_split if cab_split is not None else not high_cab_fp16(model))
        if hi_c:
            CmO = CmI   # fp32 mid tensor written by the plain store path: every channel of its row comes from the conv
        sp = 3 if hi_c else 1
        sites = _split_sites(SW.text("GRL_SPLIT_SITES", default=model.split_sites))
        # the CAB's first conv on split operands: everything-split `high`; the fast path's per-site choice (see build_plan); fp16 in the
        # auto-resolved `high` of a Base-width model (high_cab_fp16: every other site is split there, so this one can afford it)
        cab0_split = 3 if hi_c else (1 if hi else sites.get("cab0", 1))
        opt.update(
            hi_c=hi_c, cab0_split=cab0_split,
            cab0_w=ops.pack_conv_weight(c0.weight.to(dev), CP, CmO, split=cab0_split), cab0_b=ops.pack_conv_bias(c0.bias.to(dev), CmO),
            cab2_w=ops.pack_conv_weight(c2.weight.to(dev), CmI, CP, split=sp), cab2_b=ops.pack_conv_bias(c2.bias.to(dev), CP),
            cab_mid=CmI,
            se1_w=se[1].weight.detach().float().reshape(se[1].weight.shape[0], C).to(dev).clone(),   # copies: a plan never aliases
            se1_b=se[1].bias.detach().float().to(dev).clone(),                                        # the live parameters
            se3_w=se[3].weight.detach().float().reshape(C, -1).to(dev).clone(),
            se3_b=se[3].bias.detach().float().to(dev).clone(),
        )
        if not hi_c and CP == 192 and Cm <= 48 and CmI >= 56:
            opt["cab2_blob"], opt["cab2_bias"] = ops.pack_cab_conv2(c2.weight.to(dev), c2.bias.to(dev))   # csrc/cab_conv2.hip
    return BlockPlan(
        hi=hi, hiq=hiq, one_w=one_w, one_s=one_s, qkv_w=qkv_w, qkv_b=bp, qkv_gs=gs, anc_w=anc_w, anc_b=bap, anc_gs=anc_gs,
        proj_w=proj_w, proj_b=_padv(a.proj.bias, CP, dev), n1_g=_padv(blk.norm1.weight, CP, dev), n1_b=_padv(blk.norm1.bias, CP, dev),
        fc1_w=fc1_w, fc1_b=_padv(blk.mlp.fc1.bias, HP, dev), fc2_w=fc2_w, fc2_b=_padv(blk.mlp.fc2.bias, CP, dev),
        n2_g=_padv(blk.norm2.weight, CP, dev), n2_b=_padv(blk.norm2.bias, CP, dev),
        tab_w=tab_w, tab_a2w=tab_a2w, tab_w2a=tab_w2a, tr_w=tr_w, tr_a2w=tr_a2w, tr_w2a=tr_w2a,
        floor_w=tables.lazy_floor(sc_w), floor_a2w=tables.lazy_floor(sc_1), floor_w2a=tables.lazy_floor(sc_2),
        ceil_w=tables.lazy_ceil(sc_w, tab_w), ceil_a2w=tables.lazy_ceil(sc_1, tab_a2w), ceil_w2a=tables.lazy_ceil(sc_2, tab_w2a),
        **opt,
    )


def high_cab_fp16(model) -> bool:
    """In a `high` that `auto` chose for a Base-width model (deblur / denoise at checkpoint-like scales) the two CAB convolutions
    stay on fp16 operands with the fast path's kernels: emulated per operand on the clamp-scale deblur fixture
    (tools/precision_sites.py only ...) they are the least sensitive sites of the net -- conv1 3.4e-4 / 2.5e-4 (weights /
    input alone), conv2 1.9e-4 / 2.3e-4, against 1e-3 for the stage conv's weights alone -- and on split operands they were 41
    of a 188 ms forward.  An explicit precision='high' (and GRL-Tiny) keeps every contraction split.  GRL_HIGH_CAB=split|fp16."""
    mode = SW.text("GRL_HIGH_CAB")
    if mode in ("split", "fp16"):
        return mode == "fp16"
    return model._precision_arg == "auto" and model.embed_dim >= 160


def resolve_precision(model) -> str:
    """precision='auto' for the weights the module holds NOW (called when a plan is built, i.e. after every weight change).
    GRL-Tiny: high.  The narrow / same-resolution models (GRL-Small, anything without the smoothing upsampler tail: denoise,
    deblur) hold the 1e-3 bar on fp16 operands only at random-init logit scales (7.2e-4 / 8.2e-4); with checkpoint-like
    scales the round-4 clamp-scale fixtures measure 2.5e-3 (Base deblur) and worse (Small), against 5.9e-4 in the `high` chosen here
    (5.0e-5 with every contraction split, high_cab_fp16) -- the
    cosine logits are multiplied by up to 100 and these nets have no tail that averages the error out.  So above
    GRL_NARROW_HIGH_SCALE (25: random init draws 5 .. 20) they run on split operands throughout.  GRL-Base SR stays fast at
    every scale (blocks above GRL_HIQ_SCALE take the split-operand q / k / anchor projection: 8.1e-4 at the clamp)."""
    if model._precision_arg != "auto":
        return model._precision_arg
    if model.embed_dim < 100:
        return "high"
    if model._narrow:
        smax = 0.0
        for layer in model.layers:
            for blk in layer.blocks:
                a = blk.attn
                for t in (a.window_attn.attn_transform, a.stripe_attn.attn_transform1, a.stripe_attn.attn_transform2):
                    smax = max(smax, float(tables.clamped_scale(t.logit_scale).max()))
        calibrate, high_scale = SW.on("GRL_CALIBRATE"), SW.num("GRL_NARROW_HIGH_SCALE")
        if smax <= high_scale and model.window_size[0] <= 8:
            # 8x8 windows (the demosaicking geometry): fp16 operands miss the 1e-3 bar even at random-init scales (GRL-Small
            # 1.07e-3 against 7.1e-4 at the 16x16 denoising geometry), so the blocks are chosen by measurement here as well
            if calibrate:
                model._calibrate_narrow = True
        elif smax > high_scale:
            # round 6: not `high` throughout any more -- the blocks are chosen by measurement (calibrated_plan), everything split
            # only if the probe asks for it; GRL_CALIBRATE=0 restores the blanket rule
            if not calibrate:
                return "high"
            model._calibrate_narrow = True
    return "fast"


def build_plan(model, x_size, dev, precision: str, cab_split: Optional[bool] = None, allow_hiq: bool = True) -> Plan:
    """Packed weights / tables of the whole network for one input size, every block in ``precision`` ('fast' | 'high').
    ``allow_hiq=False``: no block takes the split-operand q / k / anchor projection (plain fp16 operands everywhere)."""
    hi = precision == "high"
    sp = 3 if hi else 1
    CP = _pad32(model.embed_dim)
    sched = block_schedule(model.depths, model.num_heads_window, model.num_heads_stripe, model.window_size,
                           model.stripe_size, model.stripe_groups, model.stripe_shift, model.df, x_size)
    # fast mode: convolutions named in GRL_SPLIT_SITES (stage_conv, after, last) still run on split operands -- per-site
    # precision for the models whose fast-mode error sits at the 1e-3 limit (tools/precision_sites.py)
    sites = _split_sites(SW.text("GRL_SPLIT_SITES", default=model.split_sites))
    xs = {k: (3 if hi else sites.get(k, 1)) for k in ("stage_conv", "after", "last")}

    def pconv(conv, cin_pad, cout_pad, r=0, cg=0, site=None):
        return (ops.pack_conv_weight(conv.weight.to(dev), cin_pad, cout_pad, r, cg, split=xs.get(site, sp)),
                ops.pack_conv_bias(conv.bias.to(dev), cout_pad, r, cg))

    with torch.no_grad():
        stages = []
        for si, stage in enumerate(model.layers):
            blocks = [pack_block(model, blk, sched[si][bi], dev, hi, cab_split, allow_hiq) for bi, blk in enumerate(stage.blocks)]
            cw, cb = pconv(stage.conv, CP, CP, site="stage_conv")
            stages.append(StagePlan(blocks=blocks, conv_w=cw, conv_b=cb))
        plan = Plan(
            sched=sched, stages=stages, split=sp, xs=xs,
            ns_g=_padv(model.norm_start.weight, CP, dev), ns_b=_padv(model.norm_start.bias, CP, dev),
            ne_g=_padv(model.norm_end.weight, CP, dev), ne_b=_padv(model.norm_end.bias, CP, dev),
            # conv_first always runs on split operands: K = 27, the cost is nil, and its operand rounding alone is 4e-4 of the
            # 1e-3 budget of a clamp-scale checkpoint (tools/precision_sites.py base_sr4_ckpt_256_hiscale)
            first=(ops.pack_conv_weight(model.conv_first.weight.to(dev), _pad32(model.in_channels), CP, split=3),
                   ops.pack_conv_bias(model.conv_first.bias.to(dev), CP)),
            after=pconv(model.conv_after_body, CP, CP, site="after"),
        )
        out_p = (model.out_channels + 15) // 16 * 16
        if model.upsampler == "pixelshuffle":
            plan.cbu = pconv(model.conv_before_upsample[0], CP, 64)
            r = 3 if model.upscale == 3 else 2
            plan.ups = [pconv(m, 64, (64 * r * r + 15) // 16 * 16, r, 64) for m in model.upsample.up if isinstance(m, nn.Conv2d)]
            plan.ups_r = r
            plan.last = pconv(model.conv_last, 64, out_p)
        elif model.upsampler == "pixelshuffledirect":
            r = model.upscale
            cg = (model.out_channels + 3) // 4 * 4
            plan.upd = pconv(model.upsample.up[0], CP, (cg * r * r + 15) // 16 * 16, r, cg)
            plan.upd_cg = cg
        elif model.upsampler == "nearest+conv":
            plan.cbu = pconv(model.conv_before_upsample[0], CP, 64)
            plan.up1, plan.up2 = pconv(model.conv_up1, 64, 64), pconv(model.conv_up2, 64, 64)
            plan.hr, plan.last = pconv(model.conv_hr, 64, 64), pconv(model.conv_last, 64, out_p)
        else:
            plan.last = pconv(model.conv_last, CP, out_p, site="last")
    return plan


# ---- precision `auto` for the wide SR models at checkpoint-like logit scales: chosen block by block, by measurement ----------
def probe_input(model, H: int, W: int, dev):
    """A fixed smooth probe image in [0, 1]: box-blurred uniform noise at the output resolution, down-sampled by the model's
    scale (the statistics of a low-quality SR input: SURVEY 8(d)'s synthetic recipe, own seed).  How far fp16 operands move the
    output depends on the input as well as on the weights -- on a high-contrast probe (coarse random blobs + fine noise) a
    clamp-scale random-weight network is 50x more sensitive than on smooth ones -- so the probe has to look like what the
    network restores."""
    g = torch.Generator().manual_seed(20240607)
    s = max(int(model.upscale), 1) if model.upsampler else 1
    hr = F.avg_pool2d(torch.rand(1, model.in_channels, H * s + 4, W * s + 4, generator=g), 5, 1)
    x = F.avg_pool2d(hr, s) if s > 1 else hr
    if not model.upsampler:                # same-resolution tasks: the input may be a NOISY image (denoising, sigma 25 / 255:
        x = x + (25.0 / 255.0) * torch.randn(x.shape, generator=g)    # data/datasets/restoration_dn.py:126-144) -- the harder case
    return x.contiguous().to(dev)


def calibrated_plan(model, x_size, dev, force: bool = False) -> Plan:
    """GRL-Base SR on fp16 operands sits AT the 1e-3 parity bar when the logit scales are checkpoint-like (clamped at 100), weight
    set by weight set: 7.7e-4 / 5.9e-4 / 1.9e-3 on three draws (round 5, float64 reference), with no single site to blame (q.k
    rounding 38 % of the variance, fc1 17 %, CAB conv2 11 %, fc2 9 %).  So `auto` MEASURES the weights it holds: a fixed probe
    image runs through the all-split network (the reference here: 5e-6 from the float64 truth) and through the fp16-operand
    one; if the difference exceeds the calibration bars, blocks move to split operands -- the ones whose fp16 rounding costs
    the most first (error of the network with ONLY that block on fp16 operands) -- until the probe passes.  One-time cost per
    weight set and input size: 3 plan builds + ~(blocks + 8) probe forwards.  Bars: rms <= GRL_CAL_RMS (1.3e-4: the maximum
    over the 3 M outputs of a 256x256 tile sits 5.5-6.6 rms above zero) and max <= GRL_CAL_MAX (8.5e-4) on the probe.
    (Every plan is built through the module global ``build_plan``, so a caller that wraps it sees each build.)"""
    fast = build_plan(model, x_size, dev, "fast")
    blocks = [(si, bi) for si, st in enumerate(fast.stages) for bi in range(len(st.blocks))]
    info = dict(blocks=len(blocks), split=0)
    model.calibration = info
    n_hiq = sum(fast.stages[si].blocks[bi].hiq for si, bi in blocks)
    if not force and not n_hiq:
        return fast                       # random-init-like scales: fp16 operands hold 2e-4 (fixtures); nothing to measure
    bar_rms = SW.num("GRL_CAL_RMS")
    bar_max = SW.num("GRL_CAL_MAX")
    H, W = x_size
    # the probe is a crop when the image is large and the block geometry does not depend on the image size
    ph, pw = min(H, 256 // model.pad_size * model.pad_size or model.pad_size), min(W, 256 // model.pad_size * model.pad_size or model.pad_size)
    if (ph, pw) != (H, W):
        small = block_schedule(model.depths, model.num_heads_window, model.num_heads_stripe, model.window_size, model.stripe_size,
                               model.stripe_groups, model.stripe_shift, model.df, (ph, pw))
        if small != fast.sched:
            ph, pw = H, W
    x = probe_input(model, ph, pw, dev)
    with torch.no_grad():
        ref_plan = build_plan(model, x_size, dev, "high", cab_split=True)
        y_ref = model._forward_eager(x, ref_plan).double()
        del ref_plan
        hi_plan = build_plan(model, x_size, dev, "high")       # its BLOCKS are what a split block runs (CAB as high_cab_fp16 says)

        def mixed(split_set):
            return dataclasses.replace(fast, stages=[
                dataclasses.replace(st, blocks=[(hi_plan if (si, bi) in split_set else fast).stages[si].blocks[bi]
                                                for bi in range(len(st.blocks))]) for si, st in enumerate(fast.stages)])

        def err(plan):
            d = model._forward_eager(x, plan).double() - y_ref
            return float(d.abs().max()), float(d.pow(2).mean().sqrt())

        ok = lambda e: e[0] <= bar_max and e[1] <= bar_rms
        info.update(bar_max=bar_max, bar_rms=bar_rms, probe=(ph, pw), qkv_split_blocks=n_hiq)
        if n_hiq:
            # cheapest first: plain fp16 operands in EVERY projection (the split q / k / anchor projection of blocks above
            # hiq_scale costs 206 against 150 us per 4 tiles and block) -- kept only where the measurement asks for it
            plain = build_plan(model, x_size, dev, "fast", allow_hiq=False)
            e_plain = err(plain)
            info.update(plain_max=e_plain[0], plain_rms=e_plain[1])
            if ok(e_plain):
                info.update(probe_max=e_plain[0], probe_rms=e_plain[1], qkv_split_blocks=0)
                return plain
            del plain
        e_fast = err(fast)
        info.update(fast_max=e_fast[0], fast_rms=e_fast[1])
        if ok(e_fast):
            info.update(probe_max=e_fast[0], probe_rms=e_fast[1])
            return fast
        every = frozenset(blocks)
        e_all = err(mixed(every))
        info.update(all_split_max=e_all[0], all_split_rms=e_all[1])
        if not ok(e_all):                 # the fp16 convolutions around the blocks alone exceed the bars: everything split
            model.precision = "high"
            info.update(split=len(blocks), probe_max=0.0, probe_rms=0.0, everything=True)
            return build_plan(model, x_size, dev, "high", cab_split=True)
        # cost of each block's fp16 operands: the network with ONLY that block fast
        var = {b: max(err(mixed(every - {b}))[1] ** 2 - e_all[1] ** 2, 0.0) for b in blocks}
        order = sorted(blocks, key=lambda b: -var[b])
        # predicted number of blocks (variances add), then verified by measurement and raised until the probe passes
        k = predicted_split_count([var[b] for b in order], e_all[1] ** 2, bar_rms)
        while True:
            e = err(mixed(frozenset(order[:k])))
            if ok(e) or k >= len(order):
                break
            k = min(len(order), k + max(1, len(order) // 16))
        info.update(split=k, probe_max=e[0], probe_rms=e[1], split_blocks=sorted(order[:k]))
        model.precision = f"mixed({k}/{len(order)} blocks split)"
        plan = mixed(frozenset(order[:k]))
    return plan
