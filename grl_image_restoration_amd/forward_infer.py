"""The inference launch sequence of ``GRL`` (grl.py:506-551) over a packed plan (plan.py): which HIP kernel runs where.

Every function takes the model as its first argument.  Which route a block takes is read off its ``BlockPlan``: an optional field
that is packed (``is not None``) selects the kernel that consumes it, and the rest is decided from the shape.  No environment switch chooses a kernel here.
"""
import torch

from . import _lib as L
from . import ops
from . import switches as SW
from .geometry import BlockGeo
from .plan import BlockPlan, Plan


def cab(model, r, pk: BlockPlan, B, H, W, CP):
    """CAB branch (mixed_attn_block.py:948-983): returns the un-gated conv output and the per-image squeeze-excite
    gate; the gate is applied inside the proj+norm1 epilogue.  fast: fp16 intermediates; high: fp32 + split operands."""
    hi = pk.hi_c
    sp, dt = (3, torch.float32) if hi else (1, ops.GEMM_DTYPE)
    mid = ops.empty(B * H * W, pk.cab_mid, dtype=dt, device=r.device)  # fast: pad channels zero-filled by the conv store
    ops.conv3x3(r, pk.cab0_w, pk.cab0_b, B, H, W, act=1, out=mid, x_split=pk.cab0_split)
    # (The squeeze-excite gate stays a launch of its own.  Folding it into the conv2 launch, the gate by the last workgroup of each
    # image, measured SLOWER in the two-stream bench, 88.1 against 82.6 ms/step: the serial tail of one workgroup per image holds the
    # whole launch, while the separate 10-us se_kernel hides behind the other tile group's kernels.)
    if pk.cab2_blob is not None:
        raw, pool = ops.cab_conv2(mid, pk.cab2_blob, pk.cab2_bias, B, H, W)
    else:
        raw, pool = ops.conv3x3(mid, pk.cab2_w, pk.cab2_b, B, H, W, want_pool=True, out_dtype=dt, x_split=sp)
    gate = ops.se_scale(pool, B, CP, model.embed_dim, H * W, pk.se1_w, pk.se1_b, pk.se3_w, pk.se3_b)
    return raw, gate


def attention(model, qkv, anc, att, pk: BlockPlan, geo: BlockGeo, B, H, W, lse=None, qkv_lo=None, anc_lo=None):
    """The three attention launches of a block on head planes: window (efficient.py:128-165), anchors -> stripe tokens
    and stripe tokens -> anchors (:215-270).  ``att``: [M, (nh_w+nh_s)*32] output (fp16 or fp32).  ``qkv_lo`` / ``anc_lo``:
    rounding-residual twins of the planes (precision 'high': split-precision attention operands)."""
    C = model.embed_dim
    nh_w, nh_s = geo.nh_w, geo.nh_s
    d_w, d_s = C // 2 // nh_w, C // 2 // nh_s
    g_w, g_s, g_an = geo.grids(H, W)
    y = ops.empty(nh_s, B * g_an[0] * g_an[1], 32, dtype=ops.PLANE_DTYPE, device=att.device)
    split = qkv_lo is not None
    y_lo = ops.empty_like(y) if split else None

    TG = ops.TokenGrid
    ls = lse if lse is not None else (None, None, None)
    tr = lambda flag, *gs: tuple(g.T() for g in gs) if flag else gs    # transposed view where the plan chose it
    ops.attention(
        *tr(pk.tr_w, TG(qkv, 0, *g_w), TG(qkv, nh_w, *g_w), TG(qkv, 2 * nh_w, *g_w), TG(att, 0, *g_w)),
        B=B, nh=nh_w, table=pk.tab_w, masked=geo.window_shift > 0,
        ones_col=d_w if d_w < 32 else -1, head_dim=d_w, k_one31=pk.one_w, lazy_floor=pk.floor_w, lse=ls[0], lazy_ceil=pk.ceil_w,
        q_lo=qkv_lo, k_lo=qkv_lo, v_lo=qkv_lo,
    )
    s0 = 3 * nh_w
    g_q = TG(qkv, s0, *g_s)
    g_k = TG(qkv, s0 + nh_s, *g_s)
    g_v = TG(qkv, s0 + 2 * nh_s, *g_s)
    g_a = TG(anc, 0, *g_an)
    g_y = TG(y, 0, *g_an)
    oc = d_s if d_s < 32 else -1
    ops.attention(*tr(pk.tr_a2w, g_a, g_k, g_v, g_y), B=B, nh=nh_s, table=pk.tab_a2w, masked=geo.stripe_shift,
                  ones_col=oc, head_dim=d_s, k_one31=pk.one_s, lazy_floor=pk.floor_a2w, lse=ls[1], lazy_ceil=pk.ceil_a2w,
                  q_lo=anc_lo, k_lo=qkv_lo, v_lo=qkv_lo, o_lo=y_lo)
    ops.attention(*tr(pk.tr_w2a, g_q, g_a, g_y, TG(att, nh_w, *g_s)), B=B, nh=nh_s, table=pk.tab_w2a,
                  masked=geo.stripe_shift, ones_col=oc, head_dim=d_s, k_one31=pk.one_s,
                  lazy_floor=pk.floor_w2a, lse=ls[2], q_lo=qkv_lo, k_lo=anc_lo, v_lo=y_lo, lazy_ceil=pk.ceil_w2a)
    return y


def block(model, r, pk: BlockPlan, geo: BlockGeo, B, H, W):
    C, CP = model.embed_dim, r.shape[1]
    M = B * H * W
    nh_w, nh_s, df = geo.nh_w, geo.nh_s, geo.df
    dev = r.device
    if pk.hi:
        return block_high(model, r, pk, geo, B, H, W)
    # q/k/v, anchors and the anchor-side values live as head planes [slot][token][32]: a key tile of 32
    # consecutive tokens is 2 KB contiguous for the attention kernel's staging loads
    one_pass = pk.qa_blob is not None and df == 2 and H % 2 == 0 and W % 64 == 0
    if pk.hiq and one_pass and pk.qa_lo is not None:
        qkv, anc = ops.qkv_anchor(r, pk.qa_blob, pk.qa_slots[0], pk.qa_slots[1], B, H, W, lo_blob=pk.qa_lo)
    elif pk.hiq:
        qkv = ops.linear(r, pk.qkv_w3, pk.qkv_b, epi=L.EPI_GROUPNORM, gscale=pk.qkv_gs, planes=True, a_split=3, w_regs=pk.qkv_w3r)
        anc = ops.linear(r, pk.anc_w3, pk.anc_b, epi=L.EPI_GROUPNORM, gscale=pk.anc_gs, pool=(df, H, W), planes=True, a_split=3)
    elif one_pass:
        qkv, anc = ops.qkv_anchor(r, pk.qa_blob, pk.qa_slots[0], pk.qa_slots[1], B, H, W)
    else:
        if pk.qkv_blob is not None:
            qkv = ops.qkv(r, pk.qkv_blob, pk.qkv_slots)
        else:
            qkv = ops.linear(r, pk.qkv_w, pk.qkv_b, epi=L.EPI_GROUPNORM, gscale=pk.qkv_gs, planes=True)
        anc = ops.linear(r, pk.anc_w, pk.anc_b, epi=L.EPI_GROUPNORM, gscale=pk.anc_gs, pool=(df, H, W), planes=True)
    att = ops.empty(M, (nh_w + nh_s) * 32, dtype=ops.GEMM_DTYPE, device=dev)  # operand of the proj GEMM
    attention(model, qkv, anc, att, pk, geo, B, H, W)
    cab_, gate = cab(model, r, pk, B, H, W, CP) if model.local_connection else (None, None)
    if pk.proj_blob is not None and pk.mlp_blob is not None and H * W >= 128:
        return ops.block_tail(att, r, cab_, gate, H * W, pk.proj_blob, pk.proj_b, pk.n1_g, pk.n1_b, pk.mlp_blob,
                              pk.fc2_b, pk.n2_g, pk.n2_b, Hpad=pk.mlp_hp, n_real=C, res_scale=model.res_scale,
                              rblob=pk.tail_rblob)
    # x = x + res_scale * norm1(proj(attn)) + cab(x)   (efficient.py:543-548)
    r1 = ops.linear(att, pk.proj_w, pk.proj_b, epi=L.EPI_LN_RES, out_dtype=torch.float32, ln_g=pk.n1_g,
                    ln_b=pk.n1_b, n_real=C, res_scale=model.res_scale, resid=r, add2=cab_, add2_scale=gate,
                    rows_per_image=H * W)
    # x = x + res_scale * norm2(mlp(x))                 (efficient.py:554)
    if pk.mlp_blob is not None:
        return ops.mlp(r1, pk.mlp_blob, pk.fc2_b, pk.n2_g, pk.n2_b, Hpad=pk.mlp_hp, n_real=C,
                       res_scale=model.res_scale)
    h = ops.linear(r1, pk.fc1_w, pk.fc1_b, epi=L.EPI_GELU)
    return ops.linear(h, pk.fc2_w, pk.fc2_b, epi=L.EPI_LN_RES, out_dtype=torch.float32, ln_g=pk.n2_g,
                      ln_b=pk.n2_b, n_real=C, res_scale=model.res_scale, resid=r1)


def block_high(model, r, pk: BlockPlan, geo: BlockGeo, B, H, W):
    """precision='high': every linear / conv contraction on split operands (activation hi+lo staged in-kernel from fp32,
    weights packed hi|hi|lo), fp32 intermediates, the row norms as separate launches; attention on hi + lo operand planes
    (3 QK^T terms, 2 PV terms in the generic kernel) with an fp32 output."""
    C, CP = model.embed_dim, r.shape[1]
    M = B * H * W
    f32 = torch.float32
    G = pk.qkv_w.shape[0] // 32
    Ma = M // (geo.df * geo.df)
    qkv_lo = ops.empty(G, M, 32, dtype=ops.PLANE_DTYPE, device=r.device)
    anc_lo = ops.empty(geo.nh_s, Ma, 32, dtype=ops.PLANE_DTYPE, device=r.device)
    qkv = ops.linear(r, pk.qkv_w, pk.qkv_b, epi=L.EPI_GROUPNORM, gscale=pk.qkv_gs, planes=True, a_split=3, out_lo=qkv_lo, w_regs=pk.qkv_wr)
    if pk.anc_wr is not None and Ma % 32 == 0:
        # AnchorLinear's avg-pool (mixed_attn_block.py:727-736) as a reduction of its own, then the weights-stationary kernel on
        # the M / df^2 pooled rows (the generic kernel with the pool fused into its A load: 440 us of a 384x384 x4 deblur block)
        pooled = r.view(B, H // geo.df, geo.df, W // geo.df, geo.df, CP).mean(dim=(2, 4)).view(Ma, CP)
        anc = ops.linear(pooled, pk.anc_w, pk.anc_b, epi=L.EPI_GROUPNORM, gscale=pk.anc_gs, planes=True, a_split=3,
                         out_lo=anc_lo, w_regs=pk.anc_wr)
    else:
        anc = ops.linear(r, pk.anc_w, pk.anc_b, epi=L.EPI_GROUPNORM, gscale=pk.anc_gs, pool=(geo.df, H, W), planes=True,
                         a_split=3, out_lo=anc_lo)
    att = ops.empty(M, (geo.nh_w + geo.nh_s) * 32, dtype=f32, device=r.device)
    # attention on split operands too: q, k, v (and the anchor-side values) as fp16 hi + lo planes -> generic kernel
    attention(model, qkv, anc, att, pk, geo, B, H, W, qkv_lo=qkv_lo, anc_lo=anc_lo)
    cab_, gate = cab(model, r, pk, B, H, W, CP) if model.local_connection else (None, None)
    # norm + residual (+ gated CAB branch) in the epilogue of the weights-stationary kernel where it takes the shape (a row of
    # <= 192 channels is one slab): the fp32 products p1 / p2 never reach memory
    fuse = CP <= 192 and M % 32 == 0 and (H * W) % 32 == 0 and pk.proj_wr is not None and pk.fc2_wr is not None
    if fuse:
        r1 = ops.linear(att, pk.proj_w, pk.proj_b, epi=L.EPI_LN_RES, out_dtype=f32, a_split=3, w_regs=pk.proj_wr,
                        ln_g=pk.n1_g, ln_b=pk.n1_b, n_real=C, res_scale=model.res_scale, resid=r, add2=cab_, add2_scale=gate,
                        rows_per_image=H * W)
    else:
        p1 = ops.linear(att, pk.proj_w, pk.proj_b, out_dtype=f32, a_split=3, w_regs=pk.proj_wr)
        r1 = ops.layernorm_res(p1, r, pk.n1_g, pk.n1_b, C, res_scale=model.res_scale, add2=cab_, add2_scale=gate,
                               rows_per_image=H * W)
    h = ops.linear(r1, pk.fc1_w, pk.fc1_b, epi=L.EPI_GELU, out_dtype=f32, a_split=3, w_regs=pk.fc1_wr)
    if fuse:
        return ops.linear(h, pk.fc2_w, pk.fc2_b, epi=L.EPI_LN_RES, out_dtype=f32, a_split=3, w_regs=pk.fc2_wr,
                          ln_g=pk.n2_g, ln_b=pk.n2_b, n_real=C, res_scale=model.res_scale, resid=r1)
    p2 = ops.linear(h, pk.fc2_w, pk.fc2_b, out_dtype=f32, a_split=3, w_regs=pk.fc2_wr)
    return ops.layernorm_res(p2, r1, pk.n2_g, pk.n2_b, C, res_scale=model.res_scale)


def forward_features(model, f, plan: Plan, B, H, W):
    """grl.py:491-504 on the token matrix f [B*H*W, CP] (fp32) -> [B*H*W, CP]."""
    C = model.embed_dim
    t = ops.layernorm(f, plan.ns_g, plan.ns_b, C)
    n = model.stream_groups(B)
    if n > 1:
        return features_streams(model, t, plan, B, H, W, n)
    check = SW.on("GRL_CHECK_RANGE")                        # debug: largest residual-stream magnitude per block (fp16 operand
    for si, st in enumerate(plan.stages):                   # staging saturates at 65504; this reports how close a checkpoint gets)
        r = t
        for bi, pk in enumerate(st.blocks):
            r = block(model, r, pk, plan.sched[si][bi], B, H, W)
            if check:
                print(f"GRL_CHECK_RANGE layers.{si}.blocks.{bi}: max|x| = {r.abs().max().item():.4g}  (fp16 operand limit 65504)")
        # TransformerStage.forward (grl.py:164-170): conv3x3 + residual
        t = ops.conv3x3(r, st.conv_w, st.conv_b, B, H, W, resid=t, x_split=plan.xs["stage_conv"])
    return ops.layernorm(t, plan.ne_g, plan.ne_b, C)


def features_streams(model, t, plan: Plan, B, H, W, n):
    """The tile batch is cut into n groups that advance block by block on n HIP streams: tiles are independent,
    and the HBM-bound linear kernels of one group overlap the MFMA-bound attention of another."""
    dev = t.device
    main = torch.cuda.current_stream(dev)
    pool = getattr(model, "_streams", None)
    if pool is None or len(pool) < n or pool[0].device != dev:
        pool = model._streams = [torch.cuda.Stream(dev) for _ in range(n)]
    Bg = B // n
    Mg = t.shape[0] // n
    parts = [t[g * Mg : (g + 1) * Mg] for g in range(n)]
    for g in range(n):
        pool[g].wait_stream(main)
    for si, st in enumerate(plan.stages):
        r = list(parts)
        for bi, pk in enumerate(st.blocks):
            for g in range(n):
                with torch.cuda.stream(pool[g]):
                    r[g] = block(model, r[g], pk, plan.sched[si][bi], Bg, H, W)
        for g in range(n):
            with torch.cuda.stream(pool[g]):
                parts[g] = ops.conv3x3(r[g], st.conv_w, st.conv_b, Bg, H, W, resid=parts[g], x_split=plan.xs["stage_conv"])
    out = ops.empty_like(t)
    for g in range(n):
        with torch.cuda.stream(pool[g]):
            ops.layernorm(parts[g], plan.ne_g, plan.ne_b, model.embed_dim, out=out[g * Mg : (g + 1) * Mg])
        main.wait_stream(pool[g])
    return out


def _tokens(x, cpad):
    """(B, C, H, W) -> channels-last token matrix [B*H*W, cpad] (zero padded)."""
    B, C, H, W = x.shape
    t = torch.zeros(B * H * W, cpad, dtype=torch.float32, device=x.device)
    t[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    return t


def _image(t, B, H, W, C):
    return t.view(B, H, W, -1)[..., :C].permute(0, 3, 1, 2)


def forward(model, x, plan: Plan):
    """conv_first, the body and the reconstruction tail on the padded, mean-free image ``x`` [B, Cin, H, W] -> the output image, still
    padded and in the network's range (GRL._forward_eager undoes both)."""
    B, _, H, W = x.shape
    s, oc = model.upscale, model.out_channels
    sp = plan.split

    def conv(*a, **kw):
        return ops.conv3x3(*a, x_split=sp, **kw)

    # fast: 16-bit intermediates of the tail feed fp16-operand convolutions; high: fp32 + split operands
    bf = torch.float32 if sp == 3 else ops.GEMM_DTYPE

    f = ops.conv3x3(_tokens(x, plan.first[0].shape[2] // 3), *plan.first, B, H, W, x_split=3)   # conv_first
    body = ops.conv3x3(forward_features(model, f, plan, B, H, W), *plan.after, B, H, W, resid=f, x_split=plan.xs["after"])  # conv_after_body + f
    if model.upsampler == "pixelshuffle":
        y = conv(body, *plan.cbu, B, H, W, act=2, slope=0.01, out_dtype=bf)
        h, w, r = H, W, plan.ups_r
        for wt, bs in plan.ups:
            y = conv(y, wt, bs, B, h, w, out_dtype=bf, shuffle_r=r, shuffle_cg=64)         # conv + PixelShuffle
            h, w = h * r, w * r
        y = _image(conv(y, *plan.last, B, h, w), B, h, w, oc)
    elif model.upsampler == "pixelshuffledirect":
        y = conv(body, *plan.upd, B, H, W, shuffle_r=s, shuffle_cg=plan.upd_cg)
        y = _image(y, B, H * s, W * s, oc)
    elif model.upsampler == "nearest+conv":
        y = conv(body, *plan.cbu, B, H, W, act=2, slope=0.01, out_dtype=bf)

        def up2(t, h, w):  # nearest x2 on a token matrix
            return t.view(B, h, 1, w, 1, -1).expand(B, h, 2, w, 2, t.shape[1]).reshape(B * 4 * h * w, -1)

        y = conv(up2(y, H, W), *plan.up1, B, 2 * H, 2 * W, act=2, slope=0.2, out_dtype=bf)
        y = conv(up2(y, 2 * H, 2 * W), *plan.up2, B, 4 * H, 4 * W, act=2, slope=0.2, out_dtype=bf)
        y = conv(y, *plan.hr, B, 4 * H, 4 * W, act=2, slope=0.2, out_dtype=bf)
        y = _image(conv(y, *plan.last, B, 4 * H, 4 * W), B, 4 * H, 4 * W, oc)
    else:
        y = _image(ops.conv3x3(body, *plan.last, B, H, W, x_split=plan.xs["last"]), B, H, W, oc)
        if model.in_channels == model.out_channels:
            y = x + y
    return y
