"""The VGG19 perceptual loss of the real-world SR GAN stage (config/loss/gan_training_loss.yaml: features before ReLU at conv1_2,
conv2_2, conv3_4, conv4_4, conv5_4 with weights 0.1 / 0.1 / 1 / 1 / 1, L1 per layer, weight 1).

  replaces  VGGFeatureExtractor (vgg19, no batch norm)     models/aux_archs/vgg.py:154-268
            PerceptualLoss at style_weight = 0             losses/losses.py:59-172
            PerceptualLoss with the style loss             losses/losses.py:147-187   (PerceptualStyleLoss)

CUDA tensors: ONE ``torch.autograd.Function``.  The forward runs the restored image and the target through the frozen VGG as one
batch of 2B -- sixteen ``grl_conv3x3_fwd`` launches on filter banks packed once when the weights are loaded, ReLU in the epilogue of
the eleven untapped layers (act = 2, slope = 0; 16-bit output, which is what the next loader contracts anyway), and per tapped
layer one ``grl_vgg_tap_fwd`` (csrc/vgg.hip): the L1 term into the loss scalar in a fixed order plus ReLU + 2 x 2 max pool of both
halves.  The backward runs the chain in reverse by hand for the restored half alone: ``grl_vgg_tap_bwd`` at the taps, the ReLU mask
``y > 0`` on the saved activated output elsewhere (as autograd._lrelu_grad), sixteen data-gradient launches of ``grl_conv3x3_fwd``
on the flipped banks, ``grl_vgg_prep_bwd`` at the end.  No weight gradient is ever formed, the target has no backward, and the
gradients travel under the chain's OWN power-of-two operand scale S (``operand_scale``): |dL/df| at a tap is exactly the layer's
coefficient, ~1e-8 at the workload's shapes and below fp16's smallest subnormal, so S is fixed from the coefficients before the first
launch, every gradient of the chain is carried as S * g in fp32 (the launches get x_scale = out_scale = 1), and
``grl_vgg_prep_bwd`` divides S out again.  The device-wide scale of autograd.GradScaleTop belongs to other networks' passes and is
not read here.  A missing kernel is an error; there is no fallback to eager torch.

CPU tensors: ``composite`` -- plain differentiable torch in float64, the yardstick of the tests (``operand_dtype=torch.float16``
emulates the kernels' operand rounding; ``decisions`` replaces the ReLU masks, pool indices and L1 signs by given ones, because the
derivative jumps wherever one of them flips and gradients of two arithmetics compare only under the same decisions).

The style loss (``style_weight > 0``) is ``PerceptualStyleLoss`` below (csrc/gram.hip); ``PerceptualLoss`` itself keeps refusing it.
Not built: the ``l2`` / ``fro`` criteria raise NotImplementedError (the reference's own ``l2`` branch cannot be constructed: it names
``torch.nn.L2loss``).  On CUDA a tap must be a ``convN_M`` layer that closes its block
(or the last layer borrowed) -- the yaml's five are, and so is a single ``conv5_4``: an untapped block-closing convolution goes
through the tap kernel with coefficient 0 for its ReLU + pool; ``relu`` / ``pool`` taps and mid-block taps work on the CPU
composite only.
"""
import math
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import nn

_BLOCKS = (2, 2, 4, 4, 4)                       # convolutions per block of vgg19 (models/aux_archs/vgg.py: NAMES["vgg19"])
_WIDTHS = (64, 128, 256, 512, 512)
NAMES: List[str] = []                            # position in this list == index in torchvision's vgg19().features
for _b, _n in enumerate(_BLOCKS, 1):
    for _j in range(1, _n + 1):
        NAMES += [f"conv{_b}_{_j}", f"relu{_b}_{_j}"]
    NAMES.append(f"pool{_b}")
CONV_INDEX = {n: i for i, n in enumerate(NAMES) if n.startswith("conv")}     # conv1_1: 0 ... conv5_4: 34
GAN_LAYER_WEIGHTS = {"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1.0, "conv4_4": 1.0, "conv5_4": 1.0}   # gan_training_loss.yaml
MIN_SIDE = 16                                    # four pools: below 16 nothing is left for block 5


def layer_names(blocks: Sequence[int]) -> List[str]:
    """The NAMES list of a VGG with ``blocks`` convolutions per block, positions as in torchvision's ``features`` without batch norm:
    ``layer_names(_BLOCKS) == NAMES``; (2, 2, 3, 3, 3) is vgg16 (lpips.py)."""
    names: List[str] = []
    for b, n in enumerate(blocks, 1):
        for j in range(1, n + 1):
            names += [f"conv{b}_{j}", f"relu{b}_{j}"]
        names.append(f"pool{b}")
    return names


def _conv_shapes(last_idx: int):
    """(name, features index, cin, cout) of the convolutions up to position ``last_idx`` of NAMES."""
    out, cin = [], 3
    for name, idx in CONV_INDEX.items():
        if idx > last_idx:
            break
        cout = _WIDTHS[int(name[4]) - 1]
        out.append((name, idx, cin, cout))
        cin = cout
    return out


def seeded_state_dict(seed: int, last: str = "conv5_4") -> Dict[str, torch.Tensor]:
    """A stand-in for vgg19-dcbb9e9d.pth with torchvision's keys (tests, tools): He-scaled normal draws from a seeded generator,
    biases 0.1 * normal, every value rounded to an fp16-representable one (an fp16-operand kernel sees no weight rounding).  float32."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for _, idx, cin, cout in _conv_shapes(NAMES.index(last)):
        w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        b = torch.randn(cout, generator=g) * 0.1
        sd[f"features.{idx}.weight"] = w.to(torch.float16).float()
        sd[f"features.{idx}.bias"] = b.to(torch.float16).float()
    return sd


def load_vgg19(path: str) -> Dict[str, torch.Tensor]:
    """The state dict of the user's ``vgg19-dcbb9e9d.pth`` (torchvision's keys) by ``torch.load`` alone: torchvision is not needed and
    nothing is ever downloaded."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(sd).__name__}")
    return sd


def _contract(t: torch.Tensor, operand_dtype) -> torch.Tensor:
    """The value a kernel's loader contracts (rounded to ``operand_dtype``), carried on in t's dtype; straight-through for autograd."""
    return t if operand_dtype is None else t + (t.to(operand_dtype).to(t.dtype) - t).detach()


class _EmuConv(torch.autograd.Function):
    """conv3x3 on operands rounded to ``od`` whose data gradient contracts dy rounded to ``od`` under the scale ``gs``."""

    @staticmethod
    def forward(ctx, x, w, b, od, gs):
        wc = w.to(od).to(x.dtype)
        ctx.save_for_backward(wc)
        ctx.od, ctx.gs, ctx.xshape = od, gs, x.shape
        return F.conv2d(x.to(od).to(x.dtype), wc, b, padding=1)

    @staticmethod
    def backward(ctx, dy):
        (wc,) = ctx.saved_tensors
        dyr = (dy * ctx.gs).to(ctx.od).to(dy.dtype) / ctx.gs
        return torch.nn.grad.conv2d_input(ctx.xshape, wc, dyr, padding=1), None, None, None, None


class VGG19Features(nn.Module):
    """The reference's VGGFeatureExtractor for ``vgg19``: ``forward(x)`` returns {layer name: feature [B, C, h, w]} for
    ``layer_name_list``; convolution features are taken BEFORE the ReLU that follows.  Only the layers up to the last requested one
    are borrowed.  ``state_dict``: torchvision's keys ``features.{0,2,5,...,34}.{weight,bias}`` (``classifier.*`` and layers past the
    last borrowed one are ignored; a missing or misshapen key raises and names the key).  The parameters are frozen."""

    def __init__(self, layer_name_list: Sequence[str], state_dict: Dict[str, torch.Tensor], use_input_norm: bool = True,
                 range_norm: bool = False):
        super().__init__()
        self.layer_name_list = list(layer_name_list)
        if not self.layer_name_list:
            raise ValueError("VGG19Features: layer_name_list is empty")
        for v in self.layer_name_list:
            if v not in NAMES:
                raise ValueError(f"VGG19Features: {v!r} is not a layer of vgg19")
        self.use_input_norm, self.range_norm = bool(use_input_norm), bool(range_norm)
        self.names = NAMES[: max(NAMES.index(v) for v in self.layer_name_list) + 1]
        self.convs = _conv_shapes(len(self.names) - 1)
        self.weights, self.biases = nn.ParameterList(), nn.ParameterList()
        for _, idx, cin, cout in self.convs:
            for kind, shape, dest in (("weight", (cout, cin, 3, 3), self.weights), ("bias", (cout,), self.biases)):
                key = f"features.{idx}.{kind}"
                if key not in state_dict:
                    raise KeyError(f"VGG19 weights: key {key!r} is missing")
                t = state_dict[key]
                if tuple(t.shape) != shape:
                    raise ValueError(f"VGG19 weights: key {key!r} has shape {tuple(t.shape)}, expected {shape}")
                dest.append(nn.Parameter(t.detach().clone().float(), requires_grad=False))
        # float32 buffers, as the reference builds them (vgg.py:240-246): the nearest floats to the decimals
        self.register_buffer("mean", torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1))
        self.register_buffer("std", torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1))
        self._packs: dict = {}                   # device -> (forward banks, data-gradient banks): packed once, not per step
        self.eval()

    def _apply(self, fn, *a, **kw):
        self._packs.clear()
        return super()._apply(fn, *a, **kw)

    def _check_size(self, x: torch.Tensor) -> None:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"VGG19Features: expected [B, 3, H, W], got {tuple(x.shape)}")
        if x.shape[2] < MIN_SIDE or x.shape[3] < MIN_SIDE:
            raise ValueError(f"VGG19Features: the input must be at least {MIN_SIDE} x {MIN_SIDE} (got {x.shape[2]} x {x.shape[3]}): "
                             "four pools would leave nothing")

    # ---- CPU: the composite ---------------------------------------------------------------------------------------------------
    def composite(self, x: torch.Tensor, operand_dtype=None, decisions: Optional[dict] = None, grad_scale: Optional[float] = None,
                  trace: Optional[list] = None) -> Dict[str, torch.Tensor]:
        """Plain torch in x's dtype.  ``operand_dtype``: both operands of every convolution rounded to that type (``grad_scale``: the
        data gradients contract dy rounded to it under that scale as well).  ``decisions``: {"masks": one boolean [B, C, h, w] per
        convolution, "pool_idx": the ``max_pool2d(return_indices=True)`` indices per pool}: ReLU and the pools take these instead of
        looking at their own argument.  ``trace`` receives the pre-ReLU output of every convolution, detached."""
        self._check_size(x)
        dt = x.dtype
        if self.range_norm:
            x = (x + 1) / 2
        if self.use_input_norm:
            x = (x - self.mean.to(dt)) / self.std.to(dt)
        masks = list(decisions["masks"]) if decisions is not None else None
        pools = list(decisions["pool_idx"]) if decisions is not None else None
        out, ci, last_conv = {}, 0, -1
        for name in self.names:
            if name.startswith("conv"):
                w, b = self.weights[ci].to(dt), self.biases[ci].to(dt)
                if operand_dtype is not None and grad_scale is not None:
                    x = _EmuConv.apply(x, w, b, operand_dtype, float(grad_scale))
                else:
                    x = F.conv2d(_contract(x, operand_dtype), _contract(w, operand_dtype), b, padding=1)
                if trace is not None:
                    trace.append(x.detach())
                last_conv, ci = ci, ci + 1
            elif name.startswith("relu"):
                x = F.relu(x) if masks is None else x * masks[last_conv].to(dt)
            else:
                if pools is None:
                    x = F.max_pool2d(x, 2, 2)
                else:
                    idx = pools.pop(0)
                    x = x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
            if name in self.layer_name_list:
                out[name] = x
        return out

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        if x.is_cuda:
            return _hip_features(self, x)
        return {k: v.clone() for k, v in self.composite(x).items()}

    # ---- CUDA: what the HIP chain needs ---------------------------------------------------------------------------------------
    def _hip_plan(self):
        """[(tapped, pooled)] per convolution, for the chain of csrc/vgg.hip.  A layer that is tapped or pooled goes through the tap
        kernel (an untapped block-closing convolution with coefficient 0: it needs the kernel's ReLU + pool); raises for tap sets
        the chain does not cover."""
        for v in self.layer_name_list:
            if not v.startswith("conv"):
                raise NotImplementedError(f"the HIP perceptual chain taps convolution layers only (got {v!r}); the CPU composite takes any layer")
        plan = []
        for name, idx, _, _ in self.convs:
            pooled = idx + 2 < len(self.names) and self.names[idx + 2].startswith("pool")
            tapped = name in self.layer_name_list
            if tapped and not pooled and idx + 1 < len(self.names):
                raise NotImplementedError(f"the HIP perceptual chain taps a block's last convolution or the last layer borrowed (got {name!r})")
            plan.append((tapped, pooled))
        return plan

    def _hip_packs(self, device):
        from . import ops

        key = str(device)
        if key not in self._packs:
            fw, bw = [], []
            for (_, _, cin, cout), w, b in zip(self.convs, self.weights, self.biases):
                w, b = w.to(device), b.to(device)
                fw.append(ops.pack_conv_train(w, b, (cout + 15) // 16 * 16, (cin + 31) // 32 * 32))
                gout = (cin + 15) // 16 * 16
                bw.append((ops.pack_conv_train(w, None, gout, (cout + 31) // 32 * 32, flip_t=True)[0],
                           torch.zeros(gout, dtype=torch.float32, device=device)))
            self._packs[key] = (fw, bw)
        return self._packs[key]


def operand_scale(coefs: Sequence[float], upstream: float = 1.0) -> float:
    """The power of two S under which the perceptual backward carries its gradients: the largest tap term S * coef * |upstream|
    lands in (2^-4, 2^-3].  At a tap |dL/df| IS the coefficient, and the yaml's coefficients span a factor 320 (0.1 / 64 channels at
    full resolution against 1 / 512 channels at 1/256 of the pixels), so the smallest tap term sits near 2e-4 -- above fp16's
    smallest normal 6.1e-5 -- and sums of gradients have 2^19 of headroom to fp16's largest value."""
    kmax = max(abs(c) for c in coefs) * abs(upstream)
    if not (kmax > 0.0 and math.isfinite(kmax)):
        return 1.0
    return 2.0 ** (-3 - math.ceil(math.log2(kmax)))


def _hip_chain(vgg: VGG19Features, x: torch.Tensor, gt: Optional[torch.Tensor], coefs: Optional[Sequence[float]], trace: Optional[list] = None,
               keep: bool = True, style: Optional[dict] = None):
    """The forward launches.  ``coefs``: one per convolution, 0 where it is not tapped.  ``gt`` None: features of x alone (the pools
    run through the tap kernel on (x, x) with coefficient 0).  ``keep``: hold what a backward pass reads -- per tap-kernel layer the
    fp32 pre-activation of both halves, per other layer the activated 16-bit output of the restored half alone (a copy: the 2B
    matrix is released once the next layer has read it).  ``trace`` receives the pre-ReLU output of every convolution [2B, C, h, w]:
    fp32 where the tap kernel reads it, else from one more launch of the same convolution without the ReLU, at the 16 bits the layer
    stores.  ``style`` ({"coefs": one per convolution}): per tapped layer one ``grl_vgg_gram_fwd`` on the 2B-image matrix and one
    ``grl_vgg_gram_loss`` (csrc/gram.hip); the dict receives "loss" [1], "sums" (per-layer sums of |D|), "diffs" {convolution index: D
    [B, C, C]} and "bounds" [convolutions, 2B] (per image sum_c max_t |F[t, c]|, 0 where not tapped).
    Returns (loss [1] fp32 or None, per-layer sums of |fx - fg|, saved, per-layer (h, w))."""
    from . import ops

    vgg._check_size(x)
    B, _, H, W = x.shape
    plan = vgg._hip_plan()
    fw, _ = vgg._hip_packs(x.device)
    halves = [x] if gt is None else [x, gt]
    nb = B * len(halves)
    n0 = B * H * W
    t = ops.empty(nb * H * W, 4, dtype=torch.float32, device=x.device)
    for j, img in enumerate(halves):
        ops.vgg_prep(img.detach().float(), t[j * n0:(j + 1) * n0], use_input_norm=vgg.use_input_norm, range_norm=vgg.range_norm)
    loss = ops.empty(1, dtype=torch.float32, device=x.device)
    sums = ops.empty(len(plan), dtype=torch.float32, device=x.device)
    saved, dims, h, w, first = [], [], H, W, True
    if style is not None:
        assert gt is not None
        style.update(loss=torch.zeros(1, dtype=torch.float32, device=x.device), sums=torch.zeros(len(plan), dtype=torch.float32, device=x.device),
                     diffs={}, bounds=torch.zeros(len(plan), nb, dtype=torch.float32, device=x.device))
    for i, (tapped, pooled) in enumerate(plan):
        wp, bp = fw[i]
        kw = dict(x_cols=4) if i == 0 else {}
        dims.append((h, w))
        n = B * h * w
        if tapped or pooled:
            f = ops.conv3x3(t, wp, bp, nb, h, w, **kw)                     # the pre-activation, fp32: what the tap kernels read
            fx, fg = f[:n], f[n:] if gt is not None else f[:n]
            pool = ops.vgg_tap(fx, fg, B, h, w, loss, coefs[i] if coefs is not None else 0.0, accumulate=not first, pool=pooled,
                               layer_sum=sums[i:i + 1])
            first = False
            if style is not None and tapped:
                gram = ops.vgg_gram(f, nb, h * w, rowbound=style["bounds"][i])
                style["diffs"][i] = ops.vgg_gram_loss(gram, style["loss"], style["coefs"][i], accumulate=True, layer_sum=style["sums"][i:i + 1])
            saved.append(f if keep else None)
            pre = f
            if pooled:
                h, w = h // 2, w // 2
                t = pool if gt is not None else pool[: B * h * w]
        else:
            if trace is not None:
                pre = ops.conv3x3(t, wp, bp, nb, h, w, out_dtype=ops.GEMM_DTYPE, **kw)
            t = ops.conv3x3(t, wp, bp, nb, h, w, act=2, slope=0.0, out_dtype=ops.GEMM_DTYPE, **kw)   # ReLU rides in the epilogue
            saved.append(t[:n].clone() if keep else None)
        if trace is not None:
            trace.append(pre.detach().float().view(nb, dims[-1][0], dims[-1][1], -1).permute(0, 3, 1, 2))
    return (loss, sums, saved, dims) if gt is not None else (None, None, saved, dims)


def _hip_features(vgg: VGG19Features, x: torch.Tensor) -> Dict[str, torch.Tensor]:
    trace: list = []
    with torch.no_grad():
        _hip_chain(vgg, x, None, None, trace, keep=False)
    return {name: trace[i].contiguous() for i, (name, _, _, _) in enumerate(vgg.convs) if name in vgg.layer_name_list}


def decisions_from_trace(vgg: VGG19Features, trace: Sequence[torch.Tensor], B: int, diffs: Optional[Dict[str, torch.Tensor]] = None) -> dict:
    """Tests: the ``decisions`` of the composite read off the traced features [2B, C, h, w] of a run (restored first, then target):
    ReLU masks ``f > 0``, ``max_pool2d(return_indices=True)`` on relu(f) where a pool follows, ``sign(fx - fg)`` at the taps -- each in
    the trace's own arithmetic.  ``diffs`` ({layer: D [B, C, C]}, the Gram differences of that run: PerceptualStyleLoss.forward_traced)
    adds "gram_signs" {layer: sign(D)}.  CPU tensors."""
    masks, pools, signs = [], [], {}
    for (name, idx, _, _), t in zip(vgg.convs, trace):
        t = t.detach().cpu()
        fx = t[:B]
        masks.append(fx > 0)
        if idx + 2 < len(vgg.names) and vgg.names[idx + 2].startswith("pool"):
            pools.append(F.max_pool2d(F.relu(fx), 2, 2, return_indices=True)[1])
        if name in vgg.layer_name_list:
            signs[name] = torch.sign(fx - t[B:])
    dec = dict(masks=masks, pool_idx=pools, signs=signs)
    if diffs is not None:
        dec["gram_signs"] = {k: torch.sign(v.detach().cpu()) for k, v in diffs.items()}
    return dec


class _PerceptualFn(torch.autograd.Function):
    """loss = sum_l coef_l * sum |f_l(x) - f_l(gt)| on the HIP chain; backward: dL/dx alone."""

    @staticmethod
    def forward(ctx, x, gt, mod):
        vgg = mod.vgg
        B, _, H, W = x.shape
        keep = ctx.needs_input_grad[0]
        loss, sums, saved, dims = _hip_chain(vgg, x, gt, mod._coefs(B, H, W), mod._trace, keep=keep)
        mod._layer_sums = sums
        ctx.mod, ctx.dims, ctx.shape, ctx.xdtype = mod, dims, (B, H, W), x.dtype
        if keep:
            ctx.save_for_backward(*saved)
        return loss.view(())

    @staticmethod
    def backward(ctx, dloss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        mod = ctx.mod
        B, H, W = ctx.shape
        coefs = mod._coefs(B, H, W)
        up = float(dloss)                       # one host read per pass: S and the tap coefficients are launch arguments
        S = mod.last_scale = operand_scale(coefs, up)
        dx = _hip_chain_bwd(mod.vgg, ctx.saved_tensors, ctx.dims, ctx.shape, [S * c * up for c in coefs], S, dloss.device)
        return dx.to(ctx.xdtype), None, None


def _hip_chain_bwd(vgg: VGG19Features, saved, dims, shape, tap_k: Sequence[float], S: float, device, gram_k: Optional[Sequence[float]] = None,
                   diffs: Optional[dict] = None) -> torch.Tensor:
    """The backward launches for the restored half: dL/dx [B, 3, H, W] fp32.  ``tap_k``: per convolution S * coefficient * upstream;
    ``gram_k`` / ``diffs`` (the style loss): per convolution the k of ``grl_vgg_gram_bwd`` and the forward's D -- one launch after
    ``grl_vgg_tap_bwd`` adds k * F * sign(D) into the gradient matrix that kernel has just written."""
    from . import ops

    B, H, W = shape
    plan = vgg._hip_plan()
    _, bw = vgg._hip_packs(device)
    g = None
    for i in reversed(range(len(plan))):
        tapped, pooled = plan[i]
        h, w = dims[i]
        n = B * h * w
        if tapped or pooled:
            d = ops.vgg_tap_bwd(saved[i][:n], saved[i][n:], B, h, w, tap_k[i], g)
            if gram_k is not None and i in diffs and gram_k[i] != 0.0:
                ops.vgg_gram_bwd(saved[i], diffs[i], h * w, gram_k[i], d)
        else:
            d = torch.where(saved[i] > 0, g, 0.0)         # ReLU: the mask is y > 0 on the saved activated output
        wt, zb = bw[i]
        # the gradient arrives as S * g in fp32: nothing is left for the launch to scale
        g = ops.conv3x3(d, wt, zb, B, h, w, x_scale=1.0, out_scale=1.0, n_store=4 if i == 0 else 0)
    return ops.vgg_prep_bwd(g, B, H, W, scale=1.0 / S, use_input_norm=vgg.use_input_norm, range_norm=vgg.range_norm)


class _PerceptualStyleFn(torch.autograd.Function):
    """(perceptual, style) of one VGG pass on the HIP chain; backward: dL/dx alone, both terms in one reverse pass."""

    @staticmethod
    def forward(ctx, x, gt, mod):
        B, _, H, W = x.shape
        keep = ctx.needs_input_grad[0]
        style = dict(coefs=mod._style_coefs(B))
        loss, sums, saved, dims = _hip_chain(mod.vgg, x, gt, mod._coefs(B, H, W), mod._trace, keep=keep, style=style)
        mod._layer_sums, mod._style_sums, mod._diffs = sums, style["sums"], style["diffs"]
        ctx.mod, ctx.dims, ctx.shape, ctx.xdtype = mod, dims, (B, H, W), x.dtype
        ctx.diffs, ctx.bounds = style["diffs"], style["bounds"]
        if keep:
            ctx.save_for_backward(*saved)
        return loss.view(()), style["loss"].view(())

    @staticmethod
    def backward(ctx, dpercep, dstyle):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        mod = ctx.mod
        B, H, W = ctx.shape
        coefs, gk = mod._coefs(B, H, W), mod._gram_ks(B, ctx.dims)
        # one host read per pass: both upstream gradients and, per layer, the forward's bound on |F sign(D)| over the restored images
        host = torch.cat([dpercep.reshape(1).float(), dstyle.reshape(1).float(), ctx.bounds[:, :B].amax(dim=1)]).tolist()
        up_p, up_s, bounds = host[0], host[1], host[2:]
        S = mod.last_scale = operand_scale([abs(c * up_p) + abs(k * up_s) * m for c, k, m in zip(coefs, gk, bounds)])
        dx = _hip_chain_bwd(mod.vgg, ctx.saved_tensors, ctx.dims, ctx.shape, [S * c * up_p for c in coefs], S, dpercep.device,
                            gram_k=[S * k * up_s for k in gk], diffs=ctx.diffs)
        return dx.to(ctx.xdtype), None, None


class PerceptualLoss(nn.Module):
    """The reference's PerceptualLoss at ``style_weight = 0``: ``forward(x, gt)`` returns ``(percep_loss, None)`` with
    percep_loss = perceptual_weight * sum_l layer_weights[l] * L1(f_l(x), f_l(gt)), features before ReLU, gt detached.

    ``layer_weights``: {layer name: weight} (``GAN_LAYER_WEIGHTS``: the GAN stage's yaml); ``weights``: the VGG19 state dict
    (``load_vgg19(path)``).  NotImplementedError: ``style_weight > 0`` (the style loss lives in ``PerceptualStyleLoss``) and the
    criteria ``l2`` / ``fro`` (not built; the reference's ``l2`` branch cannot be constructed either: it names ``torch.nn.L2loss``).  ``perceptual_weight <= 0`` returns ``(None, None)``
    as the reference does.  CUDA tensors take the HIP chain (module docstring), CPU tensors the float64 composite;
    ``operand_dtype`` / ``decisions`` / ``grad_scale`` belong to the composite."""

    def __init__(self, layer_weights: Dict[str, float], weights: Dict[str, torch.Tensor], use_input_norm: bool = True, range_norm: bool = False,
                 perceptual_weight: float = 1.0, style_weight: float = 0.0, criterion: str = "l1"):
        super().__init__()
        if style_weight > 0:
            raise NotImplementedError("PerceptualLoss is the reference's class at style_weight = 0; the style loss is PerceptualStyleLoss")
        if criterion != "l1":
            raise NotImplementedError(f"criterion {criterion!r}: only 'l1' is built")
        self.layer_weights = dict(layer_weights)
        self.perceptual_weight, self.style_weight, self.criterion_type = float(perceptual_weight), 0.0, criterion
        self.vgg = VGG19Features(list(self.layer_weights), weights, use_input_norm, range_norm)
        self.last_layer_means: Optional[list] = None     # CPU: the per-layer L1 means of the last call (before their weights)
        self.last_scale: Optional[float] = None          # CUDA: the operand scale S of the last backward pass
        self._layer_sums, self._trace = None, None

    def _tap_order(self):
        return [n for n in self.vgg.names if n in self.layer_weights]

    def _numels(self, B: int, H: int, W: int):
        out, h, w, c = {}, H, W, 3
        for name in self.vgg.names:
            if name.startswith("conv"):
                c = _WIDTHS[int(name[4]) - 1]
            elif name.startswith("pool"):
                h, w = h // 2, w // 2
            out[name] = B * c * h * w
        return out

    def _coefs(self, B: int, H: int, W: int):
        ne = self._numels(B, H, W)
        return [self.layer_weights[n] * self.perceptual_weight / ne[n] if n in self.layer_weights else 0.0 for n, _, _, _ in self.vgg.convs]

    def layer_means(self, B: int, H: int, W: int) -> torch.Tensor:
        """CUDA: the per-layer L1 means of the last forward (a device tensor; no host read)."""
        ne = self._numels(B, H, W)
        at = [i for i, (n, _, _, _) in enumerate(self.vgg.convs) if n in self.layer_weights]
        return self._layer_sums[at] / torch.tensor([float(ne[n]) for n in self._tap_order()], device=self._layer_sums.device)

    def composite(self, x: torch.Tensor, gt: torch.Tensor, operand_dtype=None, decisions: Optional[dict] = None,
                  grad_scale: Optional[float] = None, trace: Optional[list] = None) -> torch.Tensor:
        """The yardstick: float64 torch.  ``decisions`` adds {"signs": {layer: sign(fx - fg)}} to VGG19Features.composite's: the L1
        term of a layer becomes mean(sign * (fx - fg)).  The target's own path always decides for itself (it has no gradient)."""
        fx, fg = self._features64(x, gt, operand_dtype, decisions, grad_scale, trace)
        return self._percep_term(fx, fg, decisions, torch.float64)

    def _features64(self, x, gt, operand_dtype, decisions, grad_scale, trace):
        fx = self.vgg.composite(x.double(), operand_dtype, decisions, grad_scale, trace)
        with torch.no_grad():
            fg = self.vgg.composite(gt.detach().double(), operand_dtype)
        return fx, fg

    def _percep_term(self, fx, fg, decisions, dtype):
        total, means = 0, []
        for k in fx:
            if decisions is None:
                m = F.l1_loss(fx[k], fg[k])
            else:
                m = (decisions["signs"][k].to(dtype) * (fx[k] - fg[k])).mean()
            means.append(m.detach())
            total = total + m * self.layer_weights[k]
        self.last_layer_means = means
        return total * self.perceptual_weight

    def forward(self, x: torch.Tensor, gt: torch.Tensor, operand_dtype=None):
        self.vgg._check_size(x)
        if x.shape != gt.shape:
            raise ValueError(f"PerceptualLoss: x {tuple(x.shape)} and gt {tuple(gt.shape)} differ")
        if not self.perceptual_weight > 0:
            return None, None
        if x.is_cuda:
            if operand_dtype is not None:
                raise ValueError("operand_dtype belongs to the CPU composite path")
            return _PerceptualFn.apply(x, gt.detach(), self), None
        return self.composite(x, gt, operand_dtype), None

    def forward_traced(self, x: torch.Tensor, gt: torch.Tensor):
        """Tests: (loss, [the sixteen pre-ReLU feature matrices [2B, C, h, w]: the restored images first, then the targets]) of one
        CUDA forward.  The tapped entries are the fp32 matrices the tap kernels read; an untapped layer's ReLU rides in its
        convolution's epilogue, so its entry comes from one more launch of that convolution without the ReLU, at the 16 bits the layer
        stores: ``> 0`` on it is exactly the backward's mask ``y > 0``."""
        self._trace = []
        try:
            loss = self.forward(x, gt)[0]
            return loss, self._trace
        finally:
            self._trace = None


class PerceptualStyleLoss(PerceptualLoss):
    """The reference's PerceptualLoss with the style term (losses/losses.py:59-187, criterion "l1"): ``forward(x, gt)`` returns
    ``(percep_loss, style_loss)``; a term is None exactly when its weight is <= 0.

        G_b      = F_b^T F_b / (C*h*w)            F_b [h*w, C]: the tapped pre-ReLU feature of image b       losses.py:174-187
        style    = style_weight * sum_l layer_weights[l] * mean over (b, c, c') of |G_b(x) - G_b(gt)|        losses.py:160-168
        dL/dF_b  = k_l / (C*h*w) * F_b (Sigma_b + Sigma_b^T),  Sigma_b = sign(G_b(x) - G_b(gt)),  k_l = upstream * style_weight * w_l / (B*C^2)

    ``PerceptualLoss`` keeps refusing ``style_weight > 0`` (its tests pin that); ``l2`` / ``fro`` stay NotImplementedError here too.

    CUDA: one autograd.Function with two outputs on ONE VGG pass -- the chain of ``PerceptualLoss`` plus, per tapped layer, one
    ``grl_vgg_gram_fwd`` on the 2B-image matrix and one ``grl_vgg_gram_loss`` (csrc/gram.hip: f32-input MFMA, the features are never
    rounded below fp32), and in the backward one ``grl_vgg_gram_bwd`` after ``grl_vgg_tap_bwd``.  ``perceptual_weight <= 0`` gives the
    tap kernels coefficient 0.  G is exactly symmetric there, so Sigma + Sigma^T = 2 Sigma.

    The operand scale S covers both terms.  The gradient at a tap is S * (coef_l * up_p * sign(fx - fg) + k'_l * up_s * (F Sigma)[t, c])
    with k'_l = 2 * style_weight * w_l / (B*C^2 * C*h*w); Sigma has entries -1 / 0 / 1, so |(F Sigma)[t, c]| <= sum_c |F[t, c]| <=
    m_l := max over the restored images of sum_c max_t |F[t, c]|, which the Gram forward leaves per image.  S is the power of two that
    puts  max_l (|coef_l * up_p| + |k'_l * up_s| * m_l)  -- a bound on every tap gradient, not its value -- into (2^-4, 2^-3]; the
    backward reads both upstream gradients and the five m_l with one host read.  ``last_scale`` holds S of the last backward.

    CPU: ``composite`` returns (percep, style) in float64; its ``decisions`` gain {"gram_signs": {layer: sign(D)}} (the style term of
    a layer becomes mean(sign * D)); ``last_style_means`` / ``style_layer_means`` are the per-layer means of |D| before their weights."""

    def __init__(self, layer_weights: Dict[str, float], weights: Dict[str, torch.Tensor], use_input_norm: bool = True, range_norm: bool = False,
                 perceptual_weight: float = 1.0, style_weight: float = 0.0, criterion: str = "l1"):
        super().__init__(layer_weights, weights, use_input_norm, range_norm, perceptual_weight, 0.0, criterion)
        self.style_weight = float(style_weight)
        self.last_style_means: Optional[list] = None     # CPU: the per-layer means of |D| of the last call (before their weights)
        self.last_diffs: Optional[dict] = None           # CPU: {layer: D [B, C, C]} of the last call, detached
        self._style_sums, self._diffs = None, None

    def _style_coefs(self, B: int):
        """Per convolution: style_weight * layer weight / (B*C^2), 0 where it is not tapped."""
        return [self.layer_weights[n] * self.style_weight / (B * c * c) if n in self.layer_weights else 0.0 for n, _, _, c in self.vgg.convs]

    def _gram_ks(self, B: int, dims):
        """Per convolution: the k of grl_vgg_gram_bwd before S and the upstream gradient, 2 * style coefficient / (C*h*w)."""
        return [2.0 * k / (c * h * w) for k, (_, _, _, c), (h, w) in zip(self._style_coefs(B), self.vgg.convs, dims)]

    def style_layer_means(self, B: int) -> torch.Tensor:
        """CUDA: the per-layer means of |D| of the last forward (a device tensor; no host read)."""
        at = [i for i, (n, _, _, _) in enumerate(self.vgg.convs) if n in self.layer_weights]
        return self._style_sums[at] / torch.tensor([float(B * self.vgg.convs[i][3] ** 2) for i in at], device=self._style_sums.device)

    def composite(self, x: torch.Tensor, gt: torch.Tensor, operand_dtype=None, decisions: Optional[dict] = None,
                  grad_scale: Optional[float] = None, trace: Optional[list] = None):
        """The yardstick: (percep, style) in float64 torch, both always formed (``forward`` drops the one whose weight is <= 0)."""
        fx, fg = self._features64(x, gt, operand_dtype, decisions, grad_scale, trace)
        percep = self._percep_term(fx, fg, decisions, torch.float64)
        total, means, diffs = 0, [], {}
        for k in fx:
            _, c, h, w = fx[k].shape
            tx, tg = fx[k].flatten(2), fg[k].flatten(2)
            d = (tx @ tx.transpose(1, 2) - tg @ tg.transpose(1, 2)) / (c * h * w)
            m = d.abs().mean() if decisions is None else (decisions["gram_signs"][k].to(torch.float64) * d).mean()
            means.append(m.detach())
            diffs[k] = d.detach()
            total = total + m * self.layer_weights[k]
        self.last_style_means, self.last_diffs = means, diffs
        return percep, total * self.style_weight

    def forward(self, x: torch.Tensor, gt: torch.Tensor, operand_dtype=None):
        self.vgg._check_size(x)
        if x.shape != gt.shape:
            raise ValueError(f"PerceptualStyleLoss: x {tuple(x.shape)} and gt {tuple(gt.shape)} differ")
        want_p, want_s = self.perceptual_weight > 0, self.style_weight > 0
        if not (want_p or want_s):
            return None, None
        if x.is_cuda:
            if operand_dtype is not None:
                raise ValueError("operand_dtype belongs to the CPU composite path")
            if not want_s:                                   # no Gram launch: the chain of PerceptualLoss as it is
                return _PerceptualFn.apply(x, gt.detach(), self), None
            percep, style = _PerceptualStyleFn.apply(x, gt.detach(), self)
        else:
            percep, style = self.composite(x, gt, operand_dtype)
        return (percep if want_p else None), (style if want_s else None)

    def _coefs(self, B: int, H: int, W: int):
        """A perceptual term that is off (weight <= 0) gives the tap kernels coefficient 0."""
        return super()._coefs(B, H, W) if self.perceptual_weight > 0 else [0.0] * len(self.vgg.convs)

    def forward_traced(self, x: torch.Tensor, gt: torch.Tensor):
        """Tests: ((percep, style), the sixteen traced feature matrices of PerceptualLoss.forward_traced, {layer: D [B, C, C]} of that
        run) of one CUDA forward."""
        self._trace = []
        try:
            losses = self.forward(x, gt)
            names = [n for n, _, _, _ in self.vgg.convs]
            return losses, self._trace, {names[i]: d for i, d in (self._diffs or {}).items()}
        finally:
            self._trace = None
