"""LPIPS with the VGG trunk: ``val_lpips`` of the reference's ``restorer_perceptual`` metric group (config/metric/restorer_perceptual.yaml).

  replaces  lpips.LPIPS(net="vgg").forward(img1, img2, normalize=True)      utils/metrics/lpips.py:20,40 (default net_type="vgg")

The ``lpips`` package was not available where this was built and is not in the reference tree, so the definition is restated here from the
package's version 0.1 and pinned against that statement and against the float64 composite below -- NOT against a run of the package.
For images x0, x1 in [0, 1]:

  1. x <- 2x - 1
  2. scaling layer (x - shift) / scale per channel, float32 buffers built from shift = (-0.030, -0.088, -0.188),
     scale = (0.458, 0.448, 0.450)
  3. torchvision ``vgg16().features`` (no batch norm; convolutions at 0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28; blocks of
     2, 2, 3, 3, 3 convolutions, widths 64, 128, 256, 512, 512), tapped AFTER the ReLU that closes each block: relu1_2, relu2_2,
     relu3_3, relu4_3, relu5_3 (indices 3, 8, 15, 22, 29); pool5 is not run
  4. per tap l and pixel: u = f / (sqrt(sum_c f_c^2) + 1e-10) for both images (the eps outside the root; an all-zero pixel gives zeros)
  5. d_l = mean over the h_l x w_l pixels of sum_c w_l[c] * (u0_c - u1_c)^2, w_l the bias-free 1x1 convolution
     ``lin{l}.model.1.weight`` [1, C_l, 1, 1] of the package's weights/v0.1/vgg.pth (its dropout is inactive in eval)
  6. lpips = sum_l d_l, one value per image

Both weight files are the user's: torchvision's ``vgg16-397923af.pth`` and the package's ``vgg.pth``, read with ``torch.load``; nothing
is downloaded.  Their key names (``features.{idx}.{weight,bias}``; ``lin{l}.model.1.weight``, or plain ``lin{l}`` of shape [C_l])
could not be checked against the files here; the loader names the key it misses.

CUDA tensors: both images as one batch of 2B through thirteen ``grl_conv3x3_fwd`` launches on filter banks packed once per device --
ReLU in the epilogue of the eight untapped layers (act = 2, 16-bit output), fp32 output at the five block closers -- and per closer one
``grl_lpips_tap`` (csrc/lpips.hip): ReLU, steps 4-5 into out[b] (float64, fixed order, no atomics) and the 2 x 2 max pool of both
halves as the next block's 16-bit operand.  A missing kernel is an error; there is no fallback to eager torch.
CPU tensors: ``composite`` -- plain float64 torch, the yardstick of the tests (``operand_dtype=torch.float16`` emulates the kernels'
operand rounding as ``perceptual._contract`` does).

LPIPS as a training loss is ``LPIPSLoss`` below: one ``autograd.Function`` on the same forward launches, ``grl_lpips_tap_bwd`` and
``grl_lpips_prep_bwd`` (csrc/lpips.hip) plus thirteen data-gradient launches of ``grl_conv3x3_fwd`` in the backward, for the restored
image alone, under a power-of-two scale S measured per pass (``loss_scale``).  ``GanStep(lpips=...)`` / ``train --gan --lpips-weight``.

Not built: ``net="alex"`` / ``"squeeze"``, ``spatial=True`` maps, gradients for the target or the weights, the LPIPS term in a
captured GAN step (the data-parallel ``GanStep`` carries it as it is: no trained parameters, a per-pass scale that cancels), a tap backward fused into a convolution.
"""
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from .perceptual import MIN_SIDE, _contract, _EmuConv, layer_names, operand_scale

BLOCKS = (2, 2, 3, 3, 3)                         # convolutions per block of vgg16
WIDTHS = (64, 128, 256, 512, 512)
NAMES: List[str] = layer_names(BLOCKS)           # position in this list == index in torchvision's vgg16().features
CONV_INDEX = {n: i for i, n in enumerate(NAMES) if n.startswith("conv")}     # conv1_1: 0 ... conv5_3: 28
TAPS = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
TAP_INDEX = tuple(NAMES.index(n) for n in TAPS)  # 3, 8, 15, 22, 29
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10


def _conv_shapes():
    """(name, features index, cin, cout) of the thirteen convolutions."""
    out, cin = [], 3
    for name, idx in CONV_INDEX.items():
        cout = WIDTHS[int(name[4]) - 1]
        out.append((name, idx, cin, cout))
        cin = cout
    return out


def lin_key(l: int) -> str:
    return f"lin{l}.model.1.weight"


def lpips_term(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Steps 4-5 on two post-ReLU features [B, C, h, w] with the weights w [C]: (B,), in the features' dtype.  Evaluated as written:
    normalise, subtract, square."""
    u0 = f0 / (f0.pow(2).sum(dim=1, keepdim=True).sqrt() + EPS)
    u1 = f1 / (f1.pow(2).sum(dim=1, keepdim=True).sqrt() + EPS)
    return ((u0 - u1).pow(2) * w.view(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def seeded_weights(seed: int) -> Tuple[Dict[str, torch.Tensor], Dict[str, torch.Tensor]]:
    """Stand-ins for the two weight files (tests, tools): (vgg16 state dict, lin state dict), float32.  The VGG as
    ``perceptual.seeded_state_dict`` draws it -- He-scaled normals, biases 0.1 * normal; the lin weights |normal| / C_l under the
    package's key; every value rounded to an fp16-representable one."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for _, idx, cin, cout in _conv_shapes():
        w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        b = torch.randn(cout, generator=g) * 0.1
        sd[f"features.{idx}.weight"] = w.to(torch.float16).float()
        sd[f"features.{idx}.bias"] = b.to(torch.float16).float()
    lin = {}
    for l, c in enumerate(WIDTHS):
        lin[lin_key(l)] = (torch.randn(c, generator=g).abs() / c).to(torch.float16).float().view(1, c, 1, 1)
    return sd, lin


class LPIPS(nn.Module):
    """``forward(restored, target)``: LPIPS (net "vgg", version 0.1) of every image pair of two equal-shaped RGB batches [B, 3, H, W]
    in [0, 1], sides >= 16: a float64 tensor of shape (B,), lower is better.  ``vgg16_state_dict``: torchvision's keys
    ``features.{0,2,5,...,28}.{weight,bias}`` (``classifier.*`` is ignored); ``lin_state_dict``: ``lin{l}.model.1.weight`` of shape
    [1, C_l, 1, 1], or plain ``lin{l}`` of shape [C_l], l = 0..4.  A missing or misshapen key raises and names the key.  Everything is
    frozen; there is no backward."""

    def __init__(self, vgg16_state_dict: Dict[str, torch.Tensor], lin_state_dict: Dict[str, torch.Tensor]):
        super().__init__()
        self.convs = _conv_shapes()
        self.weights, self.biases, self.lins = nn.ParameterList(), nn.ParameterList(), nn.ParameterList()
        for _, idx, cin, cout in self.convs:
            for kind, shape, dest in (("weight", (cout, cin, 3, 3), self.weights), ("bias", (cout,), self.biases)):
                key = f"features.{idx}.{kind}"
                if key not in vgg16_state_dict:
                    raise KeyError(f"VGG16 weights: key {key!r} is missing")
                t = vgg16_state_dict[key]
                if tuple(t.shape) != shape:
                    raise ValueError(f"VGG16 weights: key {key!r} has shape {tuple(t.shape)}, expected {shape}")
                dest.append(nn.Parameter(t.detach().clone().float(), requires_grad=False))
        for l, c in enumerate(WIDTHS):
            key = lin_key(l) if lin_key(l) in lin_state_dict else f"lin{l}"
            if key not in lin_state_dict:
                raise KeyError(f"LPIPS linear weights: key {lin_key(l)!r} (or plain {f'lin{l}'!r}) is missing")
            t = lin_state_dict[key]
            if tuple(t.shape) != ((1, c, 1, 1) if key == lin_key(l) else (c,)):
                raise ValueError(f"LPIPS linear weights: key {key!r} has shape {tuple(t.shape)}, expected "
                                 f"{(1, c, 1, 1) if key == lin_key(l) else (c,)}")
            self.lins.append(nn.Parameter(t.detach().clone().float().reshape(c), requires_grad=False))
        # float32 buffers, as the package's ScalingLayer builds them: the nearest floats to the decimals
        self.register_buffer("shift", torch.Tensor(SHIFT).view(1, 3, 1, 1))
        self.register_buffer("scale", torch.Tensor(SCALE).view(1, 3, 1, 1))
        self._packs: dict = {}                   # device -> forward banks: packed once, not per call
        self.eval()

    def _apply(self, fn, *a, **kw):
        self._packs.clear()
        return super()._apply(fn, *a, **kw)

    def _check(self, restored: torch.Tensor, target: torch.Tensor) -> None:
        if restored.dim() != 4 or restored.shape[1] != 3:
            raise ValueError(f"LPIPS: expected RGB images [B, 3, H, W], got {tuple(restored.shape)}")
        if restored.shape != target.shape:
            raise ValueError(f"LPIPS: restored {tuple(restored.shape)} and target {tuple(target.shape)} differ")
        if restored.shape[2] < MIN_SIDE or restored.shape[3] < MIN_SIDE:
            raise ValueError(f"LPIPS: the images must be at least {MIN_SIDE} x {MIN_SIDE} (got {restored.shape[2]} x {restored.shape[3]}): "
                             "four pools would leave nothing")
        if restored.device != target.device:
            raise ValueError(f"LPIPS: restored on {restored.device}, target on {target.device}")

    # ---- CPU: the composite -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def composite(self, restored: torch.Tensor, target: torch.Tensor, operand_dtype=None, trace: Optional[list] = None) -> torch.Tensor:
        """The yardstick: float64 torch on the tensors' device, (B,).  ``operand_dtype``: both operands of every convolution rounded
        to that type.  ``trace`` receives the five tapped post-ReLU features [2B, C, h, w], the restored images first."""
        self._check(restored, target)
        B = restored.shape[0]
        x = torch.cat([restored, target]).double()
        x = ((2 * x - 1) - self.shift.double()) / self.scale.double()
        total, ci, tap = 0, 0, 0
        for pos, name in enumerate(NAMES[: TAP_INDEX[-1] + 1]):
            if name.startswith("conv"):
                w, b = self.weights[ci].double(), self.biases[ci].double()
                x = F.conv2d(_contract(x, operand_dtype), _contract(w, operand_dtype), b, padding=1)
                ci += 1
            elif name.startswith("relu"):
                x = F.relu(x)
            else:
                x = F.max_pool2d(x, 2, 2)
            if pos == TAP_INDEX[tap]:
                if trace is not None:
                    trace.append(x)
                total = total + lpips_term(x[:B], x[B:], self.lins[tap].double())
                tap += 1
        return total

    # ---- CUDA: the HIP chain ------------------------------------------------------------------------------------------------------
    def _hip_packs(self, device):
        from . import ops

        key = str(device)
        if key not in self._packs:
            banks = [ops.pack_conv_train(w.to(device), b.to(device), (cout + 15) // 16 * 16, (cin + 31) // 32 * 32)
                     for (_, _, cin, cout), w, b in zip(self.convs, self.weights, self.biases)]
            self._packs[key] = (banks, [w.to(device).contiguous() for w in self.lins])
        return self._packs[key]

    @torch.no_grad()
    def _hip(self, restored: torch.Tensor, target: torch.Tensor, trace: Optional[list] = None, keep: Optional[dict] = None) -> torch.Tensor:
        """``keep`` (the training forward of ``LPIPSLoss``): a dict that receives what the backward reads -- "saved": per convolution
        the fp32 pre-activation of both halves at a block closer, else a copy of the 16-bit activated output of the restored half;
        "dims": per convolution (h, w); "gmax" [5] fp32: the taps' gradient bounds G_l (the TRAIN instantiation of the tap kernel).
        Without it the launches are the metric's, bit for bit."""
        from . import ops

        B, _, H, W = restored.shape
        banks, lins = self._hip_packs(restored.device)
        n0 = B * H * W
        t = ops.empty(2 * n0, 4, dtype=torch.float32, device=restored.device)
        for j, img in enumerate((restored, target)):
            ops.lpips_prep(img.detach().float(), t[j * n0:(j + 1) * n0])
        out = ops.empty(B, dtype=torch.float64, device=restored.device)
        if keep is not None:
            keep.update(saved=[], dims=[], gmax=ops.empty(len(TAPS), dtype=torch.float32, device=restored.device))
        h, w, tap = H, W, 0
        for i, (_, idx, _, _) in enumerate(self.convs):
            wp, bp = banks[i]
            kw = dict(x_cols=4) if i == 0 else {}
            if keep is not None:
                keep["dims"].append((h, w))
            if idx + 1 == TAP_INDEX[tap]:                                       # a block closer: fp32, what the tap kernel reads
                f = ops.conv3x3(t, wp, bp, 2 * B, h, w, **kw)
                last = tap == len(TAPS) - 1
                t = ops.lpips_tap(f, lins[tap], B, h, w, out, accumulate=tap > 0, pool=not last,
                                  gmax=keep["gmax"][tap:tap + 1] if keep is not None else None)
                if trace is not None:
                    trace.append(torch.relu(f).view(2 * B, h, w, -1).permute(0, 3, 1, 2))
                if keep is not None:
                    keep["saved"].append(f)
                h, w, tap = h // 2, w // 2, tap + 1
            else:
                t = ops.conv3x3(t, wp, bp, 2 * B, h, w, act=2, slope=0.0, out_dtype=ops.GEMM_DTYPE, **kw)   # ReLU rides in the epilogue
                if keep is not None:                                            # a copy: the 2B matrix goes once the next layer has read it
                    keep["saved"].append(t[: B * h * w].clone())
        return out

    def forward(self, restored: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        self._check(restored, target)
        if restored.is_cuda:
            return self._hip(restored, target)
        return self.composite(restored, target)

    def forward_traced(self, restored: torch.Tensor, target: torch.Tensor):
        """Tests: (value (B,), [the five tapped post-ReLU features [2B, C, h, w] of one CUDA forward: ReLU of the fp32 matrices the tap
        kernel read, the restored images first])."""
        self._check(restored, target)
        if not restored.is_cuda:
            raise ValueError("forward_traced belongs to the CUDA path; the composite takes trace=")
        trace: list = []
        return self._hip(restored, target, trace), trace


def _load_state_dict(path: str, what: str) -> Dict[str, torch.Tensor]:
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: expected the state dict of {what}, got {type(sd).__name__}")
    return sd


def load_lpips(vgg16_path: str, lin_path: str) -> LPIPS:
    """The metric from the user's two files by ``torch.load(..., weights_only=True)`` alone: torchvision's ``vgg16-397923af.pth`` and
    the lpips package's ``weights/v0.1/vgg.pth``.  Neither torchvision nor the package is needed and nothing is ever downloaded."""
    return LPIPS(_load_state_dict(vgg16_path, "torchvision's vgg16"), _load_state_dict(lin_path, "the lpips package's vgg.pth"))


# ---- LPIPS as a training loss -------------------------------------------------------------------------------------------------------
def _safe_norm(f: torch.Tensor) -> torch.Tensor:
    """sqrt(sum_c f_c^2) with derivative 0 where it is 0: the same value as the plain root, but ``sqrt'(0) * 0`` never forms, so a
    pixel whose features are all zero under MULTIPLIED ReLU masks gets a finite (zero) gradient, as torch's selecting relu gives it."""
    s = f.pow(2).sum(dim=1, keepdim=True)
    pos = s > 0
    return torch.where(pos, torch.where(pos, s, torch.ones_like(s)).sqrt(), torch.zeros_like(s))


def _safe_term(f0: torch.Tensor, f1: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``lpips_term`` through ``_safe_norm``: the same values, a derivative that is defined at a zero norm."""
    u0, u1 = f0 / (_safe_norm(f0) + EPS), f1 / (_safe_norm(f1) + EPS)
    return ((u0 - u1).pow(2) * w.view(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def _tap_parts(pre: torch.Tensor, w: torch.Tensor, B: int):
    """Float64 pieces of the closed form on pre [2B, C, h, w]: (f0, r, f0 / n, e, sum_j e_j u0_j, ebar, sum_j ebar_j u0_j)."""
    f = F.relu(pre.double())
    f0, f1 = f[:B], f[B:]
    n0, n1 = f0.pow(2).sum(dim=1, keepdim=True).sqrt(), f1.pow(2).sum(dim=1, keepdim=True).sqrt()
    r = 1.0 / (n0 + EPS)
    u0, u1 = f0 * r, f1 / (n1 + EPS)
    fn = torch.where(n0 > 0, f0 / torch.where(n0 > 0, n0, torch.ones_like(n0)), torch.zeros_like(f0))
    w = w.double().view(1, -1, 1, 1)
    e, ebar = 2 * w * (u0 - u1), 2 * w.abs() * (u0 + u1)
    return f0, r, fn, e, (e * u0).sum(dim=1, keepdim=True), ebar, (ebar * u0).sum(dim=1, keepdim=True)


def tap_backward_reference(pre: torch.Tensor, w: torch.Tensor, B: int, k: float, dpool: Optional[torch.Tensor] = None):
    """The closed form of one tap's backward in float64.  pre [2B, C, h, w]: the pre-activation, restored images first; w [C];
    k = upstream / (B*h*w); dpool [B, C, h//2, w//2] or None: the gradient of the pooled output.  Returns (g, A): g [B, C, h, w] =
    dL/dpre0 = [pre0 > 0] * (k * r * (e - (f0 / n) * sum_j e_j u0_j) + dpool at the first maximum of its window), and A, the same
    expression with every term replaced by its absolute value (ebar_c = 2 |w_c| (u0_c + u1_c)): the scale of the first-order error
    bound of an fp32 evaluation."""
    f0, r, fn, e, dot, ebar, dotbar = _tap_parts(pre, w, B)
    g, A = k * r * (e - fn * dot), abs(k) * r * (ebar + fn * dotbar)
    if dpool is not None:
        idx = F.max_pool2d(f0, 2, 2, return_indices=True)[1]
        routed = torch.zeros_like(f0).flatten(2).scatter_(2, idx.flatten(2), dpool.double().flatten(2)).view_as(f0)
        g, A = g + routed, A + routed.abs()
    mask = pre[:B] > 0
    return torch.where(mask, g, torch.zeros_like(g)), torch.where(mask, A, torch.zeros_like(A))


def tap_bound_reference(pre: torch.Tensor, w: torch.Tensor, B: int):
    """(G, Gbar) in float64: the gradient bound G_l of one tap -- the largest |r * (e_c - (f0_c / n) * sum_j e_j u0_j)| over the
    restored pixels and unmasked channels, without k -- and the same maximum with every term replaced by its absolute value."""
    g, A = tap_backward_reference(pre, w, B, 1.0)
    return float(g.abs().max()), float(A.max())


def loss_scale(terms: Sequence[float]) -> float:
    """The power of two S of one backward pass: ``perceptual.operand_scale``'s rule on T = max_l k_l * G_l, so that the largest tap
    term S * T lands in (2^-4, 2^-3]; 1.0 where T is zero or any term is not finite.  The tap gradient carries 1 / ||f||, which has no
    a-priori bound, so the G_l are measured by the forward (``grl_lpips_tap`` with gmax) and not derived from coefficients."""
    terms = [abs(float(t)) for t in terms]
    if not terms or not all(math.isfinite(t) for t in terms):
        return 1.0
    return operand_scale([max(terms)])


def decisions_from_trace(layers: Sequence[torch.Tensor], B: int) -> dict:
    """The ``decisions`` of ``LPIPSLoss.composite`` read off the thirteen layer outputs [>= B, C, h, w] of a run (the restored images
    first): ReLU masks ``t > 0`` -- the same on a pre-activation and on an activated output -- and the
    ``max_pool2d(return_indices=True)`` indices on relu(t) after every block but the last.  CPU tensors."""
    masks, pools, tap = [], [], 0
    for (_, idx, _, _), t in zip(_conv_shapes(), layers):
        fx = t.detach().cpu()[:B]
        masks.append(fx > 0)
        if idx + 1 == TAP_INDEX[tap]:
            if tap < len(TAPS) - 1:
                pools.append(F.max_pool2d(F.relu(fx.double()), 2, 2, return_indices=True)[1])
            tap += 1
    return dict(masks=masks, pool_idx=pools)


class _LpipsFn(torch.autograd.Function):
    """loss = mean_b LPIPS(x_b, gt_b) on the HIP chain; backward: dL/dx alone, under the measured power-of-two scale S."""

    @staticmethod
    def forward(ctx, x, gt, mod):
        B, _, H, W = x.shape
        keep = {} if ctx.needs_input_grad[0] else None
        out = mod.lpips._hip(x, gt, mod._trace, keep)
        ctx.mod, ctx.shape, ctx.xdtype = mod, (B, H, W), x.dtype
        if keep is not None:
            ctx.dims = keep["dims"]
            ctx.save_for_backward(keep["gmax"], *keep["saved"])
            mod._layers = (keep["saved"], keep["dims"]) if mod._trace is not None else None
        return out.mean().float()                # the fp32 rounding of the float64 mean

    @staticmethod
    def backward(ctx, dloss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        from . import ops

        mod = ctx.mod
        B, H, W = ctx.shape
        gmax, saved = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        # one host read per pass: the upstream gradient and the five measured bounds; S and the k_l are launch arguments
        host = torch.cat([dloss.reshape(1).float(), gmax]).tolist()
        up, bounds = host[0], host[1:]
        closers = [i for i, (_, idx, _, _) in enumerate(mod.lpips.convs) if idx + 1 in TAP_INDEX]
        ks = [up / (B * ctx.dims[i][0] * ctx.dims[i][1]) for i in closers]
        S = loss_scale([k * g for k, g in zip(ks, bounds)])
        mod.last_scale, mod.last_bounds = S, bounds
        _, lins = mod.lpips._hip_packs(dloss.device)
        bw = mod._bw_packs(dloss.device)
        g, tap = None, len(TAPS) - 1
        for i in reversed(range(len(mod.lpips.convs))):
            h, w = ctx.dims[i]
            if i in closers:
                d = ops.lpips_tap_bwd(saved[i], lins[tap], B, h, w, S * ks[tap], g)
                tap -= 1
            else:
                d = torch.where(saved[i] > 0, g, 0.0)     # ReLU: the mask is y > 0 on the saved activated output
            wt, zb = bw[i]
            # the gradient arrives as S * g in fp32: nothing is left for the launch to scale
            g = ops.conv3x3(d, wt, zb, B, h, w, x_scale=1.0, out_scale=1.0, n_store=4 if i == 0 else 0)
        return ops.lpips_prep_bwd(g, B, H, W, scale=1.0 / S).to(ctx.xdtype), None, None


class LPIPSLoss(nn.Module):
    """LPIPS as a training loss: ``forward(restored, target)`` is the scalar mean over the batch of what ``lpips_model`` (an ``LPIPS``,
    shared with the metric) returns; only ``restored`` gets a gradient.

    CUDA: ONE ``autograd.Function``.  The forward is the metric's launch sequence; with a gradient wanted the five tap launches take
    the TRAIN instantiation, which also leaves the gradient bound G_l per tap, and the fp32 pre-activations of the five block closers
    and the 16-bit activated output of the restored half elsewhere are kept.  The backward runs the chain in reverse for the restored
    half: ``grl_lpips_tap_bwd`` at the closers, the mask y > 0 elsewhere, thirteen data-gradient launches of ``grl_conv3x3_fwd`` on
    banks packed once per device with ``flip_t=True``, ``grl_lpips_prep_bwd`` at the end.  The gradients travel as S * g in fp32 with
    S = ``loss_scale`` of k_l * G_l, k_l = upstream / (B*h*w); one host read per pass fetches the upstream gradient and the five
    G_l.  ``last_scale`` holds S of the last backward, ``last_bounds`` its G_l.  Under ``no_grad``, or when ``restored`` needs no
    gradient, nothing is kept.

    CPU: ``composite``, differentiable float64 torch."""

    def __init__(self, lpips_model: LPIPS):
        super().__init__()
        if not isinstance(lpips_model, LPIPS):
            raise TypeError(f"LPIPSLoss: expected an lpips.LPIPS, got {type(lpips_model).__name__}")
        self.lpips = lpips_model
        self.last_scale: Optional[float] = None
        self.last_bounds: Optional[list] = None
        self._bw: dict = {}                      # device -> data-gradient banks: packed once, not per step
        self._trace, self._layers = None, None

    def _apply(self, fn, *a, **kw):
        self._bw.clear()
        return super()._apply(fn, *a, **kw)

    def _bw_packs(self, device):
        from . import ops

        key = str(device)
        if key not in self._bw:
            bw = []
            for (_, _, cin, cout), w in zip(self.lpips.convs, self.lpips.weights):
                gout = (cin + 15) // 16 * 16
                bw.append((ops.pack_conv_train(w.to(device), None, gout, (cout + 31) // 32 * 32, flip_t=True)[0],
                           torch.zeros(gout, dtype=torch.float32, device=device)))
            self._bw[key] = bw
        return self._bw[key]

    def composite(self, x: torch.Tensor, gt: torch.Tensor, operand_dtype=None, grad_scale: Optional[float] = None,
                  decisions: Optional[dict] = None, trace: Optional[list] = None) -> torch.Tensor:
        """The yardstick: differentiable float64 torch, a scalar.  ``operand_dtype``: both operands of every convolution rounded to
        that type (``grad_scale``: the data gradients contract dy rounded to it under that scale as well, ``perceptual._EmuConv``).
        ``decisions`` ({"masks": one boolean [B, C, h, w] per convolution, "pool_idx": the four pools' indices;
        ``decisions_from_trace``): the restored half's ReLUs multiply by these masks and its pools gather these indices; the norm goes
        through ``_safe_norm``, so an all-zero pixel gets the gradient 0 and not NaN.  The target always decides for itself.
        ``trace`` receives the restored half's thirteen pre-ReLU convolution outputs, detached."""
        m = self.lpips
        m._check(x, gt)
        fx = self._trunk(x.double(), operand_dtype, grad_scale, decisions, trace)
        with torch.no_grad():
            fg = self._trunk(gt.detach().double(), operand_dtype, None, None, None)
        total = 0
        for l in range(len(TAPS)):
            total = total + _safe_term(fx[l], fg[l], m.lins[l].double())
        return total.mean()

    def _trunk(self, x, operand_dtype, grad_scale, decisions, trace):
        m = self.lpips
        x = ((2 * x - 1) - m.shift.double()) / m.scale.double()
        masks = list(decisions["masks"]) if decisions is not None else None
        pools = list(decisions["pool_idx"]) if decisions is not None else None
        feats, ci, tap = [], 0, 0
        for pos, name in enumerate(NAMES[: TAP_INDEX[-1] + 1]):
            if name.startswith("conv"):
                w, b = m.weights[ci].double(), m.biases[ci].double()
                if operand_dtype is not None and grad_scale is not None:
                    x = _EmuConv.apply(x, w, b, operand_dtype, float(grad_scale))
                else:
                    x = F.conv2d(_contract(x, operand_dtype), _contract(w, operand_dtype), b, padding=1)
                if trace is not None:
                    trace.append(x.detach())
                ci += 1
            elif name.startswith("relu"):
                x = F.relu(x) if masks is None else x * masks[ci - 1].to(x.dtype)
            elif pools is None:
                x = F.max_pool2d(x, 2, 2)
            else:
                idx = pools.pop(0)
                x = x.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
            if pos == TAP_INDEX[tap]:
                feats.append(x)
                tap += 1
        return feats

    def forward(self, restored: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        self.lpips._check(restored, target)
        if restored.is_cuda:
            return _LpipsFn.apply(restored, target.detach(), self)
        return self.composite(restored, target)

    def forward_traced(self, restored: torch.Tensor, target: torch.Tensor):
        """Tests: (loss, [the five tapped post-ReLU features [2B, C, h, w] of one CUDA forward, the restored images first], [the
        thirteen layer outputs of the restored half [B, C, h, w] that the backward's decisions are read from: the fp32 pre-activation
        at a block closer, the activated 16-bit output elsewhere -- ``> 0`` on either is exactly the backward's mask]).  ``restored``
        must require a gradient."""
        if not restored.is_cuda:
            raise ValueError("forward_traced belongs to the CUDA path; the composite takes trace=")
        self._trace = []
        try:
            loss = self.forward(restored, target)
            B = restored.shape[0]
            layers = [t[: B * h * w].float().view(B, h, w, -1).permute(0, 3, 1, 2) for t, (h, w) in zip(*self._layers)] \
                if self._layers is not None else None
            return loss, self._trace, layers
        finally:
            self._trace, self._layers = None, None
