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

Not built: ``net="alex"`` / ``"squeeze"``, ``spatial=True`` maps, gradients -- LPIPS as a training loss.
"""
import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from .perceptual import MIN_SIDE, _contract, layer_names

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
    def _hip(self, restored: torch.Tensor, target: torch.Tensor, trace: Optional[list] = None) -> torch.Tensor:
        from . import ops

        B, _, H, W = restored.shape
        banks, lins = self._hip_packs(restored.device)
        n0 = B * H * W
        t = ops.empty(2 * n0, 4, dtype=torch.float32, device=restored.device)
        for j, img in enumerate((restored, target)):
            ops.lpips_prep(img.detach().float(), t[j * n0:(j + 1) * n0])
        out = ops.empty(B, dtype=torch.float64, device=restored.device)
        h, w, tap = H, W, 0
        for i, (_, idx, _, _) in enumerate(self.convs):
            wp, bp = banks[i]
            kw = dict(x_cols=4) if i == 0 else {}
            if idx + 1 == TAP_INDEX[tap]:                                       # a block closer: fp32, what the tap kernel reads
                f = ops.conv3x3(t, wp, bp, 2 * B, h, w, **kw)
                last = tap == len(TAPS) - 1
                t = ops.lpips_tap(f, lins[tap], B, h, w, out, accumulate=tap > 0, pool=not last)
                if trace is not None:
                    trace.append(torch.relu(f).view(2 * B, h, w, -1).permute(0, 3, 1, 2))
                h, w, tap = h // 2, w // 2, tap + 1
            else:
                t = ops.conv3x3(t, wp, bp, 2 * B, h, w, act=2, slope=0.0, out_dtype=ops.GEMM_DTYPE, **kw)   # ReLU rides in the epilogue
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
