"""The spectrally normalised U-Net discriminator of the real-world SR GAN stage (config/experiment/bsr/grl.yaml).

  replaces  UNetDiscriminatorSN                    models/aux_archs/discriminator.py:92-144
            torch.nn.utils.spectral_norm on conv1 .. conv8 (one power iteration per training forward)

Parameter and buffer names are the reference's -- ``conv0.weight``, ``conv0.bias``, ``convN.weight_orig`` / ``weight_u`` /
``weight_v`` (N = 1..8), ``conv9.weight``, ``conv9.bias`` -- so a reference ``bsr_discriminator_checkpoint`` loads with
``strict=True`` (28 keys).

CUDA tensors: every contraction is a launch of libgrl_hip.so -- torch.ops.grl.conv3x3_lrelu (3x3), torch.ops.grl.conv4x4s2 (the
encoder's 4x4 stride-2 convolutions) and torch.ops.grl.upsample2x (the decoder's bilinear x2), forward and backward (autograd.py).
LeakyReLU(0.2) rides in the convolutions' epilogues.  The spectral normalisation of the eight layers is ONE call of
autograd.SpectralNormFn per forward (grl_spectral_norm_fwd: three launches for the power iteration, sigma and W / sigma of all
layers; grl_spectral_norm_bwd: two), without atomics: replicas that hold the same weights keep bit-identical ``weight_u`` /
``weight_v`` with no broadcast (gan.GanStep(process_group=...)).  The skip additions are torch glue.  CPU tensors take
``composite_forward`` and ``_SNConv.weight()``: plain differentiable torch in the parameters' dtype (float64-capable), the
yardstick of the GPU tests; it is not a fallback for the GPU path.
"""
import math
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

SLOPE = 0.2


class _Conv(nn.Module):
    """Holder of a plain convolution's parameters (conv0, conv9: 3x3 with bias)."""

    def __init__(self, cin: int, cout: int, k: int, bias: bool):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))             # nn.Conv2d.reset_parameters
        if bias:
            bound = 1.0 / math.sqrt(cin * k * k)
            self.bias = nn.Parameter(torch.empty(cout).uniform_(-bound, bound))
        else:
            self.register_parameter("bias", None)


class _SNConv(nn.Module):
    """A bias-free convolution under torch.nn.utils.spectral_norm, restated value for value (torch/nn/utils/spectral_norm.py):
    W = weight_orig.reshape(Cout, -1); training forward: v <- normalize(W^T u), u <- normalize(W v) under no_grad, in place;
    sigma = u . (W v) with u, v constants; weight = weight_orig / sigma."""

    def __init__(self, cin: int, cout: int, k: int):
        super().__init__()
        self.weight_orig = nn.Parameter(torch.empty(cout, cin, k, k))
        nn.init.kaiming_uniform_(self.weight_orig, a=math.sqrt(5))
        self.register_buffer("weight_u", F.normalize(torch.randn(cout), dim=0, eps=1e-12))
        self.register_buffer("weight_v", F.normalize(torch.randn(cin * k * k), dim=0, eps=1e-12))

    def weight(self) -> torch.Tensor:
        w = self.weight_orig
        wm = w.reshape(w.shape[0], -1)
        u, v = self.weight_u, self.weight_v
        if self.training:
            with torch.no_grad():
                v = F.normalize(torch.mv(wm.t(), u), dim=0, eps=1e-12, out=v)
                u = F.normalize(torch.mv(wm, v), dim=0, eps=1e-12, out=u)
                u, v = u.clone(memory_format=torch.contiguous_format), v.clone(memory_format=torch.contiguous_format)
        sigma = torch.dot(u, torch.mv(wm, v))
        return w / sigma


def spectral_norm_grad(g: torch.Tensor, w: torch.Tensor, u: torch.Tensor, v: torch.Tensor, sigma: torch.Tensor) -> torch.Tensor:
    """The derivative of ``w / sigma(w)``, sigma = u . (W v) with u and v held constant as in ``_SNConv.weight()``, for the output
    gradient ``g``, in closed form: dW = g / sigma - (<g, w> / sigma^2) u v^T.  What grl_spectral_norm_bwd evaluates
    (include/grl_hip.h), stated in torch in the arguments' dtype: the float64 yardstick of that kernel
    (tests/test_spectral_norm.py holds it against autograd through ``_SNConv.weight()``)."""
    return g / sigma - ((g * w).sum() / sigma ** 2) * torch.outer(u, v).view_as(w)


def _contract(t: torch.Tensor, operand_dtype: Optional[torch.dtype]) -> torch.Tensor:
    """``operand_dtype``: the value the kernels' loaders contract -- rounded to that type -- carried on in float64."""
    return t if operand_dtype is None else t.to(operand_dtype).to(torch.float64)


def conv4x4s2_composite(x, w, operand_dtype=None):
    return F.conv2d(_contract(x, operand_dtype), _contract(w, operand_dtype), None, stride=2, padding=1)


def conv3x3_composite(x, w, b=None, operand_dtype=None):
    return F.conv2d(_contract(x, operand_dtype), _contract(w, operand_dtype), b, stride=1, padding=1)


def upsample2x_composite(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)


class UNetDiscriminatorSN(nn.Module):
    def __init__(self, num_in_ch: int = 3, num_feat: int = 64, skip_connection: bool = True):
        super().__init__()
        if num_feat % 4:
            raise ValueError("num_feat must be a multiple of 4 (the kernels move channels in 16-byte pieces)")
        self.skip_connection = skip_connection
        nf = num_feat
        self.conv0 = _Conv(num_in_ch, nf, 3, bias=True)
        self.conv1 = _SNConv(nf, nf * 2, 4)
        self.conv2 = _SNConv(nf * 2, nf * 4, 4)
        self.conv3 = _SNConv(nf * 4, nf * 8, 4)
        self.conv4 = _SNConv(nf * 8, nf * 4, 3)
        self.conv5 = _SNConv(nf * 4, nf * 2, 3)
        self.conv6 = _SNConv(nf * 2, nf, 3)
        self.conv7 = _SNConv(nf, nf, 3)
        self.conv8 = _SNConv(nf, nf, 3)
        self.conv9 = _Conv(nf, 1, 3, bias=True)

    def _weights(self, chain: bool = False):
        """The eight normalised weights of this forward, in layer order (advances u / v in training mode).  CUDA parameters: one
        call of the HIP kernels for the eight layers; ``chain=True`` takes the torch chain of ``_SNConv.weight()`` there as well, the
        form the kernels replaced (tools/bench_disc.py --sn measures the two against each other by rebinding this method).  CPU parameters always take the chain."""
        convs = [getattr(self, f"conv{i}") for i in range(1, 9)]
        if chain or not convs[0].weight_orig.is_cuda:
            return [c.weight() for c in convs]
        from . import autograd as AG

        return AG.spectral_norm([c.weight_orig for c in convs], [c.weight_u for c in convs], [c.weight_v for c in convs], self.training)

    def forward(self, x: torch.Tensor, operand_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """x [B, C, H, W] (H, W multiples of 8) -> logits [B, 1, H, W].  ``operand_dtype`` (CPU only): emulate the kernels' operand
        rounding -- both operands of every convolution rounded to that type, float64 accumulation; used to derive test tolerances."""
        return self._forward_traced(x, operand_dtype)

    def _forward_traced(self, x, operand_dtype=None, acts=None, masks=None):
        """``forward`` with the LeakyReLU decisions in view (tests).  ``acts``: a list that receives the nine LeakyReLU outputs
        [B, C, h, w] (before the skip additions), detached.  ``masks`` (CPU only): nine boolean tensors; LeakyReLU takes slope 1
        where True and 0.2 elsewhere instead of looking at its own argument's sign.  The derivative of LeakyReLU jumps at 0, so two
        runs in different arithmetic have comparable GRADIENTS only under the same masks."""
        if x.dim() != 4 or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"UNetDiscriminatorSN: H and W must be multiples of 8 (got {tuple(x.shape)})")
        if x.is_cuda:
            if operand_dtype is not None or masks is not None:
                raise ValueError("operand_dtype and masks belong to the CPU composite path")
            return self._forward_hip(x, acts)
        return self.composite_forward(x, operand_dtype, acts, masks)

    def composite_forward(self, x, operand_dtype=None, acts=None, masks=None):
        w = self._weights()
        od = operand_dtype
        todo = list(masks) if masks is not None else None

        def act(t):
            y = F.leaky_relu(t, SLOPE) if todo is None else t * torch.where(todo.pop(0), 1.0, SLOPE).to(t.dtype)
            if acts is not None:
                acts.append(y.detach())
            return y

        x0 = act(conv3x3_composite(x, self.conv0.weight, self.conv0.bias, od))
        x1 = act(conv4x4s2_composite(x0, w[0], od))
        x2 = act(conv4x4s2_composite(x1, w[1], od))
        x3 = act(conv4x4s2_composite(x2, w[2], od))
        x3 = upsample2x_composite(x3)
        x4 = act(conv3x3_composite(x3, w[3], None, od))
        if self.skip_connection:
            x4 = x4 + x2
        x4 = upsample2x_composite(x4)
        x5 = act(conv3x3_composite(x4, w[4], None, od))
        if self.skip_connection:
            x5 = x5 + x1
        x5 = upsample2x_composite(x5)
        x6 = act(conv3x3_composite(x5, w[5], None, od))
        if self.skip_connection:
            x6 = x6 + x0
        out = act(conv3x3_composite(x6, w[6], None, od))
        out = act(conv3x3_composite(out, w[7], None, od))
        return conv3x3_composite(out, self.conv9.weight, self.conv9.bias, od)

    def _forward_hip(self, x, acts=None):
        from . import autograd as AG      # (loads the HIP library; a missing kernel is an error, never a fallback)

        B, C_, H, W = x.shape
        w = self._weights()
        up = torch.ops.grl.upsample2x

        def keep(t, h, w_):
            if acts is not None:
                acts.append(t.detach().view(B, h, w_, -1).permute(0, 3, 1, 2))
            return t

        def c3(t, wt, b, B_, h, w_, slope):
            y = torch.ops.grl.conv3x3_lrelu(t, wt, b, B_, h, w_, slope)
            return keep(y, h, w_) if slope != 1.0 else y

        def c4(t, wt, B_, h, w_, slope):
            return keep(torch.ops.grl.conv4x4s2(t, wt, B_, h, w_, slope), h // 2, w_ // 2)

        t = x.float().permute(0, 2, 3, 1).reshape(B * H * W, C_)
        t0 = c3(t, self.conv0.weight, self.conv0.bias, B, H, W, SLOPE)
        t1 = c4(t0, w[0], B, H, W, SLOPE)
        t2 = c4(t1, w[1], B, H // 2, W // 2, SLOPE)
        t3 = c4(t2, w[2], B, H // 4, W // 4, SLOPE)
        t4 = c3(up(t3, B, H // 8, W // 8), w[3], None, B, H // 4, W // 4, SLOPE)
        if self.skip_connection:
            t4 = t4 + t2
        t5 = c3(up(t4, B, H // 4, W // 4), w[4], None, B, H // 2, W // 2, SLOPE)
        if self.skip_connection:
            t5 = t5 + t1
        t6 = c3(up(t5, B, H // 2, W // 2), w[5], None, B, H, W, SLOPE)
        if self.skip_connection:
            t6 = t6 + t0
        o = c3(t6, w[6], None, B, H, W, SLOPE)
        o = c3(o, w[7], None, B, H, W, SLOPE)
        o = c3(o, self.conv9.weight, self.conv9.bias, B, H, W, 1.0)
        y = o.view(B, H, W, 1).permute(0, 3, 1, 2)
        return AG.GradScaleTop.apply(y)      # (the gradient operand scale of the fp16 backward contractions, autograd.py)
