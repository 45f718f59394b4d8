"""The discriminator's HIP kernels (csrc/disc.hip, grl_gemm_tn taps = 16) and the whole U-Net discriminator on the GPU against the
float64 composite on the CPU (discriminator.py).

Tolerances.  Convolutions and the whole network: 4 x the max-abs error of the composite's own ``operand_dtype=float16`` emulation
against float64 on the same case, computed here on the CPU per compared tensor (the factor 4 covers fp32 accumulation and summation
order, which the emulation does not have).  Upsampling: the weights are exact in fp32 and an output is a four-term sum, so
8 * 2^-24 * max|x|; its adjoint sums up to 16 terms: four times that.  u / v: the two fp32 mat-vecs of a power iteration,
2 * K * 2^-24 with K the longer side of the weight matrix.  Every measured figure is printed next to its bound.

LeakyReLU's backward mask is the sign of the kernel's OWN output, so where a pre-activation lies within rounding of zero the GPU and
a float64 run may choose different slopes, and a gradient then differs by 0.8 x a whole term -- nothing an operand-rounding
emulation bounds.  (First GPU run, whole network at num_feat 64 on (1, 3, 8, 8), every run under its own masks: conv3.weight_orig
was 4.4e-5 off against an emulation error of 1.5e-6 -- one channel of the 1 x 1 x 512 bottleneck on the other side of zero -- while
all kernel-level checks sat on the emulation to four digits.)  The kernel-level gradient checks therefore run without the activation,
the masked backward is checked against the float64 adjoint taken with the mask of the GPU's own forward output, and the whole-network
GRADIENT checks hand the GPU run's masks to the float64 run and to the emulation (``_forward_traced(acts=..., masks=...)``); logits
are compared with every run under its own masks.  That the GPU's masks are the float64 run's own masks up to rounding is asserted
per layer (``check_masks``): they may differ only where the float64 pre-activation lies within 4 x the emulation's error of that
layer's pre-activations, and at no more than max(4, 1 %) of the layer's elements -- the emulation error is about 1e-3 of the
pre-activations' spread, so a band of that width around zero holds a few tenths of a percent of them, and a sign flips for fewer still.

The adjoint identity of the upsampling is a sanity check only: its bound adds the element bounds over the l1 norm of the other
factor and comes out 1e3 to 1e4 times the measured figure.  The check that would catch a wrong weight at an edge is the backward
against autograd of the composite, at 32 * 2^-24 * max|dy|.

Measured on MI355X (2026-10-19; of the whole network the logits, the input gradient and two of the parameter gradients are listed):
  conv4x4s2 fwd (2, 64, 128, 8, 24) act=False: gpu 1.231e-03  emu 1.231e-03  bound 4.926e-03
  conv4x4s2 fwd (2, 64, 128, 8, 24) act=True: gpu 1.008e-03  emu 1.008e-03  bound 4.032e-03
  conv4x4s2 dx (2, 64, 128, 8, 24): gpu 8.292e-08  emu 8.293e-08  bound 3.317e-07
  conv4x4s2 dW (2, 64, 128, 8, 24): gpu 1.577e-06  emu 1.577e-06  bound 6.309e-06
  conv4x4s2 masked dx (2, 64, 128, 8, 24): gpu 5.877e-08  emu 5.876e-08  bound 2.350e-07
  conv4x4s2 masked dW (2, 64, 128, 8, 24): gpu 1.208e-06  emu 1.208e-06  bound 4.831e-06
  conv4x4s2 fwd (1, 8, 16, 2, 2) act=False: gpu 2.904e-04  emu 2.904e-04  bound 1.161e-03
  conv4x4s2 fwd (1, 8, 16, 2, 2) act=True: gpu 2.904e-04  emu 2.904e-04  bound 1.161e-03
  conv4x4s2 dx (1, 8, 16, 2, 2): gpu 2.158e-08  emu 2.158e-08  bound 8.631e-08
  conv4x4s2 dW (1, 8, 16, 2, 2): gpu 1.485e-07  emu 1.485e-07  bound 5.941e-07
  conv4x4s2 masked dx (1, 8, 16, 2, 2): gpu 1.460e-08  emu 1.460e-08  bound 5.839e-08
  conv4x4s2 masked dW (1, 8, 16, 2, 2): gpu 1.355e-07  emu 1.355e-07  bound 5.418e-07
  conv4x4s2 fwd (1, 64, 128, 40, 72) act=False: gpu 1.256e-03  emu 1.256e-03  bound 5.024e-03
  conv4x4s2 fwd (1, 64, 128, 40, 72) act=True: gpu 1.256e-03  emu 1.256e-03  bound 5.024e-03
  conv4x4s2 dx (1, 64, 128, 40, 72): gpu 9.625e-08  emu 9.627e-08  bound 3.851e-07
  conv4x4s2 dW (1, 64, 128, 40, 72): gpu 3.535e-06  emu 3.535e-06  bound 1.414e-05
  conv4x4s2 masked dx (1, 64, 128, 40, 72): gpu 7.226e-08  emu 7.226e-08  bound 2.890e-07
  conv4x4s2 masked dW (1, 64, 128, 40, 72): gpu 2.525e-06  emu 2.525e-06  bound 1.010e-05
  conv4x4s2 fwd (1, 256, 512, 8, 8) act=False: gpu 1.081e-03  emu 1.081e-03  bound 4.325e-03
  conv4x4s2 fwd (1, 256, 512, 8, 8) act=True: gpu 1.081e-03  emu 1.081e-03  bound 4.325e-03
  conv4x4s2 dx (1, 256, 512, 8, 8): gpu 7.954e-08  emu 7.952e-08  bound 3.181e-07
  conv4x4s2 dW (1, 256, 512, 8, 8): gpu 9.471e-07  emu 9.471e-07  bound 3.788e-06
  conv4x4s2 masked dx (1, 256, 512, 8, 8): gpu 5.975e-08  emu 5.974e-08  bound 2.390e-07
  conv4x4s2 masked dW (1, 256, 512, 8, 8): gpu 8.180e-07  emu 8.181e-07  bound 3.272e-06
  upsample2x fwd (2, 16, 3, 5): max|d| 1.490e-07 bound 1.370e-06
  upsample2x bwd (2, 16, 3, 5): max|d| 3.967e-07 bound 6.690e-06
  upsample2x adjoint (2, 16, 3, 5): |<up x, y> - <x, up^T y>| 4.934e-07 bound 4.528e-03
  upsample2x fwd (1, 64, 1, 1): max|d| 0.000e+00 bound 1.041e-06
  upsample2x bwd (1, 64, 1, 1): max|d| 2.384e-07 bound 5.370e-06
  upsample2x adjoint (1, 64, 1, 1): |<up x, y> - <x, up^T y>| 5.243e-08 bound 4.531e-04
  upsample2x fwd (1, 8, 9, 33): max|d| 1.919e-07 bound 1.623e-06
  upsample2x bwd (1, 8, 9, 33): max|d| 3.339e-07 bound 7.360e-06
  upsample2x adjoint (1, 8, 9, 33): |<up x, y> - <x, up^T y>| 3.552e-06 bound 2.602e-02
  nf64 (2, 3, 32, 48) eval logits: gpu 9.325e-05  emu 1.097e-04  bound 4.387e-04
  nf64 (2, 3, 32, 48) train logits: gpu 8.455e-05  emu 8.063e-05  bound 3.225e-04
  nf64 (2, 3, 32, 48) grad conv3.weight_orig: gpu 3.065e-07  emu 6.233e-07  bound 2.493e-06
  nf64 (2, 3, 32, 48) grad conv8.weight_orig: gpu 7.418e-06  emu 3.579e-05  bound 1.431e-04
  nf64 (2, 3, 32, 48) input gradient: gpu 1.591e-08  emu 2.515e-07  bound 1.006e-06
  nf64 (1, 3, 8, 8) eval logits: gpu 5.575e-05  emu 5.691e-05  bound 2.277e-04
  nf64 (1, 3, 8, 8) train logits: gpu 4.274e-05  emu 3.841e-05  bound 1.536e-04
  nf64 (1, 3, 8, 8) grad conv3.weight_orig: gpu 1.566e-07  emu 1.690e-07  bound 6.761e-07
  nf64 (1, 3, 8, 8) grad conv8.weight_orig: gpu 6.316e-06  emu 2.109e-05  bound 8.436e-05
  nf64 (1, 3, 8, 8) input gradient: gpu 4.564e-07  emu 5.219e-07  bound 2.087e-06
  nf8 (2, 3, 16, 24) eval logits: gpu 5.052e-05  emu 4.278e-05  bound 1.711e-04
  nf8 (2, 3, 16, 24) train logits: gpu 4.080e-05  emu 4.201e-05  bound 1.681e-04
  nf8 (2, 3, 16, 24) grad conv3.weight_orig: gpu 9.079e-08  emu 1.661e-07  bound 6.643e-07
  nf8 (2, 3, 16, 24) grad conv8.weight_orig: gpu 4.536e-06  emu 9.491e-06  bound 3.796e-05
  nf8 (2, 3, 16, 24) input gradient: gpu 6.021e-08  emu 8.931e-08  bound 3.572e-07
  masks, worst layer of each case: nf64 (2, 3, 32, 48) 34 of 196608 differ, largest |pre-activation| there 2.5e-04 (allowed 1.5e-03);
  nf64 (1, 3, 8, 8) 1 of 512, 7.9e-06 (1.5e-04); nf8 (2, 3, 16, 24) 2 of 1536, 5.7e-05 (7.6e-04)
"""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
SLOPE = 0.2
SN = [f"conv{i}" for i in range(1, 9)]


def r16(t):
    return t.to(torch.float16).to(torch.float64)


def tokens(t):      # [B, C, H, W] -> [B*H*W, C]
    B, C_, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, C_).contiguous()


def image(t, B, H, W):
    return t.view(B, H, W, -1).permute(0, 3, 1, 2)


def report(what, got, want, emu):
    err = float((got.detach().double().cpu() - want).abs().max())
    bound = 4.0 * float((emu - want).abs().max())
    print(f"{what}: max|gpu - fp64| {err:.3e}  emulation {bound / 4:.3e}  bound {bound:.3e}  (max|ref| {float(want.abs().max()):.3e})")
    return err, bound


def check_masks(what, gpu_acts, acts64, acts_emu):
    """The GPU run's LeakyReLU decisions against the float64 run's own, layer by layer (module docstring)."""
    pre = lambda y: torch.where(y > 0, y, y / SLOPE)       # the slope is positive: the activation determines its argument
    assert len(gpu_acts) == len(acts64) == len(acts_emu) == 9
    for i, (g, a, e) in enumerate(zip(gpu_acts, acts64, acts_emu)):
        tol = 4.0 * float((pre(e) - pre(a)).abs().max())
        flip = (g.cpu() > 0) != (a > 0)
        n = int(flip.sum())
        worst = float(pre(a)[flip].abs().max()) if n else 0.0
        print(f"{what} layer {i}: {n} of {a.numel()} masks differ, largest |pre-activation| there {worst:.3e}  (allowed {tol:.3e})")
        assert worst <= tol and n <= max(4, a.numel() // 100), (what, i, n, worst, tol)


def check(what, got, want, emu):
    err, bound = report(what, got, want, emu)
    assert err <= bound, (what, err, bound)


CONV_CASES = [(2, 64, 128, 8, 24), (1, 8, 16, 2, 2), (1, 64, 128, 40, 72), (1, 256, 512, 8, 8)]


@pytest.fixture(scope="module", params=CONV_CASES, ids=lambda c: "B{}_{}to{}_{}x{}".format(*c))
def conv_case(request):
    """Inputs and the float64 / emulated references of one shape, computed once."""
    B, Cin, Cout, H, W = request.param
    g = torch.Generator().manual_seed(B * 1000 + Cin + H)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 4, 4, generator=g) / (16 * Cin) ** 0.5
    dy = torch.randn(B, Cout, H // 2, W // 2, generator=g) * 1e-4          # gradients of a mean-reduced loss are small
    x64, w64, dy64 = x.double(), w.double(), dy.double()
    conv = lambda a, b: F.conv2d(a, b, None, stride=2, padding=1)
    ref = conv(x64, w64)
    emu = conv(r16(x64), r16(w64))
    return dict(shape=request.param, x=x, w=w, dy=dy, x64=x64, w64=w64, dy64=dy64, ref=ref, emu=emu, conv=conv)


def _scaled16(dy64):
    """dy as the backward kernels contract it: times the power of two of autograd.GradScaleTop, to fp16, divided again."""
    import math

    s = 2.0 ** math.floor(math.log2(64.0 / float(dy64.abs().max())))
    return r16(dy64 * s) / s


def _grads64(c, dy_eff):
    """(dx, dw) in float64 and their operand-rounded emulations for output gradient dy_eff."""
    xr, wr = c["x64"].clone().requires_grad_(True), c["w64"].clone().requires_grad_(True)
    dx, dw = torch.autograd.grad(c["conv"](xr, wr), (xr, wr), dy_eff)
    d16 = _scaled16(dy_eff)
    dx_e, = torch.autograd.grad(c["conv"](xr, r16(c["w64"])), xr, d16)
    dw_e, = torch.autograd.grad(c["conv"](r16(c["x64"]), wr), wr, d16)
    return dx, dw, dx_e, dw_e


@pytest.mark.parametrize("act", [False, True])
def test_conv4x4s2_forward(conv_case, act):
    import grl_image_restoration_amd.autograd  # noqa: F401  (registers torch.ops.grl)

    c = conv_case
    B, Cin, Cout, H, W = c["shape"]
    y = torch.ops.grl.conv4x4s2(tokens(c["x"]).cuda(), c["w"].cuda(), B, H, W, SLOPE if act else 1.0)
    assert y.shape == (B * (H // 2) * (W // 2), Cout)
    f = (lambda t: F.leaky_relu(t, SLOPE)) if act else (lambda t: t)
    check(f"conv4x4s2 fwd {c['shape']} act={act}", image(y, B, H // 2, W // 2), f(c["ref"]), f(c["emu"]))


def test_conv4x4s2_gradients(conv_case):
    from grl_image_restoration_amd import autograd as AG

    c = conv_case
    B, Cin, Cout, H, W = c["shape"]
    xt, w = tokens(c["x"]).cuda().requires_grad_(True), c["w"].cuda().requires_grad_(True)
    y = AG.GradScaleTop.apply(torch.ops.grl.conv4x4s2(xt, w, B, H, W))
    y.backward(tokens(c["dy"]).cuda())
    assert AG.grad_scale(xt.device) > 1.0                                   # the operand scale was taken from this dy
    dx, dw, dx_e, dw_e = _grads64(c, c["dy64"])
    check(f"conv4x4s2 dx {c['shape']}", image(xt.grad, B, H, W), dx, dx_e)
    check(f"conv4x4s2 dW {c['shape']}", w.grad, dw, dw_e)


def test_conv4x4s2_masked_backward(conv_case):
    """LeakyReLU in the epilogue: the backward uses the mask of the forward's own output."""
    from grl_image_restoration_amd import autograd as AG

    c = conv_case
    B, Cin, Cout, H, W = c["shape"]
    xt, w = tokens(c["x"]).cuda().requires_grad_(True), c["w"].cuda().requires_grad_(True)
    y0 = torch.ops.grl.conv4x4s2(xt, w, B, H, W, SLOPE)
    AG.GradScaleTop.apply(y0).backward(tokens(c["dy"]).cuda())
    mask = image(torch.where(y0.detach() > 0, 1.0, SLOPE).double().cpu(), B, H // 2, W // 2)
    dx, dw, dx_e, dw_e = _grads64(c, c["dy64"] * mask)
    check(f"conv4x4s2 masked dx {c['shape']}", image(xt.grad, B, H, W), dx, dx_e)
    check(f"conv4x4s2 masked dW {c['shape']}", w.grad, dw, dw_e)


@pytest.mark.parametrize("shape", [(2, 16, 3, 5), (1, 64, 1, 1), (1, 8, 9, 33)], ids=lambda s: "B{}_C{}_{}x{}".format(*s))
def test_upsample2x_forward_backward_adjoint(shape):
    import grl_image_restoration_amd.autograd  # noqa: F401

    B, C_, H, W = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    x, yv = torch.randn(B, C_, H, W, generator=g), torch.randn(B, C_, 2 * H, 2 * W, generator=g)
    up64 = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)
    xt = tokens(x).cuda().requires_grad_(True)
    o = torch.ops.grl.upsample2x(xt, B, H, W)
    err = float((image(o.detach().cpu().double(), B, 2 * H, 2 * W) - up64(x.double())).abs().max())
    bound = 8 * U * float(x.abs().max())
    print(f"upsample2x fwd {shape}: max|d| {err:.3e} bound {bound:.3e}")
    assert err <= bound
    o.backward(tokens(yv).cuda())
    dx = image(xt.grad.cpu().double(), B, H, W)
    x64 = x.double().requires_grad_(True)
    want, = torch.autograd.grad(up64(x64), x64, yv.double())
    errb, boundb = float((dx - want).abs().max()), 4 * 8 * U * float(yv.abs().max())
    print(f"upsample2x bwd {shape}: max|d| {errb:.3e} bound {boundb:.3e}")
    assert errb <= boundb
    # <up(x), y> = <x, up^T(y)>: each side's error is its element bound times the l1 norm of the other factor -- a worst-case sum,
    # 1e3 to 1e4 times what is measured: a sanity check of the pairing; the tight check of the backward is the one above
    a = float((image(o.detach().cpu().double(), B, 2 * H, 2 * W) * yv.double()).sum())
    b = float((dx * x.double()).sum())
    bounda = 8 * U * float(x.abs().max()) * float(yv.abs().sum()) + 4 * 8 * U * float(yv.abs().max()) * float(x.abs().sum())
    print(f"upsample2x adjoint {shape}: |<up x, y> - <x, up^T y>| {abs(a - b):.3e} bound {bounda:.3e}")
    assert abs(a - b) <= bounda


def _warm(d):
    """u / v as a trained checkpoint has them (a fresh random pair gives sigma near zero)."""
    d.train()
    with torch.no_grad():
        for _ in range(5):
            d(torch.zeros(1, 3, 8, 8, dtype=next(d.parameters()).dtype))
    return d


def _fixture_state():
    z = np.load(os.path.join(HERE, "golden", "gan", "disc.npz"), allow_pickle=False)
    sd = {k[len("d__p__"):]: torch.from_numpy(z[k].astype(np.float64)) for k in z.files if k.startswith("d__p__")}
    for c in SN:
        sd[f"{c}.weight_u"], sd[f"{c}.weight_v"] = torch.from_numpy(z[f"d__u0__{c}"]), torch.from_numpy(z[f"d__v0__{c}"])
    return sd, z


@pytest.fixture(scope="module")
def nets():
    return build_nets()


def build_nets():
    """num_feat -> float64 state dict (64: seeded init with warmed u / v; 8: the reference fixture's)."""
    from grl_image_restoration_amd.discriminator import UNetDiscriminatorSN

    torch.manual_seed(3)
    d = _warm(UNetDiscriminatorSN(3, 64, True))
    return {64: {k: v.double() for k, v in d.state_dict().items()}, 8: _fixture_state()[0]}


def _pair(nets, nf):
    from grl_image_restoration_amd.discriminator import UNetDiscriminatorSN

    cpu = UNetDiscriminatorSN(3, nf, True).double()
    cpu.load_state_dict(nets[nf], strict=True)
    gpu = copy.deepcopy(cpu).float().cuda()
    return cpu, gpu


def _bce(z, real):
    from grl_image_restoration_amd.gan import gan_loss

    return gan_loss(z, real, is_disc=True)


@pytest.mark.parametrize("nf,shape", [(64, (2, 3, 32, 48)), (64, (1, 3, 8, 8)), (8, (2, 3, 16, 24))], ids=["nf64_32x48", "nf64_8x8", "nf8_fixture"])
def test_whole_discriminator(nets, nf, shape):
    g = torch.Generator().manual_seed(shape[2])
    x, xf = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if nf == 8:                                            # the reference's own case A
        z = _fixture_state()[1]
        x, xf = torch.from_numpy(z["d__A__x"]), torch.from_numpy(z["d__A__xf"])
    x64, xf64 = x.double(), xf.double()
    # eval logits
    cpu, gpu = _pair(nets, nf)
    cpu.eval(), gpu.eval()
    with torch.no_grad():
        ref, emu, got = cpu(x64), cpu(x64, operand_dtype=torch.float16), gpu(x.cuda())
    check(f"nf{nf} {shape} eval logits", got, ref, emu)
    if nf == 8:
        e = float((ref - torch.from_numpy(z["d__A__eval"])).abs().max())
        assert e <= 1e-10, e                               # the yardstick is the reference's own run
    # train logits, u / v
    cpu, gpu = _pair(nets, nf)
    emu_net = copy.deepcopy(cpu)
    with torch.no_grad():
        ref, emu, got = cpu(x64), emu_net(x64, operand_dtype=torch.float16), gpu(x.cuda())
    check(f"nf{nf} {shape} train logits", got, ref, emu)
    for c in SN:
        m = getattr(cpu, c)
        K = max(m.weight_orig.shape[0], m.weight_orig[0].numel())
        for b in ("weight_u", "weight_v"):
            err = float((getattr(getattr(gpu, c), b).double().cpu() - getattr(m, b)).abs().max())
            assert err <= 2 * K * U, (c, b, err)
    # D loss gradients with respect to every parameter
    cpu, gpu = _pair(nets, nf)
    emu_net, own64, own_emu = copy.deepcopy(cpu), copy.deepcopy(cpu), copy.deepcopy(cpu)
    a1, a2 = [], []
    (_bce(gpu._forward_traced(x.cuda(), acts=a1), True) + _bce(gpu._forward_traced(xf.cuda(), acts=a2), False)).backward()
    m1, m2 = [(t > 0).cpu() for t in a1], [(t > 0).cpu() for t in a2]
    assert len(m1) == 9 and len(m2) == 9
    o1, o2, e1, e2 = [], [], [], []
    with torch.no_grad():                                  # the same two forwards, each run under its own masks
        own64._forward_traced(x64, acts=o1), own64._forward_traced(xf64, acts=o2)
        own_emu._forward_traced(x64, torch.float16, acts=e1), own_emu._forward_traced(xf64, torch.float16, acts=e2)
    check_masks(f"nf{nf} {shape} real", a1, o1, e1)
    check_masks(f"nf{nf} {shape} fake", a2, o2, e2)
    (_bce(cpu._forward_traced(x64, masks=m1), True) + _bce(cpu._forward_traced(xf64, masks=m2), False)).backward()
    (_bce(emu_net._forward_traced(x64, torch.float16, masks=m1), True) + _bce(emu_net._forward_traced(xf64, torch.float16, masks=m2), False)).backward()
    fails = []
    pe = dict(emu_net.named_parameters())
    pg = dict(gpu.named_parameters())
    for k, p in cpu.named_parameters():
        err, bound = report(f"nf{nf} {shape} grad {k}", pg[k].grad, p.grad, pe[k].grad)
        if err > bound:
            fails.append((k, err, bound))
    # generator-side loss: gradient with respect to the input, the discriminator's parameters off
    cpu, gpu = _pair(nets, nf)
    emu_net = copy.deepcopy(cpu)
    for n in (cpu, emu_net, gpu):
        for p in n.parameters():
            p.requires_grad_(False)
    xa, xb, xc = x64.clone().requires_grad_(True), x64.clone().requires_grad_(True), x.cuda().requires_grad_(True)
    a1 = []
    _bce(gpu._forward_traced(xc, acts=a1), True).backward()
    m1 = [(t > 0).cpu() for t in a1]
    _bce(cpu._forward_traced(xa, masks=m1), True).backward()
    _bce(emu_net._forward_traced(xb, torch.float16, masks=m1), True).backward()
    assert all(p.grad is None for p in gpu.parameters())
    err, bound = report(f"nf{nf} {shape} input gradient", xc.grad, xa.grad, xb.grad)
    if err > bound:
        fails.append(("input", err, bound))
    assert not fails, fails


def test_every_contraction_is_a_launch_of_this_library(nets):
    """With the launch profile on, a forward and backward on CUDA tensors issues one named launch per layer and direction."""
    from grl_image_restoration_amd import ops

    _, gpu = _pair(nets, 8)
    x = torch.rand(1, 3, 16, 24).cuda().requires_grad_(True)
    ops.profile_begin()
    try:
        _bce(gpu(x), True).backward()
    finally:
        rec = ops.profile_end()
    count = lambda prefix: sum(len(v) for k, v in rec.items() if k.split(" ")[0] == prefix)
    print({k: len(v) for k, v in rec.items()})
    assert count("conv4x4s2") == 3 and count("conv4x4s2_bwd_data") == 3          # conv1..3, forward and data gradient
    assert count("upsample2x_bilinear_fwd") == 3 and count("upsample2x_bilinear_bwd") == 3
    assert count("conv3x3") == 14                                                # conv0, conv4..9: forward + data gradient
    assert count("gemm_tn") == 10                                                # every weight gradient (3 of them 16-tap)
    shapes = {k for k in rec if k.startswith("conv4x4s2 ")}
    assert shapes == {"conv4x4s2 32->16 16x24", "conv4x4s2 32->32 8x12", "conv4x4s2 32->64 4x6"}, shapes


def test_bad_arguments_are_refused_before_any_launch():
    from grl_image_restoration_amd import _lib as L
    from grl_image_restoration_amd import ops

    x = torch.randn(1 * 6 * 8, 32, device="cuda")
    w = ops.pack_conv4x4(torch.randn(16, 32, 4, 4, device="cuda"), 16, 32)
    out = torch.full((1 * 3 * 4, 16), 7.0, device="cuda")

    def args(**kw):
        base = dict(x=C.c_void_p(x.data_ptr()), x_dtype=L.DT_F32, ldx=32, w=C.c_void_p(w.data_ptr()), w_tap_stride=16 * 32, B=1, H=6, W=8,
                    CinP=32, CoutP=16, out=C.c_void_p(out.data_ptr()), out_dtype=L.DT_F32, ldo=16, x_cols=32, n_store=16)
        base.update(kw)
        return L.GrlConvArgs(**base)

    s = L.stream_ptr()
    for fn in (L.lib().grl_conv4x4s2_fwd, L.lib().grl_conv4x4s2_bwd_data):
        assert fn(s, C.byref(args(H=5))) == -2                        # odd H: unsupported shape
        assert fn(s, C.byref(args(W=7))) == -2
        assert fn(s, C.byref(args(ldx=34))) == -1                     # rows not in 16-byte pieces
        assert fn(s, C.byref(args(ldo=18))) == -1
        assert fn(s, C.byref(args(CinP=40))) == -1
    up = L.lib().grl_upsample2x_bilinear_fwd
    assert up(s, C.c_void_p(x.data_ptr()), 34, C.c_void_p(out.data_ptr()), 16, 1, 1, 1, 16) == -1
    assert up(s, C.c_void_p(x.data_ptr()), 32, C.c_void_p(out.data_ptr()), 16, 1, 1, 1, 6) == -1
    assert L.lib().grl_upsample2x_bilinear_bwd(s, C.c_void_p(x.data_ptr() + 4), 32, C.c_void_p(out.data_ptr()), 16, 1, 1, 1, 16) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                   # nothing was launched
    with pytest.raises(RuntimeError, match="unsupported shape"):
        ops.conv4x4s2(torch.randn(5 * 8, 32, device="cuda"), w, 1, 5, 8, x_cols=32, n_store=16)
