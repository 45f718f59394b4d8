"""grl_spectral_norm_fwd / grl_spectral_norm_bwd (csrc/spectral_norm.hip) through ops, autograd and the discriminator, against the
float64 evaluation of the same expressions on the CPU.

Bars are measured, not chosen (the convention of jitter.py and isp.py): per quantity -- out, u', v', sigma, dW -- four times the
largest deviation of torch's own fp32 CPU evaluation from float64 over the shapes below, every deviation relative to the largest
magnitude of that quantity.  ``yardstick`` computes them once per session and the tests print them next to the kernels' figures.
"""
import copy
import ctypes as C
import math

import pytest
import torch

import tests.test_gpu_disc as DISC
from grl_image_restoration_amd import _lib, ops
from grl_image_restoration_amd import autograd as AG
from grl_image_restoration_amd.discriminator import spectral_norm_grad
from tests.test_gpu_gan import TOL as LOGIT_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (3, 7), (5, 65), (65, 5), (130, 1025), (64, 576), (256, 4608), (512, 4096)]
QUANTITIES = ("out", "u", "v", "sigma")


def forward_ref(W, u, v, advance):
    """The header's expressions in the arguments' dtype: (out, u', v', sigma)."""
    if advance:
        t = torch.mv(W.t(), u)
        v = t / t.norm().clamp_min(1e-12)
        s = torch.mv(W, v)
        u = s / s.norm().clamp_min(1e-12)
    else:
        s = torch.mv(W, v)
    sigma = torch.dot(u, s)
    return W / sigma, u, v, sigma


def rel(got, want, scale=None):
    """max|got - want| over the largest magnitude of the quantity (``scale``: that magnitude where ``want`` does not show it)."""
    want = want.double()
    return float((got.double().cpu() - want).abs().max() / (want.abs().max() if scale is None else scale))


def dw_scale(c):
    """dW = G / sigma - (a rank-one projection of it): the magnitude of the quantity is max|G / sigma|.  (max|dW| itself will not
    do for every shape: the 1 x 1 layer's dW is exactly zero.)"""
    return float(c["G"].double().abs().max() / c["train"][3].abs())


def make_layer(cout, k):
    """Kaiming-uniform weights as the constructor draws them, u / v warmed by five float64 power iterations, a random G."""
    g = torch.Generator().manual_seed(cout * 7919 + k)
    W = torch.empty(cout, k)
    bound = 1.0 / math.sqrt(k)                         # kaiming_uniform_(a = sqrt(5)): gain sqrt(1/3), bound = gain sqrt(3 / fan_in)
    W.uniform_(-bound, bound, generator=g)
    u = torch.nn.functional.normalize(torch.randn(cout, generator=g, dtype=torch.float64), dim=0)
    v = torch.nn.functional.normalize(torch.randn(k, generator=g, dtype=torch.float64), dim=0)
    for _ in range(5):
        _, u, v, _ = forward_ref(W.double(), u, v, True)
    G = torch.randn(cout, k, generator=g)
    return dict(W=W, u=u.float(), v=v.float(), G=G)


@pytest.fixture(scope="module")
def layers():
    return build_layers()


def build_layers():
    """Per shape the inputs, the float64 results of a training and an eval forward and of the backward, and the fp32 CPU deviations."""
    out = []
    for cout, k in SHAPES:
        c = make_layer(cout, k)
        W64, u64, v64, G64 = c["W"].double(), c["u"].double(), c["v"].double(), c["G"].double()
        c["train"] = forward_ref(W64, u64, v64, True)
        c["eval"] = forward_ref(W64, u64, v64, False)
        c["dW"] = spectral_norm_grad(G64, W64, c["train"][1], c["train"][2], c["train"][3])
        f32 = forward_ref(c["W"], c["u"], c["v"], True)
        c["dev"] = {q: rel(a, b) for q, a, b in zip(QUANTITIES, f32, c["train"])}
        # torch's fp32 autograd through the same chain, u' and v' constants
        Wr = c["W"].clone().requires_grad_(True)
        dw32, = torch.autograd.grad(Wr / torch.dot(f32[1], torch.mv(Wr, f32[2])), Wr, c["G"])
        c["dev"]["dW"] = rel(dw32, c["dW"], dw_scale(c))
        out.append(c)
    return out


@pytest.fixture(scope="module")
def yardstick(layers):
    bars = {q: 4.0 * max(c["dev"][q] for c in layers) for q in QUANTITIES + ("dW",)}
    print("fp32 CPU deviation from float64, largest over the shapes:", {q: f"{b / 4:.2e}" for q, b in bars.items()})
    assert all(0 < b < 1e-5 for b in bars.values()), bars          # (an fp32 evaluation: a few units of 2^-24 times sqrt(terms))
    return bars


def run_forward(cs, advance, keep=True):
    ws, us, vs = [c["W"].to(DEV) for c in cs], [c["u"].to(DEV) for c in cs], [c["v"].to(DEV) for c in cs]
    outs, kept = ops.spectral_norm(ws, us, vs, advance, keep=keep)
    return ws, us, vs, outs, kept


def check_forward(cs, got, mode, bars, what):
    ws, us, vs, outs, kept = got
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for l, c in enumerate(cs):
        want = c[mode]
        figures = dict(out=rel(outs[l], want[0]), u=rel(us[l], want[1]), v=rel(vs[l], want[2]), sigma=rel(kept[2][l], want[3]))
        assert torch.equal(kept[0][l], us[l]) and torch.equal(kept[1][l], vs[l])         # the forward's own copies
        for q, e in figures.items():
            worst[q] = max(worst[q], e)
    print(f"{what}: " + "  ".join(f"{q} gpu {worst[q]:.2e} / fp32 cpu {bars[q] / 4:.2e} / bar {bars[q]:.2e}" for q in QUANTITIES))
    for q in QUANTITIES:
        assert worst[q] <= bars[q], (what, q, worst[q], bars[q])


CASES = [[i] for i in range(len(SHAPES))] + [list(range(len(SHAPES)))]
IDS = ["{}x{}".format(*s) for s in SHAPES] + ["all"]


@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_training_forward(layers, yardstick, idx):
    cs = [layers[i] for i in idx]
    got = run_forward(cs, True)
    for l, c in enumerate(cs):                        # u and v were advanced in place
        assert not torch.equal(got[1][l].cpu(), c["u"]) or c["W"].numel() == 1
    check_forward(cs, got, "train", yardstick, f"train {[SHAPES[i] for i in idx]}")


@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_eval_forward_leaves_u_and_v_alone(layers, yardstick, idx):
    cs = [layers[i] for i in idx]
    got = run_forward(cs, False)
    for l, c in enumerate(cs):
        assert torch.equal(got[1][l].cpu(), c["u"]) and torch.equal(got[2][l].cpu(), c["v"])
    check_forward(cs, got, "eval", yardstick, f"eval {[SHAPES[i] for i in idx]}")


@pytest.mark.parametrize("idx", CASES, ids=IDS)
def test_backward(layers, yardstick, idx):
    cs = [layers[i] for i in idx]
    ws, us, vs, outs, kept = run_forward(cs, True)
    dws = ops.spectral_norm_bwd([c["G"].to(DEV) for c in cs], ws, kept)
    worst = 0.0
    for c, dw, u, v, s in zip(cs, dws, kept[0], kept[1], kept[2]):
        # against the closed form at the vectors the GPU forward produced (their own deviation is test_training_forward's business)
        want = spectral_norm_grad(c["G"].double(), c["W"].double(), u.double().cpu(), v.double().cpu(), s.double().cpu())
        worst = max(worst, rel(dw, want, dw_scale(c)), rel(dw, c["dW"], dw_scale(c)))
    print(f"backward {[SHAPES[i] for i in idx]}: dW gpu {worst:.2e} / fp32 cpu {yardstick['dW'] / 4:.2e} / bar {yardstick['dW']:.2e}")
    assert worst <= yardstick["dW"], (worst, yardstick["dW"])


def test_backward_of_the_first_of_two_forwards(layers, yardstick):
    """GanStep's discriminator step: real forward, fake forward, one backward.  The first forward's backward runs after the second
    has advanced the buffers; it must use the first forward's u', v', sigma.  One layer is frozen."""
    cs = [layers[4], layers[5], layers[1]]
    ws = [c["W"].to(DEV).requires_grad_(l != 1) for l, c in enumerate(cs)]
    us, vs = [c["u"].to(DEV) for c in cs], [c["v"].to(DEV) for c in cs]
    first = AG.spectral_norm(ws, us, vs, True)
    AG.spectral_norm(ws, us, vs, True)
    gs = [c["G"].to(DEV) for c in cs]
    torch.autograd.backward([first[0], first[2]], [gs[0], gs[2]])
    assert ws[1].grad is None
    for l in (0, 2):
        c = cs[l]
        W64 = c["W"].double()
        _, u2, v2, s2 = forward_ref(W64, c["train"][1], c["train"][2], True)       # what the second forward left in the buffers
        wrong = spectral_norm_grad(c["G"].double(), W64, u2, v2, s2)
        err, err_wrong = rel(ws[l].grad, c["dW"], dw_scale(c)), rel(ws[l].grad, wrong, dw_scale(c))
        print(f"{tuple(c['W'].shape)}: dW against the first forward's vectors {err:.2e}, against the second's {err_wrong:.2e}, "
              f"bar {yardstick['dW']:.2e}")
        assert err <= yardstick["dW"] and err_wrong > yardstick["dW"]
        assert rel(us[l], u2) <= yardstick["u"] and rel(vs[l], v2) <= yardstick["v"]       # the buffers did advance twice


def test_nothing_is_kept_when_no_weight_needs_a_gradient(layers):
    cs = [layers[2], layers[3]]
    ws = [c["W"].to(DEV) for c in cs]
    ops.profile_begin()
    try:
        outs = AG.spectral_norm(ws, [c["u"].to(DEV) for c in cs], [c["v"].to(DEV) for c in cs], True)
    finally:
        rec = ops.profile_end()
    assert all(not o.requires_grad for o in outs) and set(rec) == {"spectral_norm"} and len(rec["spectral_norm"]) == 1


def _everything(cs):
    ws, us, vs, outs, kept = run_forward(cs, True)
    dws = ops.spectral_norm_bwd([c["G"].to(DEV) for c in cs], ws, kept)
    ev = run_forward(cs, False)
    torch.cuda.synchronize()
    return [*us, *vs, *outs, *kept[0], *kept[1], kept[2], *dws, *ev[3], ev[4][2]]


def test_two_calls_give_the_same_bits(layers):
    a, b = _everything(layers), _everything(layers)
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_poisoned_workspaces_guard_bands_and_dirty_lds(layers):
    clean = _everything(layers)
    prev_guards = ops._GUARDS
    prev_poison = ops.set_poison(True, guards=True)
    prev_lds = _lib.set_dirty_lds(True)
    try:
        dirty = _everything(layers)
    finally:
        _lib.set_dirty_lds(prev_lds)
        ops.set_poison(prev_poison, guards=prev_guards)
        ops.check_guards()
    assert all(bool(torch.isfinite(x).all()) for x in dirty)
    assert all(torch.equal(x, y) for x, y in zip(clean, dirty))


def test_bad_arguments_are_refused_before_any_launch(layers):
    c = layers[1]
    W, u, v = c["W"].to(DEV), c["u"].to(DEV), c["v"].to(DEV)
    out = torch.full_like(W, 7.0)
    ws = torch.zeros(1024, device=DEV)
    sigma = torch.full((1,), 7.0, device=DEV)

    def args(n=1, **kw):
        a = _lib.GrlSpectralNormArgs(n_layers=n, advance=1, ws=ws.data_ptr(), ws_bytes=4096)
        for l in range(min(n, _lib.SN_MAX_LAYERS)):
            a.w[l], a.u[l], a.v[l], a.out[l], a.sigma[l], a.g[l] = (t.data_ptr() for t in (W, u, v, out, sigma, W))
            a.cout[l], a.k[l] = W.shape
        for name, (l, val) in kw.items():
            getattr(a, name)[l] = val
        return a

    s = _lib.stream_ptr()
    for fn in (_lib.lib().grl_spectral_norm_fwd, _lib.lib().grl_spectral_norm_bwd):
        assert fn(s, C.byref(args(17))) == -1
        assert fn(s, C.byref(args(0))) == -1
        assert fn(s, C.byref(args(w=(0, None)))) == -1
        assert fn(s, C.byref(args(2, out=(1, None)))) == -1
        assert fn(s, C.byref(args(cout=(0, 0)))) == -1
        assert fn(s, C.byref(args(2, k=(1, -3)))) == -1
        small = args()
        small.ws_bytes = 4
        assert fn(s, C.byref(small)) == -1
        assert fn(s, None) == -1
    assert _lib.lib().grl_spectral_norm_bwd(s, C.byref(args(sigma=(0, None)))) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and float(sigma) == 7.0 and torch.equal(u.cpu(), c["u"])        # nothing was launched
    with pytest.raises(RuntimeError, match="grl_spectral_norm_fwd failed: bad argument"):
        ops.spectral_norm([W] * 17, [u.clone() for _ in range(17)], [v.clone() for _ in range(17)], True)


def test_the_discriminator_runs_on_the_kernels(yardstick):
    """UNetDiscriminatorSN(3, 8) with the reference fixture's weights: one training forward and backward on the GPU against the same
    module on the CPU in float64.  Bars: u / v as above; logits tests/test_gpu_gan.py's; weight_orig gradients tests/test_gpu_disc.py's
    (4 x the fp16 operand emulation's own error, LeakyReLU under the GPU run's masks)."""
    nets = {8: DISC._fixture_state()[0]}
    cpu, gpu = DISC._pair(nets, 8)
    emu, own = copy.deepcopy(cpu), copy.deepcopy(cpu)
    x = torch.from_numpy(DISC._fixture_state()[1]["d__A__x"])
    ptrs = [(getattr(gpu, c).weight_u.data_ptr(), getattr(gpu, c).weight_v.data_ptr()) for c in DISC.SN]
    ops.profile_begin()
    try:
        acts = []
        logits = gpu._forward_traced(x.to(DEV), acts=acts)
        logits.mean().backward()
    finally:
        rec = ops.profile_end()
    assert len(rec["spectral_norm"]) == 1 and len(rec["spectral_norm_bwd"]) == 1          # one call each for the eight layers
    masks = [(t > 0).cpu() for t in acts]
    ref = cpu._forward_traced(x.double(), masks=masks)
    ref.mean().backward()
    emu._forward_traced(x.double(), torch.float16, masks=masks).mean().backward()
    assert ptrs == [(getattr(gpu, c).weight_u.data_ptr(), getattr(gpu, c).weight_v.data_ptr()) for c in DISC.SN]
    for c in DISC.SN:
        for b in ("u", "v"):
            e = rel(getattr(getattr(gpu, c), "weight_" + b), getattr(getattr(cpu, c), "weight_" + b))
            assert e <= yardstick[b], (c, b, e)
    with torch.no_grad():                              # (the logits: every run under its own masks, as in tests/test_gpu_disc.py)
        err = float((logits.double().cpu() - own(x.double())).abs().max())
    print(f"logits: max|gpu - fp64| {err:.2e}  (bar {LOGIT_TOL:.0e})")
    assert err <= LOGIT_TOL
    pe, pg = dict(emu.named_parameters()), dict(gpu.named_parameters())
    for k, p in cpu.named_parameters():
        if k.endswith("weight_orig"):
            DISC.check(f"grad {k}", pg[k].grad, p.grad, pe[k].grad)
