"""The closed-form backward of the spectral normalisation that grl_spectral_norm_bwd evaluates (include/grl_hip.h;
``discriminator.spectral_norm_grad`` states it in torch),
    dW = G / sigma - (<G, W> / sigma^2) u v^T        (u, v the vectors sigma was formed with, held constant),
against float64 autograd through ``discriminator._SNConv.weight()``, the restatement of torch.nn.utils.spectral_norm, in train and
eval mode.  The two are the same function of the same float64 numbers: 1e-12 relative to max|dW| (measured: 1e-16).
"""
import pytest
import torch

from grl_image_restoration_amd.discriminator import _SNConv, spectral_norm_grad

SHAPES = [(4, 36), (8, 64), (65, 5)]


def warmed(cout, k, seed):
    """A layer whose u / v have seen five power iterations (a fresh random pair gives sigma near zero)."""
    torch.manual_seed(seed)
    m = _SNConv(k, cout, 1).double().train()
    with torch.no_grad():
        for _ in range(5):
            m.weight()
    return m


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_closed_form_backward_is_autograd_of_the_torch_chain(shape, training):
    cout, k = shape
    m = warmed(cout, k, cout * 100 + k).train(training)
    u0, v0 = m.weight_u.clone(), m.weight_v.clone()
    out = m.weight()
    assert out.dtype == torch.float64
    G = torch.randn(out.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(k))
    want, = torch.autograd.grad(out, m.weight_orig, G)
    # the vectors of THIS forward: advanced in place in training mode, untouched in eval mode
    u, v = m.weight_u.clone(), m.weight_v.clone()
    assert (not torch.equal(u, u0)) == training and (not torch.equal(v, v0)) == training
    W = m.weight_orig.detach().reshape(cout, k)
    sigma = torch.dot(u, W @ v)
    got = spectral_norm_grad(G.reshape(cout, k), W, u, v, sigma).reshape(want.shape)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"{shape} training={training}: max|closed form - autograd| / max|dW| = {err:.2e}")
    assert err <= 1e-12
