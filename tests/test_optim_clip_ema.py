"""CPU tests of FusedAdamW's gradient clipping and weight average: the composite arithmetic (``_step_cpu``) against
``clip_grad_norm_`` + ``torch.optim.AdamW``, the reported norm and coefficient, the state round trips, the refusals, the binding,
and the accessors on a small CPU GRL."""
import copy
import math

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, FusedAdamW, _lib, make_config

SHAPES = [(96, 40), (300,), (1,), (8, 20, 3, 3), (5000,)]
KW = dict(lr=2e-4, weight_decay=1e-4)                       # config/optimizer/adamw.yaml


def _params(seed=45, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * (10.0 ** -step) for s in shapes] for step in range(4)]
    return p0, grads


def _fresh(p0):
    return [t.clone().requires_grad_(True) for t in p0]


def _set(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g.clone()


def _norm64(gs):
    return torch.cat([g.reshape(-1) for g in gs]).double().norm().item()


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def test_clipped_steps_match_clip_grad_norm_and_torch_adamw():
    p0, grads = _params()
    pa, pb = _fresh(p0), _fresh(p0)
    oa, ob = FusedAdamW(pa, max_grad_norm=1.0, **KW), torch.optim.AdamW(pb, **KW)
    for step in range(4):
        _set(pa, grads[step]); _set(pb, grads[step])
        oa.step()
        torch.nn.utils.clip_grad_norm_(pb, 1.0)
        ob.step()
        if step == 0:
            assert oa.last_clip_coef() < 1.0               # the clip bites
    for a, b in zip(pa, pb):                                # the bars of tests/test_gpu_train.py::test_fused_adamw_matches_torch
        assert (a - b).abs().max().item() <= 2e-6 * max(1.0, b.abs().max().item())
    sa, sb = oa.state[pa[0]], ob.state[pb[0]]
    assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=1e-4, atol=1e-8)
    assert torch.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=1e-4, atol=1e-10)


def test_a_clip_that_does_not_bite_changes_no_bit_and_the_norm_is_the_float64_one():
    p0, grads = _params()
    pa, pb = _fresh(p0), _fresh(p0)
    want = _norm64(grads[0])
    oa, ob = FusedAdamW(pa, max_grad_norm=2.0 * want, **KW), FusedAdamW(pb, **KW)
    _set(pa, grads[0]); _set(pb, grads[0])
    oa.step(); ob.step()
    assert oa.last_clip_coef() == 1.0
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert abs(oa.last_grad_norm() - want) <= _ulp32(want)
    # grad_scale goes into the norm: it is that of the scaled gradient
    _set(pa, grads[1])
    oa.step(grad_scale=0.25)
    want = 0.25 * _norm64(grads[1])
    assert abs(oa.last_grad_norm() - want) <= _ulp32(want)
    with pytest.raises(RuntimeError):
        ob.last_grad_norm()


def test_non_finite_gradients_follow_torch_clamp():
    p0, grads = _params()
    for bad, check in ((float("inf"), lambda c: c == 0.0), (float("nan"), math.isnan)):
        pa = _fresh(p0)
        oa = FusedAdamW(pa, max_grad_norm=1.0, **KW)
        _set(pa, grads[0])
        pa[3].grad.view(-1)[7] = bad
        oa.step()
        assert check(oa.last_clip_coef()), (bad, oa.last_clip_coef())


def test_ema_after_one_step_is_torch_lerp():
    p0, grads = _params()
    d = 0.9
    pa = _fresh(p0)
    oa = FusedAdamW(pa, ema_decay=d, **KW)
    _set(pa, grads[0])
    oa.step()
    for before, p in zip(p0, pa):
        assert torch.equal(oa.state[p]["ema"], torch.lerp(before, p.detach(), 1.0 - d))
    # a parameter that takes no step keeps its average
    kept = oa.state[pa[1]]["ema"].clone()
    _set(pa, grads[1])
    pa[1].grad = None
    oa.step()
    assert torch.equal(oa.state[pa[1]]["ema"], kept) and not torch.equal(oa.state[pa[0]]["ema"], torch.lerp(p0[0], pa[0].detach(), 1.0 - d))


def test_state_round_trips():
    p0, grads = _params()
    pa = _fresh(p0)
    oa = FusedAdamW(pa, max_grad_norm=1.0, ema_decay=0.9, **KW)
    for step in range(2):
        _set(pa, grads[step]); oa.step()
    # into a fresh FusedAdamW: two more steps stay in lock-step, averages included
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    ob = FusedAdamW(pb, max_grad_norm=1.0, ema_decay=0.9, **KW)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    assert all(torch.equal(oa.state[a]["ema"], ob.state[b]["ema"]) for a, b in zip(pa, pb))
    # into torch.optim.AdamW (extra state keys are carried along) and back
    pc = [p.detach().clone().requires_grad_(True) for p in pa]
    ot = torch.optim.AdamW(pc, **KW)
    ot.load_state_dict(copy.deepcopy(oa.state_dict()))
    assert all(torch.equal(ot.state[c]["ema"], oa.state[a]["ema"]) for a, c in zip(pa, pc))
    od = FusedAdamW(pc, **KW)                               # (the groups of the loaded state say max_grad_norm / ema_decay)
    od.load_state_dict(copy.deepcopy(ot.state_dict()))
    assert od.param_groups[0]["max_grad_norm"] == 1.0 and od.param_groups[0]["ema_decay"] == 0.9
    for step in range(2, 4):
        for ps, o in ((pa, oa), (pb, ob), (pc, od)):
            _set(ps, grads[step]); o.step()
    for a, b, c in zip(pa, pb, pc):
        assert torch.equal(a, b) and torch.equal(a, c)
        assert torch.equal(oa.state[a]["ema"], ob.state[b]["ema"]) and torch.equal(oa.state[a]["ema"], od.state[c]["ema"])
    # a state WITHOUT averages (torch.optim.AdamW's own) into an optimizer with ema_decay: the average starts from the current weights
    pe = [p.detach().clone().requires_grad_(True) for p in pa]
    plain = torch.optim.AdamW([p.detach().clone().requires_grad_(True) for p in pa], **KW)
    _set(plain.param_groups[0]["params"], grads[0]); plain.step()
    oe = FusedAdamW(pe, ema_decay=0.5, **KW)
    oe.load_state_dict(copy.deepcopy(plain.state_dict()))
    assert oe.param_groups[0]["ema_decay"] == 0.5 and "ema" not in oe.state[pe[0]]
    start = [p.detach().clone() for p in pe]
    _set(pe, grads[1]); oe.step()
    assert all(torch.equal(oe.state[p]["ema"], torch.lerp(s, p.detach(), 0.5)) for s, p in zip(start, pe))


def test_refusals():
    p0, grads = _params()
    pa = _fresh(p0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdamW([dict(params=pa[:2], max_grad_norm=1.0), dict(params=pa[2:], max_grad_norm=2.0)], **KW)
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdamW([dict(params=pa[:2], max_grad_norm=1.0), dict(params=pa[2:])], **KW)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="max_grad_norm"):
            FusedAdamW(pa, max_grad_norm=bad, **KW)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdamW(pa, ema_decay=bad, **KW)
    FusedAdamW(pa, ema_decay=0.0, **KW)
    # a group changed after construction is caught at the step
    o = FusedAdamW([dict(params=pa[:2]), dict(params=pa[2:])], max_grad_norm=1.0, **KW)
    o.param_groups[1]["max_grad_norm"] = 3.0
    _set(pa, grads[0])
    with pytest.raises(ValueError, match="max_grad_norm"):
        o.step()
    # capture mode holds both by value: a change raises instead of being ignored
    for key, new in (("max_grad_norm", 2.0), ("ema_decay", 0.5)):
        pb = _fresh(p0)
        o = FusedAdamW(pb, max_grad_norm=1.0, ema_decay=0.9, **KW)
        _set(pb, grads[0]); o.step()
        o.enable_capture()
        o.refresh_capture_hyper()
        o.param_groups[0][key] = new
        with pytest.raises(RuntimeError, match=key):
            o.refresh_capture_hyper()


def test_capture_mode_load_keeps_the_average_buffers():
    p0, grads = _params()
    pa, pb = _fresh(p0), _fresh(p0)
    oa, ob = FusedAdamW(pa, ema_decay=0.9, **KW), FusedAdamW(pb, ema_decay=0.9, **KW)
    for step in range(2):
        _set(pb, grads[step]); ob.step()
    _set(pa, grads[2]); oa.step()
    oa.enable_capture()
    ptrs = [oa.state[p]["ema"].data_ptr() for p in pa]
    oa.load_state_dict(copy.deepcopy(ob.state_dict()))
    assert [oa.state[p]["ema"].data_ptr() for p in pa] == ptrs
    assert all(torch.equal(oa.state[a]["ema"], ob.state[b]["ema"]) for a, b in zip(pa, pb))


def test_binding_has_the_entry_points():
    assert "grl_grad_sqnorm" in _lib.EXPORTS and "grl_grad_clip_finish" in _lib.EXPORTS and _lib.ABI_VERSION >= 44
    assert {"grad_clip_dev", "ema", "ema_decay"} <= {f[0] for f in _lib.GrlAdamWArgs._fields_}


def test_ema_state_dict_and_ema_applied_on_a_small_model():
    torch.manual_seed(0)
    model = GRL(**make_config("tiny", "yaml", upscale=2, img_size=16, depths=[1], num_heads_window=[2], num_heads_stripe=[2])).train()
    opt = FusedAdamW(model.parameters(), lr=1e-2, ema_decay=0.5)
    x = torch.rand(1, 3, 16, 16)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model(x).abs().mean().backward()
    opt.step()
    trained = {k: v.detach().clone() for k, v in model.state_dict().items()}
    avg = opt.ema_state_dict(model)
    assert avg.keys() == trained.keys()
    names = {k for k, _ in model.named_parameters()}
    stepped = {k for k, p in model.named_parameters() if p in opt.state}
    assert stepped and any(not torch.equal(avg[k], trained[k]) for k in stepped)
    for k in trained:
        if k in stepped:
            assert torch.equal(avg[k], opt.state[dict(model.named_parameters())[k]]["ema"])
        elif k not in names:
            assert torch.equal(avg[k], trained[k])          # buffers are as they are
    versions = {k: p._version for k, p in model.named_parameters() if k in stepped}
    with opt.ema_applied(model):
        for k, p in model.named_parameters():
            if k in stepped:
                assert torch.equal(p.detach(), avg[k]) and p._version > versions[k]
        inside = {k: p._version for k, p in model.named_parameters() if k in stepped}
    for k, p in model.named_parameters():
        assert torch.equal(p.detach(), trained[k])
        if k in stepped:
            assert p._version > inside[k]
