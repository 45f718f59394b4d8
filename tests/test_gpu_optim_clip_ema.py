"""GPU tests of FusedAdamW's gradient clipping and weight average (csrc/grad.hip: grl_grad_sqnorm, grl_grad_clip_finish, the
(clip, ema) instances of the AdamW kernel) -- needs the MI355X.  The tensor sizes hit the edges of the 4096-element chunks, and
one tensor alone has 301 chunks: the finishing workgroup (256 lanes) loops more than once per lane."""
import copy
import math
import socket

import numpy as np
import pytest
import torch

from oracle import grl_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (3, 1, 1), (4095,), (4096,), (4097,), (5000,), (64, 180, 3, 3), (300 * 4096 + 1,)]
KW = dict(lr=2e-4, weight_decay=1e-4)                       # config/optimizer/adamw.yaml
DECAY = 0.9


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.fixture(scope="module")
def data():
    return build_data()


def build_data():
    """Start weights and four steps' gradients (shrinking by 10 ** -step, as tests/test_gpu_train.py's AdamW test does), on the host;
    the float64 norm of the first step's gradients.  Computed once, never modified."""
    g = torch.Generator().manual_seed(47)
    p0 = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [[torch.randn(s, generator=g) * (10.0 ** -step) for s in SHAPES] for step in range(4)]
    norm0 = torch.cat([t.reshape(-1) for t in grads[0]]).double().norm().item()
    return p0, grads, norm0


def _fresh(p0, dev="cuda"):
    return [t.clone().to(dev).requires_grad_(True) for t in p0]


def _set(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g.clone().to(p.device)


def test_norm_is_the_float64_norm_reproducible_and_scaled_exactly(data):
    from grl_image_restoration_amd import FusedAdamW

    p0, grads, norm0 = data
    pa = _fresh(p0)
    oa = FusedAdamW(pa, max_grad_norm=1.0, **KW)
    _set(pa, grads[0])
    oa.step()
    first = (oa.last_clip_coef(), oa.last_grad_norm())
    partials = oa._clip["partials"].clone()
    print(f"norm {first[1]!r} (float64 {norm0!r}), coefficient {first[0]!r}")
    assert abs(first[1] - norm0) <= _ulp32(norm0)
    want_coef = min(1.0, 1.0 / (first[1] + 1e-6))           # the float64 restatement, from the reported norm
    assert abs(first[0] - want_coef) <= _ulp32(want_coef) and first[0] < 1.0
    _set(pa, grads[0])                                       # the same gradients again: the same bits
    oa.step()
    assert (oa.last_clip_coef(), oa.last_grad_norm()) == first and torch.equal(oa._clip["partials"], partials)
    _set(pa, grads[0])
    oa.step(grad_scale=0.25)
    assert oa.last_grad_norm() == 0.25 * first[1]


def test_clipped_step_is_the_step_with_the_coefficient_as_grad_scale(data):
    from grl_image_restoration_amd import FusedAdamW

    p0, grads, norm0 = data
    pa, pb = _fresh(p0), _fresh(p0)
    oa, ob = FusedAdamW(pa, max_grad_norm=1.0, **KW), FusedAdamW(pb, **KW)
    _set(pa, grads[0]); _set(pb, grads[0])
    oa.step()
    ob.step(grad_scale=oa.last_clip_coef())
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])
    assert pa[0]._version > 0


def test_a_clip_that_does_not_bite_changes_no_bit(data):
    from grl_image_restoration_amd import FusedAdamW

    p0, grads, norm0 = data
    pa, pb = _fresh(p0), _fresh(p0)
    oa, ob = FusedAdamW(pa, max_grad_norm=2.0 * norm0, **KW), FusedAdamW(pb, **KW)
    _set(pa, grads[0]); _set(pb, grads[0])
    oa.step(); ob.step()
    assert oa.last_clip_coef() == 1.0
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) and torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])


def test_non_finite_norms_follow_torch_clamp(data):
    from grl_image_restoration_amd import FusedAdamW

    p0, grads, norm0 = data
    for bad, check in ((float("inf"), lambda c: c == 0.0), (float("nan"), math.isnan)):
        pa = _fresh(p0[:6])
        oa = FusedAdamW(pa, max_grad_norm=1.0, **KW)
        _set(pa, grads[0][:6])
        pa[4].grad.view(-1)[4096] = bad                     # the one element of a tensor's last chunk
        oa.step()
        assert check(oa.last_clip_coef()), (bad, oa.last_clip_coef())


def _torch_steps(p0, grads, dtype, dev):
    """clip_grad_norm_ + torch.optim.AdamW + _foreach_lerp_ over the four steps: the comparator (fp32) and, in float64, the
    restatement it is measured against."""
    ps = [t.clone().to(dev, dtype).requires_grad_(True) for t in p0]
    ema = [p.detach().clone() for p in ps]
    opt = torch.optim.AdamW(ps, **KW)
    for step in range(4):
        for p, g in zip(ps, grads[step]):
            p.grad = g.clone().to(dev, dtype)
        torch.nn.utils.clip_grad_norm_(ps, 1.0, foreach=True)
        opt.step()
        torch._foreach_lerp_(ema, [p.detach() for p in ps], 1.0 - DECAY)
    return [p.detach() for p in ps], ema


@pytest.fixture(scope="module")
def four_steps(data):
    """The four clipped, averaged steps through the kernels, through ``_step_cpu``, through torch in fp32 (GPU and CPU) and in
    float64 (CPU), once."""
    from grl_image_restoration_amd import FusedAdamW

    p0, grads, _ = data
    out = {}
    for dev in ("cuda", "cpu"):
        ps = _fresh(p0, dev)
        opt = FusedAdamW(ps, max_grad_norm=1.0, ema_decay=DECAY, **KW)
        coefs = []
        for step in range(4):
            _set(ps, grads[step])
            opt.step()
            coefs.append(opt.last_clip_coef())
        out["fused_" + dev] = ([p.detach().cpu() for p in ps], [opt.state[p]["ema"].cpu() for p in ps], coefs)
    out["torch_cuda"] = tuple([t.cpu() for t in part] for part in _torch_steps(p0, grads, torch.float32, "cuda"))
    out["torch_cpu"] = _torch_steps(p0, grads, torch.float32, "cpu")
    out["f64"] = _torch_steps(p0, grads, torch.float64, "cpu")
    return out


def test_four_steps_match_clip_grad_norm_torch_adamw_and_foreach_lerp(four_steps):
    w, e, coefs = four_steps["fused_cuda"]
    wt, et = four_steps["torch_cuda"]
    assert coefs[0] < 1.0                                   # the clip bites
    for a, b in zip(w, wt):                                 # the bar of tests/test_gpu_train.py::test_fused_adamw_matches_torch
        assert (a - b).abs().max().item() <= 2e-6 * max(1.0, b.abs().max().item())
    # the average is a convex combination of the start weights and the four new ones: it inherits their bar
    for a, b, ref in zip(e, et, wt):
        assert (a - b).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item())


def test_kernel_and_cpu_arithmetic_agree_as_closely_as_torch_follows_float64(four_steps):
    """The yardstick is measured here: how far torch's own fp32 CPU evaluation of the four steps lands from the float64 one.  The
    kernel and ``_step_cpu`` get four times that, against float64 and against each other."""
    def worst(xs, ys):
        return max((x.double() - y.double()).abs().max().item() for x, y in zip(xs, ys))

    for part, name in ((0, "weights"), (1, "averages")):
        yard = worst(four_steps["torch_cpu"][part], four_steps["f64"][part])
        gpu = worst(four_steps["fused_cuda"][part], four_steps["f64"][part])
        cpu = worst(four_steps["fused_cpu"][part], four_steps["f64"][part])
        both = worst(four_steps["fused_cuda"][part], four_steps["fused_cpu"][part])
        print(f"{name}: torch fp32 vs float64 {yard:.3e}; kernel vs float64 {gpu:.3e}; _step_cpu vs float64 {cpu:.3e}; kernel vs _step_cpu {both:.3e}")
        assert yard > 0 and gpu <= 4 * yard and cpu <= 4 * yard and both <= 4 * yard


def test_ema_after_one_step_is_the_stated_expression(data):
    from grl_image_restoration_amd import FusedAdamW

    p0, grads, _ = data
    pa = _fresh(p0)
    oa = FusedAdamW(pa, ema_decay=DECAY, **KW)
    _set(pa, grads[0])
    oa.step()
    k = float(np.float32(1.0) - np.float32(DECAY))          # 1 - ema_decay, formed in fp32
    for before, p in zip(p0, pa):
        w = p.detach().cpu()                                 # the fp32 weight the kernel wrote
        assert not torch.equal(w, before)
        want = before.double() + k * (w.double() - before.double())
        got = oa.state[p]["ema"].cpu()
        big = torch.maximum(got.abs(), w.abs())
        ulp = torch.nextafter(big, torch.full_like(big, float("inf"))) - big
        assert bool(((got.double() - want).abs() <= ulp.double()).all())
    # a parameter that takes no step keeps its average
    kept = oa.state[pa[2]]["ema"].clone()
    _set(pa, grads[1])
    pa[2].grad = None
    oa.step()
    assert torch.equal(oa.state[pa[2]]["ema"], kept)


def _small_model(cfg):
    from grl_image_restoration_amd import GRL

    torch.manual_seed(0)
    m = GRL(**cfg)
    m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 0), strict=True)
    return m.cuda().train()


def test_captured_step_clips_and_averages_on_every_replay():
    """Three replays against three eager steps from the same start, at the eager-versus-replay bar of
    tests/test_gpu_train_graph.py (two eager runs are the yardstick: the gradient GEMMs accumulate with atomics)."""
    from grl_image_restoration_amd import FusedAdamW, GraphedTrainStep, make_config

    cfg = make_config("base", "sr_ckpt_df2", upscale=4, img_size=64, depths=[1], num_heads_window=[3], num_heads_stripe=[3], drop_path_rate=0.0)
    lq, gt = O.synthetic_pair("sr", (64, 64), 4, batch=2, seed=12)
    lq2, gt2 = O.synthetic_pair("sr", (64, 64), 4, batch=2, seed=13)
    lq, gt, lq2, gt2 = lq.cuda(), gt.cuda(), lq2.cuda(), gt2.cuda()
    loss_fn = lambda y, t: (y - t).abs().mean()
    probe = _small_model(cfg)                              # the first eager step's norm, measured: the clip is half of it
    loss_fn(probe(lq), gt).backward()
    max_norm = 0.5 * torch.cat([p.grad.reshape(-1) for p in probe.parameters()]).double().norm().item()
    del probe
    models = [_small_model(cfg) for _ in range(3)]         # two eager runs and the graphed one
    opts = [FusedAdamW(m.parameters(), max_grad_norm=max_norm, ema_decay=DECAY, **KW) for m in models]

    def eager(i):
        for _ in range(1 + 3):
            opts[i].zero_grad(set_to_none=True)
            loss_fn(models[i](lq), gt).backward()
            opts[i].step()

    eager(0); eager(1)
    step = GraphedTrainStep(models[2], opts[2], loss_fn, lq, gt, warmup=1)
    coefs = []
    for _ in range(3):
        step(lq, gt)
        coefs.append(opts[2].last_clip_coef())
    step.finish()

    def dist(i, j, of):
        num = sum(float((of(i, p) - of(j, q)).abs().sum()) for p, q in zip(models[i].parameters(), models[j].parameters()))
        return num / sum(p.numel() for p in models[i].parameters())

    weight = lambda i, p: p.detach()
    ema = lambda i, p: opts[i].state[p]["ema"]
    d_ee, d_eg, e_ee, e_eg = dist(0, 1, weight), dist(0, 2, weight), dist(0, 1, ema), dist(0, 2, ema)
    print(f"mean |dp| eager-eager {d_ee:.3e}, eager-graph {d_eg:.3e}; averages {e_ee:.3e} / {e_eg:.3e}; replay coefficients {coefs}")
    assert d_eg <= 4 * d_ee + 1e-6 and e_eg <= 4 * e_ee + 1e-6
    assert all(0.0 < c < 1.0 for c in coefs)
    moved = sum(float((ema(2, p) - p.detach()).abs().sum()) for p in models[2].parameters())
    assert moved > 0                                        # the average lags the weights
    assert opts[2].state[next(iter(models[2].parameters()))]["step"] == 1 + 3
    # the coefficient is computed on replay, not frozen at capture: another batch, another norm
    step(lq, gt)
    n1 = opts[2].last_grad_norm()
    step(lq2, gt2)
    n2 = opts[2].last_grad_norm()
    assert math.isfinite(n1) and math.isfinite(n2) and n1 > 0 and n2 > 0 and n1 != n2
    # load_state_dict in capture mode: the loaded averages land in the buffers the graph points at
    ptrs = [opts[2].state[p]["ema"].data_ptr() for p in models[2].parameters()]
    opts[2].load_state_dict(copy.deepcopy(opts[0].state_dict()))
    assert [opts[2].state[p]["ema"].data_ptr() for p in models[2].parameters()] == ptrs
    assert all(torch.equal(opts[2].state[p]["ema"], opts[0].state[q]["ema"]) for p, q in zip(models[2].parameters(), models[0].parameters()))
    opts[2].param_groups[0]["max_grad_norm"] = 2.0 * max_norm
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        step(lq, gt)


# (last in the file: the test runs replicas in spawned processes on the same GPU)
def _replica(rank, world, port, ret, wire_bf16):
    """A replica of the two-graph data-parallel step on the one GPU of the box, gloo between the replicas
    (tests/test_gpu_train_replicas.py), with clipping and the weight average in graph B."""
    import os

    import torch.distributed as dist

    from grl_image_restoration_amd import GRL, FusedAdamW, GraphedTrainStep, make_config

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    cfg = make_config("base", "sr_ckpt_df2", upscale=4, img_size=64, depths=[1], num_heads_window=[3], num_heads_stripe=[3], drop_path_rate=0.0)
    torch.manual_seed(rank)
    m = GRL(**cfg)
    if rank == 0:
        m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 0), strict=True)
    m = m.to(dev).train()
    lq, gt = O.synthetic_pair("sr", (64, 64), 4, batch=2, seed=21)
    x, y = lq[rank : rank + 1].to(dev), gt[rank : rank + 1].to(dev)
    # (1e-3 is far below this model's gradient norm: the clip bites on every step)
    opt = FusedAdamW(m.parameters(), max_grad_norm=1e-3, ema_decay=DECAY, **KW)
    step = GraphedTrainStep(m, opt, lambda o, t: (o - t).abs().mean(), x, y, warmup=1, wire_bf16=wire_bf16)
    for _ in range(2):
        step(x, y)
    step.finish()
    torch.cuda.synchronize()
    ret[rank] = ({k: p.detach().cpu().clone() for k, p in m.named_parameters()},
                 {k: opt.state[p]["ema"].cpu().clone() for k, p in m.named_parameters()},
                 opt.last_grad_norm(), opt.last_clip_coef(),
                 torch.cat([g.reshape(-1) for g in step._raw_grads]).cpu(),       # this replica's own gradients of the last replay
                 step._flat.cpu().clone())                                         # and what the all-reduce made of both (the sum)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("wire_bf16", [False, True])
def test_data_parallel_replicas_clip_by_the_norm_of_the_averaged_gradient(wire_bf16):
    import torch.multiprocessing as mp

    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ret = mp.Manager().dict()
    mp.spawn(_replica, args=(2, port, ret, wire_bf16), nprocs=2, join=True)
    (p0, e0, n0, c0, g0, f0), (p1, e1, n1, c1, g1, f1) = ret[0], ret[1]
    assert n0 == n1 and c0 == c1 and 0.0 < c0 < 1.0
    for k in p0:
        assert torch.equal(p0[k], p1[k]) and torch.equal(e0[k], e1[k]), k
    assert torch.equal(f0, f1)
    # the averaged gradient the optimizer launch read: the all-reduced sum times 1 / world
    want = (f0.double() / 2).norm().item()
    print(f"wire_bf16={wire_bf16}: reported norm {n0!r}, float64 norm of the averaged buffer {want!r}")
    assert abs(n0 - want) <= _ulp32(want)
    if not wire_bf16:       # fp32 on the wire: that is the mean of the two replicas' own gradients
        want = ((g0.double() + g1.double()) / 2).norm().item()
        assert abs(n0 - want) <= _ulp32(want)
