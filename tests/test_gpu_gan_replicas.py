"""gan.GanStep(process_group=...) on the GPU: two replicas in SPAWNED processes on the one GPU of the box, gloo between them (the
pattern of tests/test_gpu_train_replicas.py; RCCL refuses two ranks on one device).  Each replica takes half of a batch of four.

The replicas hold the same weights after the constructor's broadcast and the same averaged gradients after every all-reduce, so
they must stay BIT-identical, weight_u / weight_v included, although nothing broadcasts those again: that is the spectral-norm
kernels' fixed summation order (csrc/spectral_norm.hip) seen across processes.  Against the single-process full-batch step the
yardstick is tests/test_gpu_train_replicas.py's: what two single-process runs differ by (fp32 atomics in the weight-gradient
reductions), times 4, plus 2e-6 on the mean absolute weight difference and 1e-4 on the losses.
"""
import pytest
import torch

import tests.test_gan_replicas_gloo as CPU

pytestmark = pytest.mark.gpu


def _single():
    g, d, step = CPU.make("cuda", torch.float32)
    rows = CPU.run_steps(step, CPU.batch("cuda", torch.float32), 2)
    return rows, CPU.state(g, d)


# (last in the file: the test runs replicas in spawned processes on the same GPU -- three processes at most)
def test_two_replicas_stay_bit_identical_and_follow_the_single_process_step():
    r0, r1 = CPU.spawn_replicas("cuda", torch.float32)
    assert r0["collectives"] == r1["collectives"] == 4
    for k, v in r0["constructed"].items():
        assert torch.equal(v, r1["constructed"][k]), k
    for key in ("final", "final_bf16"):
        for k, v in r0[key].items():
            assert torch.equal(v, r1[key][k]), (key, k)               # every weight, and weight_u / weight_v
    assert any("weight_u" in k and not torch.equal(v, r0["constructed"][k]) for k, v in r0["final"].items())
    (la, pa), (lb, pb) = _single(), _single()                          # two single-process runs: the yardstick
    keys = [k for k in pa if pa[k].is_floating_point()]
    n = sum(pa[k].numel() for k in keys)
    d_ee = sum(float((pa[k] - pb[k]).abs().sum()) for k in keys) / n
    d_eg = sum(float((pa[k] - r0["final"][k]).abs().sum()) for k in keys) / n
    lg = [{s: 0.5 * (a[s] + b[s]) for s in CPU.SCALARS} for a, b in zip(r0["rows"], r1["rows"])]      # means are linear in the batch
    l_ee = max(abs(a[s] - b[s]) for a, b in zip(la, lb) for s in CPU.SCALARS)
    l_eg = max(abs(a[s] - b[s]) for a, b in zip(la, lg) for s in CPU.SCALARS)
    print(f"mean |dw| single-single {d_ee:.3e}, single-replicas {d_eg:.3e}; max |dloss| {l_ee:.3e} / {l_eg:.3e}")
    assert d_eg <= 4.0 * d_ee + 2e-6 and l_eg <= 4.0 * l_ee + 1e-4
    assert all(x == x and abs(x) < float("inf") for r in (r0, r1) for x in r["rows_bf16"][0].values())
