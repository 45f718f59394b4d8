"""Which kernels one inference forward launches, per route of the block plan -- needs the MI355X.

A plan field that is packed but never consumed (or consumed under another name) fails no numeric test: the forward takes the
generic kernels and is merely slower.  So every case below runs one ``no_grad`` forward between ``ops.profile_begin()`` and
``ops.profile_end()`` and compares {kernel name: launches} with a literal dict.

The dicts were recorded on the commit BEFORE the plan became typed and model.py was split (string-keyed plan dicts, all of the
launch sequence in ``GRL``), with exactly the shapes and weights below; they are not regenerated from the code under test.
All weights are seeded (oracle.grl_oracle.seeded_state_dict, as tests/test_gpu_model.py::_product).

The profiler names a launch by its C-ABI entry and shape, not by the variant inside it: cases (a) and (b) record the same counts
(``qkv_anchor`` with and without the split-operand blob; ``block_tail`` with and without the register image).  So each case also
asserts the plan fields that select its route.  Every case reached its route at the shape the issue names; none was adjusted.
"""
import math

import pytest
import torch

from oracle import grl_oracle as O
from tests.util import load_golden

pytestmark = pytest.mark.gpu

_CUT = dict(depths=[2, 1], num_heads_window=[3, 3], num_heads_stripe=[3, 3])
_CUT_SMALL = dict(depths=[2, 1], num_heads_window=[2, 2], num_heads_stripe=[2, 2])


def _case(name):
    """(constructor kwargs, weight seed, input shape, clamp: every logit scale set to ln 100, environment)."""
    from grl_image_restoration_amd import make_config

    base = make_config("base", "sr_ckpt_df2", upscale=4, img_size=64, **_CUT)
    if name == "a_base_fast":          # one-pass qkv_anchor, fused tail on the register image, cab_conv2, two stream groups
        return dict(base, precision="fast"), 0, (2, 3, 64, 64), False, {}
    if name == "b_base_fast_clamp":    # hiq blocks: the split-operand q / k / anchor pass (qa_lo)
        return dict(base, precision="fast"), 0, (2, 3, 64, 64), True, {"GRL_CALIBRATE": "0"}
    if name == "c_base_high":          # block_high: fused-LN epilogues, pooled anchor route
        return dict(base, precision="high"), 0, (1, 3, 64, 64), False, {}
    if name == "d_small_dn_fast":      # 128x64 stripes of every other block: transposed tables
        return (dict(make_config("small", "dn_df4", upscale=1, img_size=128, **_CUT_SMALL), precision="fast"), 0, (1, 3, 128, 128),
                False, {})
    if name == "e_tiny_auto":          # GRL-Tiny: `auto` resolves to `high`, CP = 64
        return dict(load_golden("tiny_sr2_ckpt_64")[0]["cfg"], precision="auto"), 0, (1, 3, 64, 64), False, {}
    raise KeyError(name)


def run_case(name, setenv):
    """One forward of case ``name`` -> ({kernel: launches}, output on the CPU, the model).  ``setenv(key, value)`` sets an environment
    variable for the duration of the caller's scope (monkeypatch.setenv in the test)."""
    from grl_image_restoration_amd import GRL, ops

    cfg, seed, shape, clamp, env = _case(name)
    for k, v in env.items():
        setenv(k, v)
    m = GRL(**cfg).eval()
    m.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed), strict=True)
    if clamp:
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("logit_scale"):
                    p.fill_(math.log(100.0))
    m = m.to("cuda:0")
    x = torch.rand(shape, generator=torch.Generator().manual_seed(1)).to("cuda:0")
    with torch.no_grad():
        ops.profile_begin()
        try:
            y = m(x)
        finally:
            rec = ops.profile_end()
    return {k: len(v) for k, v in sorted(rec.items())}, y.float().cpu(), m


# recorded on the parent commit (see the module docstring)
LAUNCHES = {
    "a_base_fast": {'attention q32x32 k32x32': 6,
                    'attention q32x32 k64x64': 6,
                    'attention q64x64 k32x32': 6,
                    'block_tail': 6,
                    'cab_conv2': 6,
                    'conv3x3 192->192 64x64': 5,
                    'conv3x3 192->48 64x64': 6,
                    'conv3x3 192->64 64x64': 1,
                    'conv3x3 64->16 256x256': 1,
                    'conv3x3 64->256 128x128': 2,
                    'conv3x3 64->256 64x64': 2,
                    'conv3x3 96->192 64x64': 1,
                    'qkv_anchor': 6},
    "b_base_fast_clamp": {'attention q32x32 k32x32': 6,
                          'attention q32x32 k64x64': 6,
                          'attention q64x64 k32x32': 6,
                          'block_tail': 6,
                          'cab_conv2': 6,
                          'conv3x3 192->192 64x64': 5,
                          'conv3x3 192->48 64x64': 6,
                          'conv3x3 192->64 64x64': 1,
                          'conv3x3 64->16 256x256': 1,
                          'conv3x3 64->256 128x128': 2,
                          'conv3x3 64->256 64x64': 2,
                          'conv3x3 96->192 64x64': 1,
                          'qkv_anchor': 6},
    "c_base_high": {'attention q32x32 k32x32': 3,
                    'attention q32x32 k64x64': 3,
                    'attention q64x64 k32x32': 3,
                    'conv3x3 192->16 256x256': 1,
                    'conv3x3 192->192 64x64': 3,
                    'conv3x3 192->256 128x128': 2,
                    'conv3x3 192->256 64x64': 2,
                    'conv3x3 576->192 64x64': 3,
                    'conv3x3 576->64 64x64': 4,
                    'conv3x3 96->192 64x64': 1,
                    'linear 1152->192': 3,
                    'linear 576->192': 3,
                    'linear 576->384': 3,
                    'linear 576->576': 3,
                    'linear 576->96': 3},
    "d_small_dn_fast": {'attention q16x16 k16x16': 3,
                        'attention q16x32 k64x128': 3,
                        'attention q64x128 k16x32': 3,
                        'conv3x3 384->128 128x128': 3,
                        'conv3x3 384->16 128x128': 1,
                        'conv3x3 96->128 128x128': 1,
                        'linear 128->128': 3,
                        'linear 128->64': 3,
                        'mlp': 3,
                        'qkv': 3},
    "e_tiny_auto": {'attention q16x16 k64x64': 16,
                    'attention q32x32 k32x32': 16,
                    'attention q64x64 k16x16': 16,
                    'conv3x3 192->16 64x64': 1,
                    'conv3x3 192->64 64x64': 5,
                    'conv3x3 96->64 64x64': 1,
                    'linear 192->128': 16,
                    'linear 192->384': 16,
                    'linear 192->64': 16,
                    'linear 384->64': 32},
}
PRECISION = {"a_base_fast": "fast", "b_base_fast_clamp": "fast", "c_base_high": "high", "d_small_dn_fast": "fast", "e_tiny_auto": "high"}


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_forward_launches_the_recorded_kernels(name, monkeypatch):
    got, y, m = run_case(name, monkeypatch.setenv)
    print(name, m.precision, got)
    assert bool(torch.isfinite(y).all())
    assert m.precision == PRECISION[name]
    assert got == LAUNCHES[name]
    blocks = [pk for st in next(iter(m._plan_cache.values())).stages for pk in st.blocks]
    if name == "a_base_fast":
        assert m.stream_groups(2) == 2 and all(pk.qa_blob is not None and pk.tail_rblob is not None and pk.cab2_blob is not None
                                               for pk in blocks)
    if name == "b_base_fast_clamp":
        assert all(pk.hiq and pk.qa_lo is not None for pk in blocks)
    if name == "c_base_high":
        assert all(pk.hi and pk.anc_wr is not None and pk.proj_wr is not None for pk in blocks)
    if name == "d_small_dn_fast":
        assert any(pk.tr_a2w for pk in blocks) and not all(pk.tr_a2w for pk in blocks)
    if name == "e_tiny_auto":
        assert m.embed_dim == 64 and all(pk.hi and pk.qkv_blob is None for pk in blocks)
