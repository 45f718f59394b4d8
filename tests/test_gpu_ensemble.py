"""The x8 self-ensemble on the MI355X (csrc/ensemble.hip through ensemble.dihedral_pack / dihedral_merge / SelfEnsemble) -- needs
the GPU.  The two kernels are held to the CPU restatement bit for bit (``torch.equal``): the transforms only move values, and the
merge is seven IEEE adds in one fixed order and an exact scaling.  The wrapper over a small GRL is held to the same wrapper over the
same weights on the CPU composite path at the project's bar for one forward, 1e-3: the mean of eight outputs that are each within
the bar is within it."""
import ctypes as C

import pytest
import torch

from grl_image_restoration_amd import GRL, _lib, ensemble as E, make_config, tiling
from oracle import grl_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-3

# below, at and across the 32 x 32 tile edge, square and not, one and several workgroups
SHAPES = [(1, 1), (1, 7), (3, 5), (32, 32), (33, 65), (70, 37), (64, 64)]
ids = lambda s: "x".join(map(str, s))


def values(shape, seed, dtype=torch.float32):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2.0 - 0.5).to(dtype)


def channels_last_padded(v, pad, col0=0):
    """``v`` (B, C, H, W) as a view of a (B*H*W, col0 + C + pad) token matrix on the GPU, built as ``forward_infer._image`` builds the
    network's output; the other columns are NaN, so a read outside the view shows."""
    B, Cn, H, W = v.shape
    t = torch.full((B * H * W, col0 + Cn + pad), float("nan"), dtype=v.dtype, device=DEV)
    t[:, col0 : col0 + Cn] = v.permute(0, 2, 3, 1).reshape(-1, Cn).to(DEV)
    return t.view(B, H, W, -1)[..., col0 : col0 + Cn].permute(0, 3, 1, 2)


def crop_view(v, top, left, bottom=1, right=2):
    """``v`` as an offset crop of a larger NaN-filled NCHW tensor on the GPU."""
    B, Cn, H, W = v.shape
    big = torch.full((B, Cn + 1, H + top + bottom, W + left + right), float("nan"), dtype=v.dtype, device=DEV)
    big[:, 1:, top : top + H, left : left + W] = v.to(DEV)
    return big[:, 1:, top : top + H, left : left + W]


def eight_views(vs):
    """Member k as a strided view of its own kind: four channels-last ones of different pitch and first column, four crops of
    different offsets."""
    return [channels_last_padded(v, pad=1 + 2 * k, col0=k % 3) if k < 4 else crop_view(v, top=k - 4, left=7 - k, bottom=k % 2, right=2 * k - 7)
            for k, v in enumerate(vs)]


def same(got, want):
    """``torch.equal`` that also holds NaN to its place."""
    got = got.cpu()
    nan = torch.isnan(want)
    zero = torch.zeros((), dtype=want.dtype)
    return (got.shape == want.shape and got.dtype == want.dtype and torch.equal(torch.isnan(got), nan)
            and torch.equal(torch.where(nan, zero, got), torch.where(nan, zero, want)))


@pytest.mark.parametrize("hw", SHAPES, ids=ids)
def test_pack_equals_the_cpu_restatement(hw):
    H, W = hw
    for B in (1, 2):
        for Cn in (1, 3, 6):
            x = values((B, Cn, H, W), seed=B * 10 + Cn)
            wa, wb = E.dihedral_pack(x)
            sources = {"contiguous": x.to(DEV), "crop": crop_view(x, 2, 3), "channels_last": channels_last_padded(x, pad=8 - Cn)}
            assert sources["crop"].storage_offset() > 0 and sources["channels_last"].stride()[1::2] == (1, 8)
            for name, src in sources.items():
                a, b = E.dihedral_pack(src)
                assert a.is_cuda and a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype == torch.float32
                assert a.shape == wa.shape and b.shape == wb.shape
                assert torch.equal(a.cpu(), wa) and torch.equal(b.cpu(), wb), (name, B, Cn, H, W)
                if H == W:                                # one batch of eight
                    assert b.data_ptr() == a.data_ptr() + a.numel() * 4


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("hw", SHAPES, ids=ids)
def test_merge_equals_the_cpu_restatement(hw, dtype):
    Ho, Wo = hw
    for B in (1, 2):
        for Cn in (1, 3, 6):
            vs = [values((B, Cn, Wo, Ho) if k % 2 else (B, Cn, Ho, Wo), seed=100 * B + 10 * Cn + k, dtype=dtype) for k in range(8)]
            want = E.dihedral_merge(vs)
            assert want.dtype == torch.float32 and want.shape == (B, Cn, Ho, Wo)
            got = E.dihedral_merge([v.to(DEV) for v in vs])
            assert got.is_cuda and got.is_contiguous() and same(got, want), ("contiguous", B, Cn, Ho, Wo)
            views = eight_views(vs)
            assert Ho * Wo == 1 or len({(m.stride(), m.storage_offset()) for m in views}) == 8
            assert same(E.dihedral_merge(views), want), ("views", B, Cn, Ho, Wo)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_merge_propagates_nan_and_inf_to_their_pixels(dtype):
    B, Cn, Ho, Wo = 2, 3, 33, 65
    vs = [values((B, Cn, Wo, Ho) if k % 2 else (B, Cn, Ho, Wo), seed=50 + k, dtype=dtype) for k in range(8)]
    vs[5][1, 2, 40, 7] = float("nan")                     # m5[i][j] = f5[Wo-1-j][Ho-1-i]: the output's (25, 24)
    vs[2][0, 0, 3, 64] = float("inf")                     # m2[i][j] = f2[Ho-1-i][Wo-1-j]: the output's (29, 0)
    want = E.dihedral_merge(vs)
    assert torch.isnan(want[1, 2, 25, 24]) and want[0, 0, 29, 0] == float("inf") and int((~torch.isfinite(want)).sum()) == 2
    for members in ([v.to(DEV) for v in vs], eight_views(vs)):
        got = E.dihedral_merge(members)
        assert same(got, want)
        assert torch.isnan(got[1, 2, 25, 24]) and got[0, 0, 29, 0] == float("inf") and int((~torch.isfinite(got)).sum()) == 2


def test_merge_of_packed_transforms_is_the_image_and_repeats_to_the_bit():
    x = values((2, 3, 37, 70), seed=7).to(DEV)
    a, b = E.dihedral_pack(x)
    members = [None] * 8
    for n, k in enumerate(E.GROUP_A):
        members[k] = a[2 * n : 2 * n + 2]
    for n, k in enumerate(E.GROUP_B):
        members[k] = b[2 * n : 2 * n + 2]
    first = E.dihedral_merge(members)
    assert torch.equal(first, x) and torch.equal(E.dihedral_merge(members), first)


def test_bad_arguments_are_refused_without_a_launch():
    x = values((2, 3, 5, 7), seed=1).to(DEV)
    with pytest.raises(TypeError):
        E.dihedral_pack(x.half())
    with pytest.raises(ValueError):
        E.dihedral_pack(x[0])
    with pytest.raises(TypeError):
        E.dihedral_merge([x.double().transpose(-2, -1) if k % 2 else x.double() for k in range(8)])
    L = _lib.lib()
    a, b = torch.zeros(8, 3, 5, 7, device=DEV), torch.zeros(8, 3, 7, 5, device=DEV)
    good = dict(x=x.data_ptr(), stride=(C.c_int64 * 4)(*x.stride()), B=2, C=3, H=5, W=7, out_a=a.data_ptr(), out_b=b.data_ptr())
    pack = lambda **kw: L.grl_dihedral_pack(_lib.stream_ptr(), C.byref(_lib.GrlDihedralPackArgs(**dict(good, **kw))))
    for kw in (dict(x=None), dict(out_a=None), dict(out_b=None), dict(B=0), dict(C=-1), dict(H=0), dict(W=-2)):
        assert pack(**kw) == -1, kw
    for kw in (dict(x=x.data_ptr() + 2), dict(out_a=a.data_ptr() + 1), dict(out_b=b.data_ptr() + 2),
               dict(B=1, C=1, H=1 << 15, W=1 << 14),                                   # 4 * 2^29 elements: exactly 2^31
               dict(B=(1 << 31) - 1, C=(1 << 31) - 1, H=(1 << 31) - 1, W=(1 << 31) - 1),  # nothing overflows on the way to the refusal
               dict(B=1 << 16, C=1, H=1, W=1), dict(B=1, C=1, H=32 * 65535 + 1, W=1)):
        assert pack(**kw) == -2, kw
    assert L.grl_dihedral_pack(_lib.stream_ptr(), None) == -1
    out = torch.zeros(2, 3, 5, 7, device=DEV)
    m = _lib.GrlDihedralMergeArgs(dtype=_lib.DT_F32, B=2, C=3, Ho=5, Wo=7, out=out.data_ptr())
    merge = lambda: L.grl_dihedral_merge(_lib.stream_ptr(), C.byref(m))
    assert merge() == -1                                                                # null members
    for k in range(8):
        m.member[k] = x.data_ptr()
    m.dtype = _lib.DT_BF16
    assert merge() == -1
    m.dtype = _lib.DT_F32
    m.member[6] = x.data_ptr() + 2
    assert merge() == -2
    m.dtype = _lib.DT_F16
    m.member[6] = x.data_ptr() + 1
    assert merge() == -2
    assert L.grl_dihedral_merge(_lib.stream_ptr(), None) == -1
    torch.cuda.synchronize()
    assert int(a.abs().sum()) == 0 and int(b.abs().sum()) == 0 and int(out.abs().sum()) == 0    # nothing was launched


# ---- the wrapper over a small GRL ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grl():
    """The depths [1, 1] x4 GRL of tests/test_gpu_train_replicas.py with its seeded weights, on the GPU and on the CPU, the two
    inputs, and the CPU composite's ensembles of them (computed once, shared, never written to)."""
    cfg = make_config("base", "sr_ckpt_df2", upscale=4, img_size=64, depths=[1, 1], num_heads_window=[3, 3], num_heads_stripe=[3, 3],
                      drop_path_rate=0.0)
    cpu, gpu = GRL(**cfg).eval(), GRL(**cfg).eval()
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in cpu.state_dict().items()}, 0)
    cpu.load_state_dict(sd, strict=True)
    gpu.load_state_dict(sd, strict=True)
    gpu = gpu.to(DEV)
    xs = {"48x80": O.synthetic_pair("sr", (48, 80), 4, seed=3)[0], "64x64": O.synthetic_pair("sr", (64, 64), 4, seed=4)[0]}
    calls = []

    def counted(x):
        calls.append(tuple(x.shape))
        return cpu(x)

    want = {k: E.SelfEnsemble(counted)(x) for k, x in xs.items()}
    assert calls == [(4, 3, 48, 80), (4, 3, 80, 48), (8, 3, 64, 64)]
    return cpu, gpu, xs, want


@pytest.mark.parametrize("name", ["48x80", "64x64"])
def test_self_ensemble_over_grl_agrees_with_the_cpu_composite(grl, name):
    cpu, gpu, xs, want = grl
    x = xs[name].to(DEV)
    se = E.SelfEnsemble(gpu)
    got = se(x)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want[name].shape == (1, 3, 4 * x.shape[2], 4 * x.shape[3])
    err = (got.cpu() - want[name]).abs().max().item()
    with torch.no_grad():
        plain = gpu(x).float()
    moved = (got - plain).abs().max().item()
    print(f"SelfEnsemble(GRL depths [1, 1] x4) {name}: max|hip - cpu composite| = {err:.3e} (bar {BAR:g}); "
          f"max|ensemble - plain forward| = {moved:.3e}")
    assert err <= BAR, err
    assert moved > BAR, moved                             # the model is not equivariant: a wrapper that does nothing fails here
    assert se.out_channels == 3 and torch.equal(se(x), got)


def test_tiled_self_ensemble_over_grl(grl):
    cpu, gpu, xs, _ = grl
    x = xs["48x80"]
    got = tiling.forward_tiled(E.SelfEnsemble(gpu), x.to(DEV), 32, 8, 4, out_channels=3)
    assert got.shape == (1, 3, 192, 320) and bool(torch.isfinite(got).all())
    want = tiling.forward_tiled(E.SelfEnsemble(cpu), x, 32, 8, 4, out_channels=3)
    err = (got.cpu() - want).abs().max().item()
    print(f"forward_tiled(SelfEnsemble(GRL), 48x80, tile 32, overlap 8): max|hip - cpu composite| = {err:.3e} (bar {BAR:g})")
    assert err <= BAR, err
