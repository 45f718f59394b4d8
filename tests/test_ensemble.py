"""The x8 self-ensemble on the CPU (ensemble.py, evaluate / restore ``self_ensemble``).  The transforms are pinned against
tests/golden/tasks/dihedral.npz, which tools/make_golden_ensemble.py wrote with the reference's own ``Augment_RGB_torch``
(utils/dataset_utils.py:6-39); everything else is ``torch.equal`` against the formula written out here: the restated transforms and
the one fixed summation order."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import grl_image_restoration_amd as G
from grl_image_restoration_amd import _lib, ensemble as E, evaluate as EV, restore, tiling
from tests.test_tasks import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVERSE = (0, 3, 2, 1, 4, 5, 6, 7)                       # the issue's table, restated: T1 and T3 undo each other, the rest themselves


def fixed_order_mean(m):
    return (((m[0] + m[1]) + (m[2] + m[3])) + ((m[4] + m[5]) + (m[6] + m[7]))) * 0.125


def explicit_ensemble(f, x):
    """out = 1/8 sum_k T_k^-1(f(T_k(x))), every member a forward of its own."""
    return fixed_order_mean([E.transform(f(E.transform(x, k).contiguous()), INVERSE[k]) for k in range(8)])


class Stub:
    """A fixed asymmetric 3 x 3 convolution and a x2 nearest upsample: not equivariant under any flip or rotation.  The convolution
    is called image by image: the CPU's conv2d picks its blocking by the batch size, and an image's bits with it, while the
    ensemble and the formula it is held to batch the members differently."""

    def __init__(self, cin=3, cout=None, scale=2):
        cout = cin if cout is None else cout
        self.out_channels, self.scale, self.calls = cout, scale, []
        w = torch.arange(cout * cin * 9, dtype=torch.float32).reshape(cout, cin, 3, 3)
        self.weight = (w * 0.37).sin() * 0.25 + torch.tensor([[0.5, -0.25, 0.125], [0.0, 1.0, -0.5], [0.25, 0.75, -1.0]]) / cin

    def __call__(self, x):
        self.calls.append(tuple(x.shape))
        y = torch.cat([F.conv2d(x[n : n + 1], self.weight, padding=1) for n in range(x.shape[0])], dim=0)
        return F.interpolate(y, scale_factor=self.scale, mode="nearest") if self.scale > 1 else y


def image(*shape, seed=0):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("k", range(8))
def test_transform_equals_the_reference_fixture(k):
    meta, z = golden("dihedral")
    assert meta["shape"] == [2, 3, 3, 5] and torch.equal(z["x"], torch.arange(90).reshape(2, 3, 3, 5))
    got = E.transform(z["x"], k)
    assert got.shape == z[f"t{k}"].shape == ((2, 3, 5, 3) if k % 2 else (2, 3, 3, 5))
    assert torch.equal(got, z[f"t{k}"])
    # and as the index map of the table
    x, H, W = z["x"], 3, 5
    src = {0: lambda i, j: (i, j), 1: lambda i, j: (H - 1 - j, i), 2: lambda i, j: (H - 1 - i, W - 1 - j), 3: lambda i, j: (j, W - 1 - i),
           4: lambda i, j: (H - 1 - i, j), 5: lambda i, j: (H - 1 - j, W - 1 - i), 6: lambda i, j: (i, W - 1 - j), 7: lambda i, j: (j, i)}[k]
    for i in range(got.shape[-2]):
        for j in range(got.shape[-1]):
            assert torch.equal(got[..., i, j], x[(..., *src(i, j))]), (k, i, j)


def test_inverse_column_and_groups():
    x = image(2, 3, 5, 7)
    assert E.INVERSE == INVERSE and E.GROUP_A == (0, 2, 4, 6) and E.GROUP_B == (1, 3, 5, 7)
    for k in range(8):
        assert torch.equal(E.transform(E.transform(x, k), INVERSE[k]), x), k
    with pytest.raises(ValueError):
        E.transform(x, 8)


@pytest.mark.parametrize("shape", [(1, 3, 6, 6), (2, 1, 5, 7), (3, 6, 4, 6)], ids=lambda s: "x".join(map(str, s)))
def test_pack_layout_and_merge_round_trip(shape):
    x = image(*shape, seed=1)
    B, C, H, W = shape
    a, b = E.dihedral_pack(x)
    assert a.shape == (4 * B, C, H, W) and b.shape == (4 * B, C, W, H) and a.is_contiguous() and b.is_contiguous()
    for n, k in enumerate((0, 2, 4, 6)):
        assert torch.equal(a[n * B : (n + 1) * B], E.transform(x, k)), k
    for n, k in enumerate((1, 3, 5, 7)):
        assert torch.equal(b[n * B : (n + 1) * B], E.transform(x, k)), k
    if H == W:                                            # the two halves of one batch of eight
        assert b.data_ptr() == a.data_ptr() + a.numel() * a.element_size()
    # members as they would come back from an identity model: the mean of eight copies of x is x, exactly
    members = [E.transform(x, k) for k in range(8)]
    assert torch.equal(E.dihedral_merge(members), x)
    assert torch.equal(E.dihedral_merge([m.contiguous() for m in members]), x)
    # the fixed order, on members that differ
    members = [E.transform(image(*shape, seed=10 + k), k).contiguous() for k in range(8)]
    want = fixed_order_mean([image(*shape, seed=10 + k) for k in range(8)])
    assert torch.equal(E.dihedral_merge(members), want)
    with pytest.raises(ValueError):
        E.dihedral_merge(members[:7])
    if H != W:
        with pytest.raises(ValueError):
            E.dihedral_merge(members[:1] * 8)


def test_merge_of_16_bit_members_sums_in_fp32_and_specials_propagate():
    ms = [E.transform(image(1, 3, 4, 6, seed=20 + k), k).half() for k in range(8)]
    got = E.dihedral_merge(ms)
    assert got.dtype == torch.float32
    assert torch.equal(got, fixed_order_mean([E.transform(m.float(), INVERSE[k]) for k, m in enumerate(ms)]))
    ms = [E.transform(image(1, 1, 3, 5, seed=30 + k), k).contiguous() for k in range(8)]
    ms[3][0, 0, 4, 1] = float("nan")                      # T3's (4, 1) is the output's (1, W-1-4) = (1, 0)
    ms[6][0, 0, 2, 0] = float("inf")                      # T6's (2, 0) is the output's (2, 4)
    got = E.dihedral_merge(ms)
    assert torch.isnan(got[0, 0, 1, 0]) and got[0, 0, 2, 4] == float("inf") and int(torch.isfinite(got).sum()) == 13


@pytest.mark.parametrize("shape,cout,max_batch,calls", [
    ((1, 3, 6, 6), 3, 8, [(8, 3, 6, 6)]),                                           # square, B = 1: ONE forward of batch 8
    ((2, 1, 5, 7), 1, 8, [(8, 1, 5, 7), (8, 1, 7, 5)]),                             # two groups
    ((3, 3, 4, 4), 3, 2, [(2, 3, 4, 4)] * 12),                 # batch 3: eight members of 2 images, then 4 x 2 members of 1
    ((1, 6, 4, 6), 3, 8, [(4, 6, 4, 6), (4, 6, 6, 4)]),                             # 6 in, 3 out
    ((2, 3, 5, 5), 3, 5, [(4, 3, 5, 5)] * 4),                                       # two members of two images per forward
], ids=["1x3x6x6", "2x1x5x7", "3x3x4x4_max2", "1x6x4x6_out3", "2x3x5x5_max5"])
def test_self_ensemble_equals_the_explicit_formula(shape, cout, max_batch, calls):
    x = image(*shape, seed=2)
    stub, ref = Stub(shape[1], cout), Stub(shape[1], cout)
    se = E.SelfEnsemble(stub, max_batch=max_batch)
    got = se(x)
    assert stub.calls == calls
    assert got.shape == (shape[0], cout, 2 * shape[2], 2 * shape[3]) and got.dtype == torch.float32
    assert torch.equal(got, explicit_ensemble(ref, x))
    assert not torch.equal(got, ref(x))                   # the stub is not equivariant: the ensemble is not the plain forward
    assert se.out_channels == cout and G.SelfEnsemble is E.SelfEnsemble


def test_self_ensemble_over_a_pointwise_model_is_the_model():
    x = image(2, 3, 5, 7, seed=3)
    f = lambda t: t * t * 3.0 - 0.25
    assert torch.equal(E.SelfEnsemble(f)(x), f(x))
    assert torch.equal(E.SelfEnsemble(f, max_batch=1)(x), f(x))


def test_self_ensemble_forwards_eval_to_and_out_channels():
    m = torch.nn.Conv2d(3, 5, 1)
    se = E.SelfEnsemble(m.train())
    assert se.eval() is se and not m.training
    assert se.to(torch.float64) is se and m.weight.dtype == torch.float64
    assert se.out_channels == 5 and E.SelfEnsemble(lambda t: t).out_channels is None
    assert se(image(1, 3, 4, 4).double()).shape == (1, 5, 4, 4) and not se(image(1, 3, 4, 4).double()).requires_grad
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            E.SelfEnsemble(m, max_batch=bad)
    assert "not swapped" in E.SelfEnsemble.__doc__ and "tile origins" in E.SelfEnsemble.__doc__


def test_forward_tiled_gives_every_tile_its_own_ensemble():
    x = image(1, 3, 7, 9, seed=4)
    stub, ref = Stub(3), Stub(3)
    got = tiling.forward_tiled(E.SelfEnsemble(stub), x, tile=4, overlap=1, scale=2)
    per_tile = lambda patch: explicit_ensemble(ref, patch)                          # the transforms act on every tile of the chunk alone
    want = tiling.forward_tiled(per_tile, x, tile=4, overlap=1, scale=2)
    assert got.shape == (1, 3, 14, 18) and torch.equal(got, want)
    assert all(s == (6, 3, 4, 4) for s in stub.calls) and len(stub.calls) == 8       # 6 tiles: eight batches of six transformed tiles
    # ... which is not the ensemble of whole tiled passes: the tile origins are not symmetric under a flip
    whole = E.SelfEnsemble(lambda t: tiling.forward_tiled(ref, t, tile=4, overlap=1, scale=2))(x)
    assert whole.shape == got.shape and not torch.equal(whole, got)


def test_evaluate_pairs_with_and_without_the_option():
    stub = Stub(3, scale=1)
    pairs = [(image(1, 3, 9, 12, seed=5), image(1, 3, 9, 12, seed=6)), (image(1, 3, 8, 8, seed=7), image(1, 3, 8, 8, seed=8))]
    plain = EV.evaluate_pairs(stub, pairs, 1, device="cpu")
    assert EV.evaluate_pairs(stub, pairs, 1, device="cpu", self_ensemble=False) == plain
    plus = EV.evaluate_pairs(stub, pairs, 1, device="cpu", self_ensemble=True)
    assert len(plus) == 2 and all(a != b for a, b in zip(plus, plain))
    want = [float(EV.psnr_y(explicit_ensemble(Stub(3, scale=1), lq), gt, 1)) for lq, gt in pairs]
    assert plus == want
    tiled = EV.evaluate_pairs(stub, pairs[:1], 1, tile=6, overlap=2, device="cpu", self_ensemble=True)
    want = tiling.forward_tiled(E.SelfEnsemble(Stub(3, scale=1)), pairs[0][0], 6, 2, 1, out_channels=3)
    assert tiled == [float(EV.psnr_y(want, pairs[0][1], 1))] and tiled != plus[:1]


def test_both_parsers_take_the_option():
    a = EV._parser().parse_args(["--model", "tiny", "--geometry", "yaml", "--gt", "x", "--self-ensemble"])
    assert a.self_ensemble is True
    assert EV._parser().parse_args(["--model", "tiny", "--geometry", "yaml", "--gt", "x"]).self_ensemble is False
    a = restore._parser().parse_args(["--lq", "a", "--out", "b", "--geometry", "yaml", "--self-ensemble"])
    assert a.self_ensemble is True
    assert restore._parser().parse_args(["--lq", "a", "--out", "b", "--geometry", "yaml"]).self_ensemble is False


def test_restore_folder_with_the_option(tmp_path):
    from PIL import Image

    from grl_image_restoration_amd import image8 as I

    im = (image(7, 9, 3, seed=9) * 255).to(torch.uint8)
    d = tmp_path / "lq"
    d.mkdir()
    Image.fromarray(im.numpy()).save(d / "a.png")
    stub = Stub(3, scale=1)
    lq = im.permute(2, 0, 1)[None].float().div(255)
    plain = restore.restore_folder(stub, str(d), str(tmp_path / "plain"), device="cpu", workers=1)
    plus = restore.restore_folder(stub, str(d), str(tmp_path / "plus"), device="cpu", workers=1, self_ensemble=True)
    read = lambda p: torch.from_numpy(np.asarray(Image.open(p)).copy())
    assert torch.equal(read(plain[0]), I.pack8(stub(lq))[0])
    assert torch.equal(read(plus[0]), I.pack8(explicit_ensemble(stub, lq))[0]) and not torch.equal(read(plus[0]), read(plain[0]))


def test_entries_are_bound_and_the_header_states_them():
    assert "grl_dihedral_pack" in _lib.EXPORTS and "grl_dihedral_merge" in _lib.EXPORTS and _lib.ABI_VERSION >= 41
    header = open(os.path.join(ROOT, "include", "grl_hip.h")).read()
    assert int(re.search(r"#define GRL_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    assert "utils/dataset_utils.py:6-39" in header and "x[H-1-j][W-1-i]" in header
    assert "((m0 + m1) + (m2 + m3)) + ((m4 + m5) + (m6 + m7))" in header


def test_the_launch_wrappers_refuse_cpu_tensors():
    """No fallback below ``ensemble``: the wrappers of the two entries take CUDA tensors only."""
    from grl_image_restoration_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dihedral_pack(image(1, 3, 4, 4), torch.empty(4, 3, 4, 4), torch.empty(4, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dihedral_merge([image(1, 3, 4, 4)] * 8, torch.empty(1, 3, 4, 4))
