"""Blended stitching of tiled inference on the CPU: the windows of ``tiling.blend_window``, the windowed restatement of
``tiling.stitch`` (the yardstick of the HIP kernel, tests/test_gpu_stitch.py), ``forward_tiled(blend=...)`` alone and over gloo, the
command lines, and the argument checks of grl_tile_stitch that need no device."""
import ctypes as C
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from grl_image_restoration_amd import _lib, evaluate, restore, tiling
from grl_image_restoration_amd.geometry import tile_origins


def _m(ts, R):
    return [min(i + 1, ts - i, R) for i in range(ts)]


@pytest.mark.parametrize("ts,R", [(12, 4), (16, 8), (6, 4), (5, 7), (64, 16), (7, 1), (9, 0)])
def test_blend_window_values(ts, R):
    """(6, 4) and (5, 7): ts < 2 R, the ramps meet before they reach the plateau."""
    assert torch.equal(tiling.blend_window("uniform", ts, R), torch.ones(ts))
    for kind in ("linear", "cosine"):
        w = tiling.blend_window(kind, ts, R)
        assert w.dtype == torch.float32 and w.shape == (ts,)
        assert bool((w > 0).all()) and bool((w <= 1).all()), kind
        assert torch.equal(w, w.flip(0)), kind
        if R <= 1:
            assert torch.equal(w, torch.ones(ts)), kind
    if R > 1:
        m = _m(ts, R)
        lin = tiling.blend_window("linear", ts, R)
        assert torch.equal(lin, torch.tensor(m, dtype=torch.float32) / torch.tensor(float(R), dtype=torch.float32))
        cos = tiling.blend_window("cosine", ts, R)
        want = torch.tensor([math.sin(math.pi * v / (2 * R)) ** 2 for v in m], dtype=torch.float64).to(torch.float32)
        assert torch.equal(cos, want)
        if ts >= 2 * R:
            assert bool((lin[R - 1 : ts - R + 1] == 1).all()) and bool((cos[R - 1 : ts - R + 1] == 1).all())
    with pytest.raises(ValueError):
        tiling.blend_window("gaussian", ts, R)


def _tiles(shape, tile, overlap, scale, oc, seed=0):
    b, c, h, w = shape
    tile, origins = tiling.tile_list(h, w, tile, overlap)
    g = torch.Generator().manual_seed(seed)
    return tile, origins, [torch.randn(b, oc, tile * scale, tile * scale, generator=g) for _ in origins]


def test_restatement_with_ones_is_the_uniform_stitch():
    shape, scale = (2, 3, 9, 11), 2
    tile, origins, outs = _tiles(shape, 4, 2, scale, 3)
    want = tiling.stitch(outs, origins, shape, tile, scale)
    got = tiling.stitch(outs, origins, shape, tile, scale, window=torch.ones(tile * scale))
    assert torch.equal(got, want)


def test_linear_blend_bounds_the_seam():
    """One row of tiles that disagree by d = 0.25: uniform averaging leaves steps of d / 2, the linear ramp of R = 4 at most
    d / (R + 1) = 0.05."""
    h, w, tile, overlap, scale = 6, 14, 6, 2, 2
    assert tile_origins(w, tile, overlap) == [0, 4, 8]
    tile, origins = tiling.tile_list(h, w, tile, overlap)
    ts, R, d = tile * scale, overlap * scale, 0.25
    outs = [torch.full((1, 1, ts, ts), 1 + d * k) for k in range(len(origins))]

    def jump(win):
        y = tiling.stitch(outs, origins, (1, 1, h, w), tile, scale, window=win)
        return float((y[..., 1:] - y[..., :-1]).abs().max())

    assert jump(None) == d / 2
    got = jump(tiling.blend_window("linear", ts, R))
    print(f"largest jump with the linear ramp: {got:.8f}")
    assert got <= d / (R + 1) * (1 + 1e-5)


class _Toy:
    """Batch-invariant x2 model: a 3 x 3 convolution and a pixel shuffle, image by image."""

    def __init__(self):
        self.w = torch.randn(3 * 4, 3, 3, 3, generator=torch.Generator().manual_seed(0)) * 0.2

    def __call__(self, x):
        F = torch.nn.functional
        return torch.cat([F.pixel_shuffle(F.conv2d(x[i : i + 1], self.w, padding=1), 2) for i in range(x.shape[0])], 0)


def _nearest(x, scale=2):
    return x.repeat_interleave(scale, -2).repeat_interleave(scale, -1)


@pytest.mark.parametrize("blend", ["linear", "cosine"])
def test_forward_tiled_with_a_blend_on_the_cpu(blend):
    shape, tile, overlap, scale = (2, 3, 33, 47), 16, 5, 2
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(5))
    model = _Toy()
    got = tiling.forward_tiled(model, x, tile, overlap, scale, tile_batch=3, blend=blend)
    _, origins = tiling.tile_list(33, 47, tile, overlap)
    outs = [model(x[..., a : a + tile, b : b + tile]) for a, b in origins]
    win = tiling.blend_window(blend, tile * scale, overlap * scale)
    assert torch.equal(got, tiling.stitch(outs, origins, shape, tile, scale, window=win))
    assert torch.equal(tiling.forward_tiled(model, x, tile, overlap, scale, window=win), got)
    assert not torch.equal(got, tiling.forward_tiled(model, x, tile, overlap, scale))
    # a pixel that one tile covers is that tile's output: exactly where its weight is 1 (the plateau), and as (o * w) / w -- two
    # roundings, |error| <= (2^-23 + 2^-48) |o| -- on the rim along the image border, where the weight is below 1 (the statement
    # of include/grl_hip.h has no special case for a single tile)
    cover = torch.zeros(33 * scale, 47 * scale)
    for a, b in origins:
        cover[a * scale : (a + tile) * scale, b * scale : (b + tile) * scale] += 1
    w2 = win[:, None] * win[None, :]
    plateau = rim = 0
    for (a, b), o in zip(origins, outs):
        sl = (slice(a * scale, (a + tile) * scale), slice(b * scale, (b + tile) * scale))
        single = cover[sl] == 1
        one = single & (w2 == 1)
        plateau += int(one.sum())
        rim += int((single & ~one).sum())
        g = got[(..., *sl)]
        assert torch.equal(g[..., one], o[..., one])
        err = (g[..., single].double() - o[..., single].double()).abs()
        assert bool((err <= (2.0 ** -23 + 2.0 ** -48) * o[..., single].double().abs()).all())
    assert plateau > 0 and rim > 0


@pytest.mark.parametrize("blend", ["uniform", "linear"])
def test_a_constant_image_stays_constant(blend):
    """Through an identity upsample, to one ulp (up to 3 x 3 tiles on a pixel here: 12 + 8 = 20 rows put the last origin at 12,
    next to 10)."""
    x = torch.full((1, 3, 20, 27), 0.3)
    y = tiling.forward_tiled(_nearest, x, 8, 3, 2, blend=blend)
    ulp = float(torch.tensor(0.3, dtype=torch.float32).nextafter(torch.tensor(1.0)) - torch.tensor(0.3, dtype=torch.float32))
    assert y.shape == (1, 3, 40, 54) and float((y - x[0, 0, 0, 0]).abs().max()) <= ulp


def test_windows_are_checked():
    x = torch.rand(1, 3, 12, 12)
    for bad in (torch.ones(7), torch.ones(16, dtype=torch.float64), torch.zeros(16), -torch.ones(16), torch.ones(4, 4),
                torch.full((16,), float("nan"))):
        with pytest.raises(ValueError):
            tiling.forward_tiled(_nearest, x, 8, 2, 2, window=bad)
    with pytest.raises(ValueError):
        tiling.forward_tiled(_nearest, x, 8, 2, 2, blend="median")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, shape, tile, overlap, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(5))
    ret[rank] = tiling.forward_tiled(_Toy(), x, tile, overlap, 2, tile_batch=2, blend="linear")
    dist.destroy_process_group()


def test_sharded_blend_is_bitwise_the_single_process_blend():
    shape, tile, overlap, world = (1, 3, 40, 56), 16, 4, 2
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(5))
    want = tiling.forward_tiled(_Toy(), x, tile, overlap, 2, tile_batch=3, blend="linear")
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), shape, tile, overlap, ret), nprocs=world, join=True)
    for r in range(world):
        assert torch.equal(ret[r], want), r


@pytest.mark.parametrize("main,argv", [
    (evaluate.main, ["--lq", "a", "--gt", "b", "--blend", "linear"]),
    (restore.main, ["--lq", "a", "--out", "b", "--geometry", "sr_ckpt_df2", "--blend", "cosine"]),
], ids=["evaluate", "restore"])
def test_blend_without_tile_is_refused(main, argv, capsys):
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2 and "--blend belongs to tiled inference" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main(argv[:-1] + ["gaussian", "--tile", "64"])


def test_folder_entries_refuse_a_blend_without_a_tile(tmp_path):
    with pytest.raises(ValueError, match="blend"):
        evaluate.evaluate_folder(None, str(tmp_path), str(tmp_path), 1, blend="linear")
    with pytest.raises(ValueError, match="blend"):
        restore.restore_folder(None, str(tmp_path), str(tmp_path / "out"), blend="cosine")


def test_abi():
    assert "grl_tile_stitch" in _lib.EXPORTS and _lib.ABI_VERSION >= 46


def _args(**over):
    """A valid call on a 9 x 11 image (tile 4, overlap 2, scale 2) with pointers that are never followed."""
    oy, ox = tile_origins(9, 4, 2), tile_origins(11, 4, 2)
    kw = dict(canvas=4096, tiles=8192, win=None, b=1, c=3, h=9, w=11, tile=4, scale=2, ny=len(oy), nx=len(ox), lo=0, hi=len(oy) * len(ox))
    kw.update({k: v for k, v in over.items() if k not in ("oy", "ox")})
    a = _lib.GrlTileStitchArgs(**kw)
    for dst, src in ((a.oy, over.get("oy", oy)), (a.ox, over.get("ox", ox))):
        for i, v in enumerate(src):
            dst[i] = v
    return a


@pytest.mark.parametrize("over", [
    dict(canvas=None), dict(tiles=None), dict(hi=21), dict(lo=5, hi=5), dict(lo=-1), dict(b=0), dict(c=0), dict(h=0), dict(w=-3),
    dict(tile=0), dict(scale=0), dict(ny=0), dict(nx=0), dict(tile=10), dict(ox=[0, 2, 4, 6, 8]), dict(oy=[0, 2, 4, 6]),
    dict(ox=[0, 2, 2, 6, 7]), dict(oy=[-1, 2, 4, 5]),
], ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()).replace(" ", ""))
def test_bad_arguments_are_refused_before_any_launch(over):
    """The checks run on the host before the first device call, so they need no GPU: a tile outside the canvas (origin 8 + tile 4 >
    11 columns, origin 6 + 4 > 9 rows), origins that do not ascend, an empty or overlong range, null pointers, non-positive sizes."""
    assert _lib.lib().grl_tile_stitch(C.c_void_p(0), C.byref(_args(**over))) == -1


def test_null_args_and_too_many_origins():
    assert _lib.lib().grl_tile_stitch(C.c_void_p(0), None) == -1
    assert _lib.lib().grl_tile_stitch(C.c_void_p(0), C.byref(_args(nx=_lib.STITCH_MAX_ORIGINS + 1))) == -2
