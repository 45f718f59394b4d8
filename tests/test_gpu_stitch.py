"""GPU tests of ``grl_tile_stitch`` (csrc/stitch.hip).  The yardstick is ``tiling.stitch`` on the CPU -- the reference's uniform
E / W loop, and its windowed restatement -- on the same tile values, and the bar is ``torch.equal``: the statement of
include/grl_hip.h fixes the order and the rounding of every operation."""
import ctypes as C
import functools

import pytest
import torch

from grl_image_restoration_amd import _lib as L
from grl_image_restoration_amd import ops, tiling
from grl_image_restoration_amd.geometry import tile_origins

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (h, w, tile, overlap, scale, b, c, tile_batch)
GEOMETRIES = {
    "9_per_pixel": (9, 11, 4, 2, 2, 2, 3, 3),        # origins [0,2,4,5] x [0,2,4,6,7]; chunks cut inside a tile row; b > 1
    "clamped_tile": (5, 7, 8, 2, 1, 1, 1, 8),        # the tile is clamped to 5: one tile row, one channel
    "scale_3": (7, 13, 5, 1, 3, 1, 3, 2),            # origins that are no multiples of 4 output pixels: unaligned tile loads
    "16_per_pixel": (9, 9, 4, 3, 1, 1, 1, 5),        # 6 x 6 tiles
    "wide_x4": (40, 72, 32, 8, 4, 1, 3, 2),          # the 16-byte path
    "two_workgroups_a_row": (8, 300, 8, 2, 4, 1, 1, 7),   # 1200 output columns: more than the 1024 one workgroup spans
}
WINDOWS = ("uniform", "linear", "cosine", "user")


def _window(kind, ts, ramp):
    if kind == "uniform":
        return None
    if kind == "user":
        return torch.rand(ts, generator=torch.Generator().manual_seed(ts)) * 0.9 + 0.1
    return tiling.blend_window(kind, ts, ramp)


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(tile, origins, CPU tile values, window, the yardstick) -- computed once and shared; nobody writes to them."""
    h, w, tile, overlap, scale, b, c, _ = GEOMETRIES[name]
    tile, origins = tiling.tile_list(h, w, tile, overlap)
    g = torch.Generator().manual_seed(len(origins))
    outs = [torch.randn(b, c, tile * scale, tile * scale, generator=g) for _ in origins]
    win = _window(kind, tile * scale, overlap * scale)
    return tile, origins, outs, win, tiling.stitch(outs, origins, (b, c, h, w), tile, scale, window=win)


def _views(outs):
    """The values of ``outs`` on the device behind strides: ``split`` views of one batch, a channel slice of a wider tensor, and
    views into a receive buffer with padded slots and padded rows (rows that are not 16-byte aligned)."""
    b, c, ts, _ = outs[0].shape
    n = len(outs)
    batch = torch.cat(outs, 0).to(DEV).split(b, dim=0)
    recv = torch.full((n + 2, b, c, ts, ts + 3), float("nan"), device=DEV)
    got = []
    for t, o in enumerate(outs):
        if t % 3 == 0:
            got.append(batch[t])
        elif t % 3 == 1:
            wide = torch.full((b, c + 2, ts, ts), float("nan"), device=DEV)
            wide[:, 1 : 1 + c] = o.to(DEV)
            got.append(wide[:, 1 : 1 + c])
        else:
            recv[t + 1, ..., :ts] = o.to(DEV)
            got.append(recv[t + 1, ..., :ts])
    return got


def _stitch(name, outs_dev, win, chunks, canvas=None):
    h, w, tile, overlap, scale, b, c, _ = GEOMETRIES[name]
    tile = min(tile, h, w)
    oy, ox = tile_origins(h, tile, overlap), tile_origins(w, tile, overlap)
    if canvas is None:
        canvas = torch.full((b, c, h * scale, w * scale), float("nan"), device=DEV)
    wd = None if win is None else win.to(DEV)
    for lo, hi in chunks:
        ops.tile_stitch(canvas, outs_dev[lo:hi], oy, ox, tile, scale, lo, wd)
    return canvas


@pytest.mark.parametrize("kind", WINDOWS)
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_kernel_equals_the_cpu_stitch(name, kind):
    """One call over [0, n), chunked calls in list order, and tiles behind strides, each into a canvas of NaN."""
    tile, origins, outs, win, want = case(name, kind)
    n, tb = len(origins), GEOMETRIES[name][7]
    chunks = [(s, min(s + tb, n)) for s in range(0, n, tb)]
    dev = [o.to(DEV) for o in outs]
    for what, tiles, ch in (("one call", dev, [(0, n)]), ("chunked", dev, chunks), ("views", _views(outs), chunks)):
        got = _stitch(name, tiles, win, ch).cpu()
        assert not bool(torch.isnan(got).any()), (what, int(torch.isnan(got).sum()))
        assert torch.equal(got, want), (what, int((got != want).sum()), float((got - want).abs().max()))


@pytest.mark.parametrize("kind", ["uniform", "linear"])
def test_negative_zero_comes_out_positive(kind):
    name = "wide_x4"
    tile, origins, outs, win, _ = case(name, kind)
    outs = [o.clone() for o in outs]
    outs[0][..., 0, 0] = -0.0                                  # the canvas corner: covered by tile 0 alone
    got = _stitch(name, [o.to(DEV) for o in outs], win, [(0, len(outs))]).cpu()
    assert bool((got[..., 0, 0] == 0).all()) and not bool(torch.signbit(got[..., 0, 0]).any())


def test_pixels_outside_the_chunk_keep_their_bits():
    name = "9_per_pixel"
    h, w, tile, overlap, scale, b, c, tb = GEOMETRIES[name]
    tile, origins, outs, win, _ = case(name, "linear")
    sentinel = 0x7FC12345
    canvas = torch.full((b, c, h * scale, w * scale), sentinel, dtype=torch.int32, device=DEV).view(torch.float32)
    _stitch(name, [o.to(DEV) for o in outs], win, [(0, tb)], canvas=canvas)
    covered = torch.zeros(h * scale, w * scale, dtype=torch.bool)
    for a, b_ in origins[:tb]:
        covered[a * scale : (a + tile) * scale, b_ * scale : (b_ + tile) * scale] = True
    bits = canvas.view(torch.int32).cpu()
    assert bool((bits[..., ~covered] == sentinel).all()) and 0 < int(covered.sum()) < covered.numel()
    assert not bool((bits[..., covered] == sentinel).any())


@pytest.mark.parametrize("name", ["scale_3", "9_per_pixel"])
def test_guard_bands_around_canvas_and_tile_hold(name):
    h, w, tile, overlap, scale, b, c, tb = GEOMETRIES[name]
    tile, origins, outs, win, want = case(name, "cosine")
    prev_guards = ops._GUARDS
    prev = ops.set_poison(True, guards=True)
    try:
        canvas = ops.empty(b, c, h * scale, w * scale, dtype=torch.float32, device=DEV)
        dev = [o.to(DEV) for o in outs]
        dev[-1] = ops.empty_like(dev[-1]).copy_(dev[-1])        # the last tile: a guarded buffer, the canvas's bottom right corner
        n = len(origins)
        _stitch(name, dev, win, [(s, min(s + tb, n)) for s in range(0, n, tb)], canvas=canvas)
    finally:
        ops.set_poison(prev, guards=prev_guards)
        ops.check_guards()
    assert torch.equal(canvas.cpu(), want)


class _Stub:
    """Nearest upsample plus an offset per tile (a quarter of the tile's first pixel): exact on either device."""

    def __init__(self, scale):
        self.scale = scale

    def __call__(self, x):
        up = x.repeat_interleave(self.scale, -2).repeat_interleave(self.scale, -1)
        return up + 0.25 * x[:, :1, :1, :1]


@pytest.mark.parametrize("blend", ["uniform", "linear"])
def test_forward_tiled_on_the_gpu_equals_the_cpu_run(blend):
    x = torch.rand(2, 3, 37, 50, generator=torch.Generator().manual_seed(3))
    model = _Stub(3)
    want = tiling.forward_tiled(model, x, 16, 5, 3, tile_batch=3, blend=blend)
    got = tiling.forward_tiled(model, x.to(DEV), 16, 5, 3, tile_batch=3, blend=blend)
    assert got.is_cuda and torch.equal(got.cpu(), want)


def test_peak_memory_is_the_canvas_and_one_chunk():
    """512 x 512 at x2 in tiles of 64: the canvas is 12.6 MB; E + W + every tile output would be more than three times that."""
    x = torch.rand(1, 3, 512, 512, device=DEV)
    model = _Stub(2)
    canvas_bytes = 3 * 1024 * 1024 * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = tiling.forward_tiled(model, x, 64, 8, 2, tile_batch=1)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise {rise / 2 ** 20:.1f} MiB, canvas {canvas_bytes / 2 ** 20:.1f} MiB")
    assert y.shape == (1, 3, 1024, 1024) and rise < 1.5 * canvas_bytes


@pytest.mark.parametrize("over", [dict(hi=21), dict(canvas=None), dict(ox=[0, 2, 4, 6, 8])], ids=["hi>n", "null_canvas", "tile_outside"])
def test_bad_arguments_launch_nothing(over):
    h, w, tile, overlap, scale, b, c, _ = GEOMETRIES["9_per_pixel"]
    tile, origins, outs, _, _ = case("9_per_pixel", "uniform")
    oy, ox = tile_origins(h, tile, overlap), tile_origins(w, tile, overlap)
    canvas = torch.full((b, c, h * scale, w * scale), 7.0, device=DEV)
    dev = [o.to(DEV) for o in outs]
    table = torch.tensor([[o.data_ptr(), *o.stride()[:3], 0, 0, 0, 0] for o in dev], dtype=torch.int64).to(DEV)
    kw = dict(canvas=canvas.data_ptr(), tiles=table.data_ptr(), win=None, b=b, c=c, h=h, w=w, tile=tile, scale=scale, ny=len(oy),
              nx=len(ox), lo=0, hi=len(origins))
    kw.update({k: v for k, v in over.items() if k != "ox"})
    args = L.GrlTileStitchArgs(**kw)
    for dst, src in ((args.oy, oy), (args.ox, over.get("ox", ox))):
        for i, v in enumerate(src):
            dst[i] = v
    assert L.lib().grl_tile_stitch(L.stream_ptr(), C.byref(args)) == -1
    torch.cuda.synchronize()
    assert bool((canvas == 7.0).all())
