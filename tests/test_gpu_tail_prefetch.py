"""The register-resident block tail's next-tile prefetch (csrc/tail_regs.hip: load_next / store_next of the fc1-only waves).

The persistent grid is min(M / 32, 256) workgroups, so a launch over at most 256 tiles (M <= 8192) never prefetches, and a
tile's result does not depend on which launch computed it.  One launch over M tokens must therefore equal, BIT FOR BIT, the
concatenation of launches over consecutive sub-ranges of at most 8192 tokens: a stale, late or misplaced prefetched tile
cannot match (the inputs are seeded random).  The sub-ranges are whole images with their own rows of `gate`; an image longer
than 8192 tokens is cut into pieces that each count as one image with that image's gate row (the image index only selects
the gate row).  C = 180, hidden 360, res_scale 0.5, operands built as in test_gpu_kernels.py::test_fused_block_tail.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C, HD, CP, HP = 180, 360, 192, 384
NOPF = 8192   # tokens: at most 256 tiles, one per workgroup


def _dev():
    return torch.device("cuda:0")


def _pad(t, n):
    return torch.cat([t, torch.zeros(*t.shape[:-1], n - t.shape[-1])], dim=-1)


@functools.lru_cache(maxsize=None)
def _weights():
    from grl_image_restoration_amd import ops

    g = torch.Generator().manual_seed(21)
    w = dict(wp=torch.zeros(CP, CP))
    w["wp"][:C] = torch.randn(C, CP, generator=g) / math.sqrt(CP)
    w["bp"] = _pad(0.1 * torch.randn(C, generator=g), CP)
    w["g1"], w["b1n"] = _pad(1 + 0.1 * torch.randn(C, generator=g), CP), _pad(0.1 * torch.randn(C, generator=g), CP)
    w["w1"] = torch.randn(HD, C, generator=g) / math.sqrt(C)
    w["b1"] = 0.1 * torch.randn(HD, generator=g)
    w["w2"] = torch.randn(C, HD, generator=g) / math.sqrt(HD)
    w["b2"] = _pad(0.1 * torch.randn(C, generator=g), CP)
    w["g2"], w["b2n"] = _pad(1 + 0.1 * torch.randn(C, generator=g), CP), _pad(0.1 * torch.randn(C, generator=g), CP)
    d = _dev()
    dw = {k: v.to(d) for k, v in w.items()}
    dw["blob"] = ops.pack_mlp(dw["w1"], dw["b1"], dw["w2"], CP, HP)
    dw["pblob"] = ops.pack_proj(dw["wp"])
    dw["rblob"] = ops.pack_tail_regs(dw["wp"], dw["w1"], dw["b1"], dw["w2"])
    return w, dw


@functools.lru_cache(maxsize=None)
def _inputs(M, rpi):
    g = torch.Generator().manual_seed(1000 + M + rpi)
    x = _pad(torch.randn(M, C, generator=g), CP)
    att = torch.randn(M, CP, generator=g).to(torch.float16)
    cab = _pad(torch.randn(M, C, generator=g), CP).to(torch.float16)
    gate = _pad(torch.rand((M + rpi - 1) // rpi, C, generator=g), CP)
    d = _dev()
    return (x, att, cab, gate), (x.to(d), att.to(d), cab.to(d), gate.to(d))


def _tail(att, x, cab, gate, rpi):
    from grl_image_restoration_amd import ops

    _, w = _weights()
    return ops.block_tail(att, x, cab, gate, rpi, w["pblob"], w["bp"], w["g1"], w["b1n"], w["blob"], w["b2"], w["g2"], w["b2n"],
                          Hpad=HP, n_real=C, res_scale=0.5, rblob=w["rblob"])


@functools.lru_cache(maxsize=None)
def _one_launch(M, rpi):
    _, (x, att, cab, gate) = _inputs(M, rpi)
    return _tail(att, x, cab, gate, rpi)


def _pieces(M, rpi):
    """(lo, hi, first image, rows_per_image of the piece) of consecutive sub-ranges of at most NOPF tokens."""
    out = []
    if rpi <= NOPF:
        step = NOPF // rpi * rpi
        for lo in range(0, M, step):
            out.append((lo, min(lo + step, M), lo // rpi, rpi))
    else:
        for img0 in range(0, M, rpi):
            for lo in range(img0, min(img0 + rpi, M), NOPF):
                hi = min(lo + NOPF, img0 + rpi, M)
                out.append((lo, hi, img0 // rpi, NOPF))      # the piece is (part of) one image
    return out


def _piecewise(M, rpi):
    _, (x, att, cab, gate) = _inputs(M, rpi)
    outs = []
    for lo, hi, img, sub_rpi in _pieces(M, rpi):
        assert hi - lo <= NOPF and lo % 32 == 0
        nimg = (hi - lo + sub_rpi - 1) // sub_rpi     # (the last image of M may be a partial one)
        outs.append(_tail(att[lo:hi], x[lo:hi], cab[lo:hi], gate[img:img + nimg].contiguous(), sub_rpi))
    return torch.cat(outs)


# rows_per_image 128 is the smallest grl_block_tail_fwd accepts (include/grl_hip.h).  A workgroup's consecutive tiles are 256
# tiles = 64 such images apart, so with it the gate row changes -- and the gate-staging barrier runs -- on EVERY tile of every
# workgroup, exactly as it would with one image per tile.
SHAPES = [
    (32 * 257, 128),         # one workgroup has two tiles, 255 have one: both outcomes of `next < ntiles`; the gate changes on every tile
    (32 * 512, 32 * 16),     # two tiles everywhere
    (32 * 773, 32 * 773),    # one image, three or four tiles per workgroup: both buffer parities reused with loads in flight
    (32 * 773, 128),         # the gate-staging barrier on every tile, inside both flight windows
    (32 * 769, 32 * 769),    # one workgroup has four tiles, the rest three
    (32, 128),               # single tile
    (32 * 256, 32 * 256),    # one tile per workgroup: no prefetch (trivially equal; guards of the single-tile path)
]


@pytest.mark.parametrize("M,rpi", SHAPES)
def test_one_launch_equals_prefetch_free_launches(M, rpi):
    one = _one_launch(M, rpi)
    parts = _piecewise(M, rpi)
    torch.cuda.synchronize()
    assert one.shape == parts.shape
    if not torch.equal(one, parts):
        bad = (one != parts).any(dim=1).nonzero().flatten()
        raise AssertionError(f"{bad.numel()} of {M} tokens differ; first tiles {sorted(set((bad // 32).tolist()))[:8]}, "
                             f"max |diff| {(one - parts).abs().max().item():.3e}")


def test_prefetching_launch_within_tolerances():
    """The tolerances of test_fused_block_tail on a launch with three or four tiles per workgroup: < 3e-3 against fp64 torch on
    the fp16-rounded operands, < 2e-3 against the separate kernels, pad channels exactly 0."""
    from grl_image_restoration_amd import _lib as L, ops

    M = rpi = 32 * 773
    (x, att, cab, gate), (dx, datt, dcab, dgate) = _inputs(M, rpi)
    w, dw = _weights()
    out = _one_launch(M, rpi).cpu()
    r1 = ops.linear(datt, dw["wp"].to(torch.float16), dw["bp"], epi=L.EPI_LN_RES, out_dtype=torch.float32, ln_g=dw["g1"], ln_b=dw["b1n"],
                    n_real=C, res_scale=0.5, resid=dx, add2=dcab, add2_scale=dgate, rows_per_image=rpi)
    out2 = ops.mlp(r1, dw["blob"], dw["b2"], dw["g2"], dw["b2n"], Hpad=HP, n_real=C, res_scale=0.5).cpu()
    assert (out - out2).abs().max().item() < 2e-3
    h16 = lambda t: t.to(torch.float16).double()
    y = att.double() @ h16(w["wp"][:C]).t() + w["bp"][:C].double()
    gr = gate[torch.arange(M) // rpi][:, :C].double()
    r1r = x[:, :C].double() + 0.5 * F.layer_norm(y, (C,), w["g1"][:C].double(), w["b1n"][:C].double(), 1e-5) + cab[:, :C].double() * gr
    hid = F.gelu(h16(r1r.float()) @ h16(w["w1"]).t() + w["b1"].double())
    y2 = h16(hid.float()) @ h16(w["w2"]).t() + w["b2"][:C].double()
    ref = r1r + 0.5 * F.layer_norm(y2, (C,), w["g2"][:C].double(), w["b2n"][:C].double(), 1e-5)
    assert (out[:, :C].double() - ref).abs().max().item() < 3e-3
    assert out[:, C:].abs().max().item() == 0.0


def test_prefetching_launch_repeats_bit_for_bit():
    M = rpi = 32 * 773
    _, (x, att, cab, gate) = _inputs(M, rpi)
    first = _one_launch(M, rpi)
    again = _tail(att, x, cab, gate, rpi)
    assert torch.equal(first, again)
    M, rpi = 32 * 773, 128
    _, (x, att, cab, gate) = _inputs(M, rpi)
    assert torch.equal(_one_launch(M, rpi), _tail(att, x, cab, gate, rpi))
