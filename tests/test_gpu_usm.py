"""GPU tests of ``grl_usm_sharp`` (csrc/usm.hip) through ``tasks.usm_sharp``, ``PatchSampler(usm=True)`` and
``evaluate_folder(usm_gt=True)``.  The fixture, the yardstick and the derivation of every tolerance: tests/test_usm.py's docstring.
In short: blur within 2 gamma_51 = 6.1e-6 (plus 2^-32, the rounding of the fixture's 2^-31 grid), the mask exact at the decided threshold, the result within
6.4e-6, 8-bit levels different only within 1.8e-3 of a half-integer level and by one."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, PatchSampler, PatchStore, _lib, evaluate as EV, make_config, tasks as T
from grl_image_restoration_amd.image8 import pack8
from oracle import grl_oracle as O
from tests.test_usm import BLUR_TOL, CASES, HALF_BAND, OUT_TOL, U24, Fixture, check_levels, reference_at

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.mark.parametrize("name", CASES)
def test_kernel_on_the_fixture_at_the_decided_threshold(fx, name):
    c = fx.cases[name]
    x = c["x"].to(DEV)
    out, blur, mask = T.usm_sharp(x, threshold=c["threshold"], parts=True)
    torch.cuda.synchronize()
    eb = np.abs(blur.double().cpu().numpy() - c["blur"]).max()
    eo = np.abs(out.double().cpu().numpy() - c["out"]).max()
    print(f"{name}: max|blur - float64| = {eb:.3e} (bound {BLUR_TOL:.3e}), max|out - float64| = {eo:.3e} (bound {OUT_TOL:.1e})")
    assert eb <= BLUR_TOL
    m = mask.cpu().numpy()
    assert set(np.unique(m)) <= {0.0, 1.0} and np.array_equal(m != 0, c["mask"])
    assert eo <= OUT_TOL
    q = T.usm_sharp(x, threshold=c["threshold"], quantise=True)
    print(f"{name}: {check_levels((q * 255).round().cpu().numpy(), c)} levels differ near a half-integer")


@pytest.mark.parametrize("name", ("A", "B"))
def test_kernel_at_the_default_threshold(fx, name):
    c = fx.cases[name]
    want_mask, want = reference_at(c, fx.taps, 10.0)
    out, _, mask = T.usm_sharp(c["x"].to(DEV), parts=True)
    assert not ((mask.cpu().numpy() != 0) != want_mask)[~c["undecided"]].any()
    err = np.abs(out.double().cpu().numpy() - want).max()
    print(f"{name} at threshold 10: max|out - float64| = {err:.3e}")
    assert err <= OUT_TOL + c["U"] * float(fx.taps.max()) ** 2 * 0.5


@pytest.mark.parametrize("name", ("B", "D", "E1"))
def test_quantise_is_the_8_bit_pack_of_the_plain_result(fx, name):
    x = fx.cases[name]["x"].to(DEV)
    q, plain = T.usm_sharp(x, quantise=True), T.usm_sharp(x)
    # the division on the CPU: torch divides a CUDA tensor by a scalar through the reciprocal
    assert torch.equal(q.cpu(), pack8(plain).cpu().permute(0, 3, 1, 2).float().div(255))
    assert not torch.equal(q, plain)


def test_a_plane_does_not_depend_on_its_place_in_the_batch(fx):
    x = fx.cases["C"]["x"].to(DEV)                           # (2, 1, 33, 64)
    both = T.usm_sharp(x)
    for n in range(2):
        assert torch.equal(T.usm_sharp(x[n : n + 1].contiguous())[0], both[n])
    assert torch.equal(T.usm_sharp(x.flip(0).contiguous()), both.flip(0))
    rgb = torch.stack([x[1, 0], x[0, 0], x[1, 0]])[None].contiguous()          # the same planes as channels of one sample
    got = T.usm_sharp(rgb)
    assert torch.equal(got[0, 0], both[1, 0]) and torch.equal(got[0, 1], both[0, 0]) and torch.equal(got[0, 2], both[1, 0])
    big = fx.cases["A"]["x"].to(DEV)                         # several tiles: next to another plane, the same bits
    pair = T.usm_sharp(torch.cat([big, big.flip(-1)]).contiguous())
    assert torch.equal(pair[0], T.usm_sharp(big)[0])


@pytest.mark.parametrize("K", (1, 3, 31, 63))
def test_other_kernel_sizes_against_the_cpu_restatement(K):
    """K from 1 to the largest the entry takes (its LDS tile is sized by K), on 70 x 45 and on 8 x 150, at a DECIDED threshold: the
    middle of the widest gap of the float64 |res| * 255 between 9 and 11, which has to be further than margin_K = 255 * 2 gamma_K +
    1e-5 from every value.  Then the blur is within 2 gamma_K, the mask is exact, and the result is within 2 gamma_K + 4 u of the
    float64 one (+ u / 2 for the CPU path's rounding to fp32), as tests/test_usm.py derives for K = 51."""
    g = torch.Generator().manual_seed(K)
    i = torch.arange(K, dtype=torch.float64) - K // 2
    taps = torch.exp(-i * i / (2 * (0.15 * K + 0.35) ** 2))
    taps = (taps / taps.sum()).float()
    gamma = K * U24 / (1 - K * U24)
    for shape in ((1, 3, 70, 45), (2, 1, 8, 150)):
        x = torch.randint(0, 256, shape, generator=g).float().div(255)
        v = ((x.double() - T._torch_usm(x, taps, 0.5, 10.0, False, True)[1]).abs() * 255).flatten()
        inside = torch.cat([torch.tensor([9.0, 11.0], dtype=torch.float64), v[(v > 9) & (v < 11)]]).sort().values
        j = int(inside.diff().argmax())
        thr = float((inside[j] + inside[j + 1]) / 2)
        assert float((v - thr).abs().min()) > 255 * 2 * gamma + 1e-5
        out, blur, mask = T.hip_usm(x.to(DEV), taps.to(DEV), 0.5, thr, parts=True)
        wout, wblur, wmask = T._torch_usm(x, taps, 0.5, thr, False, True)
        eb = float((blur.double().cpu() - wblur).abs().max())
        eo = float((out.double().cpu() - wout.double()).abs().max())
        print(f"K = {K} {shape} threshold {thr:.4f}: max|blur - float64| = {eb:.3e} (bound {2 * gamma + U24:.3e}), "
              f"max|out - cpu| = {eo:.3e} (bound {2 * gamma + 4.5 * U24:.3e})")
        assert eb <= 2 * gamma + U24
        assert torch.equal(mask.cpu().double(), wmask)
        assert eo <= 2 * gamma + 4.5 * U24


def test_bad_arguments_are_rejected_without_a_launch():
    L = _lib.lib()
    x = torch.rand(1, 3, 16, 16, device=DEV)
    taps = T.usm_taps().to(DEV)
    ws = torch.empty(2, 1, 3, 16, 16, device=DEV)
    out = torch.full((1, 3, 16, 16), 7.0, device=DEV)
    good = dict(x=x.data_ptr(), taps=taps.data_ptr(), N=1, C=3, H=16, W=16, K=51, quantise=0, weight=0.5, threshold=10.0,
                workspace=ws.data_ptr(), out=out.data_ptr())
    call = lambda **kw: L.grl_usm_sharp(_lib.stream_ptr(), C.byref(_lib.GrlUsmArgs(**dict(good, **kw))))
    for kw in (dict(K=50), dict(K=65), dict(K=0), dict(K=-1), dict(C=2), dict(C=0), dict(workspace=None), dict(x=None), dict(taps=None),
               dict(out=None), dict(N=0), dict(H=0), dict(W=-3), dict(out=out.data_ptr() + 2), dict(taps=taps.data_ptr() + 1)):
        assert call(**kw) == -1, kw
    assert L.grl_usm_sharp(_lib.stream_ptr(), None) == -1
    assert L.grl_usm_workspace_bytes(1, 3, 16, 16) == 2 * 4 * 3 * 16 * 16
    assert L.grl_usm_workspace_bytes(1, 2, 16, 16) == -1 and L.grl_usm_workspace_bytes(0, 3, 16, 16) == -1
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0                       # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, T.usm_sharp(x))


def test_replay_from_a_graph_follows_the_taps(fx):
    x = fx.cases["D"]["x"].to(DEV)
    taps = T.usm_taps().to(DEV)
    other = T.usm_taps().flip(0).roll(3).contiguous()           # another 51-tap table, not symmetric
    want_a, want_b = T.hip_usm(x, taps.clone()), T.hip_usm(x, other.to(DEV))
    assert not torch.equal(want_a, want_b)
    out = torch.empty_like(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.hip_usm(x, taps, out=out)                              # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        T.hip_usm(x, taps, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_a)
    taps.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_b)


def test_usm_sharp_is_capturable_once_the_taps_are_on_the_device(fx):
    x = fx.cases["E1"]["x"].to(DEV)
    want = T.usm_sharp(x)                                    # also puts the default taps on the device
    assert T.usm_device_taps(50, x.device) is T.usm_device_taps(50, DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = T.usm_sharp(x)
    got.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def _near_half(x):
    """Pixels of an (N, C, H, W) image whose sharpened level may round either way (from the CPU path's float64 blend)."""
    level = T.usm_sharp(x).double().clamp(0, 1) * 255.0
    return ((level - level.floor() - 0.5).abs() <= HALF_BAND)[0].permute(1, 2, 0)


def test_usm_sampler_on_a_cuda_store(fx):
    g = np.random.RandomState(3)
    gts = [np.ascontiguousarray(fx.cases["B"]["x8"][0].transpose(1, 2, 0)), g.randint(0, 256, (24, 40, 3)).astype(np.uint8)]
    lqs = [np.ascontiguousarray(im[::2, ::2]) for im in gts]
    make = lambda dev: PatchSampler("sr", PatchStore(gts, dev), PatchStore(lqs, dev), patch=8, batch=4, scale=2, seed=5, usm=True)
    cpu, gpu = make("cpu"), make(DEV)
    assert gpu.gt_store.device.type == "cuda" and gpu.gt_store.dims == cpu.gt_store.dims
    for n, im in enumerate(gts):
        a, b = gpu.gt_store.image(n).cpu().to(torch.int16), cpu.gt_store.image(n).to(torch.int16)
        near = _near_half(torch.from_numpy(im).permute(2, 0, 1)[None].float().div(255))
        diff = a != b
        print(f"image {n}: {int(diff.sum())} of {diff.numel()} levels differ between the CUDA and the CPU store")
        assert not (diff & ~near).any() and int((a - b).abs().max()) <= 1
        assert torch.equal(gpu.lq_store.image(n).cpu(), cpu.lq_store.image(n))
    work = cpu.draw()
    assert work == gpu.draw()
    (lq_c, _), (lq_g, gt_g) = cpu.next(*work), gpu.next(*work)
    assert torch.equal(lq_g.cpu(), lq_c) and gt_g.is_cuda and torch.equal(gt_g, gpu.gt_store.sample(gpu.work, 8, 2))


def test_evaluate_folder_usm_gt_on_the_device(fx, tmp_path):
    from PIL import Image

    gt8 = np.ascontiguousarray(fx.cases["B"]["x8"][0].transpose(1, 2, 0))[:48, :56]
    lq8 = np.ascontiguousarray(gt8[::2, ::2])
    (tmp_path / "lq").mkdir()
    (tmp_path / "gt").mkdir()
    Image.fromarray(lq8).save(tmp_path / "lq" / "a.png")
    Image.fromarray(gt8).save(tmp_path / "gt" / "a.png")
    model = GRL(**make_config("tiny", "dm", upscale=2, depths=[1], num_heads_window=[2], num_heads_stripe=[2])).eval()
    model.load_state_dict(O.seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1), strict=True)
    model = model.to(DEV)
    lq = torch.from_numpy(lq8).permute(2, 0, 1)[None].float().div(255)
    gt = torch.from_numpy(gt8).permute(2, 0, 1)[None].float().div(255)
    with torch.no_grad():
        got = EV.evaluate_folder(model, str(tmp_path / "lq"), str(tmp_path / "gt"), 2, device=DEV, verbose=False, usm_gt=True,
                                 save_dir=str(tmp_path / "out"), save_gt=True)
        off = EV.evaluate_folder(model, str(tmp_path / "lq"), str(tmp_path / "gt"), 2, device=DEV, verbose=False)
        sharp_cpu = T.usm_sharp(gt, quantise=True)
        sharp_gpu = T.usm_sharp(gt.to(DEV), quantise=True)
        want = EV.evaluate_pairs(model, [(lq, sharp_gpu)], 2, device=DEV)[0]
    assert got == want and got != off
    saved = torch.from_numpy(np.asarray(Image.open(tmp_path / "out" / "X2" / "gt" / "a_GT.png")).copy())
    assert torch.equal(saved, pack8(sharp_gpu)[0].cpu())
    a, b = saved.to(torch.int16), pack8(sharp_cpu)[0].to(torch.int16)
    assert not ((a != b) & ~_near_half(gt)).any() and int((a - b).abs().max()) <= 1
