"""grl_blur_depthwise (csrc/blur.hip) through tasks.py on the MI355X: against the reference fixture (tests/golden/tasks/db.npz) in every
input form, against the CPU path at the shapes the fixture does not hold, determinism, the two padding modes against each other,
bad arguments, graph capture, the db sampler, and the evaluate / train CLIs end to end.  The bound is tests/test_blur.py's:
(K^2 + 2) 2^-24 max(1, max|x|) against a float64 result, twice that against the reference's fp32 LQ."""
import ctypes as C

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, PatchSampler, PatchStore, _lib, evaluate as EV, make_config, tasks as T, train
from oracle import grl_oracle as O
from tests.test_blur import bound, check_lq, db_case, db_cases
from tests.test_tasks import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TH, TW = 32, 64                      # the kernel's output tile (csrc/blur.hip); a lane owns 8 adjacent outputs of a row


def _forms(x):
    """The same batch as a contiguous tensor, a strided crop of a larger tensor and a channels_last tensor, on the device."""
    N, Cn, H, W = x.shape
    big = torch.rand(N + 1, Cn + 2, H + 3, W + 5).to(DEV)
    big[1:, 1 : 1 + Cn, 2 : 2 + H, 3 : 3 + W] = x.to(DEV)
    crop = big[1:, 1 : 1 + Cn, 2 : 2 + H, 3 : 3 + W]
    cl = x.to(DEV).contiguous(memory_format=torch.channels_last)
    assert not crop.is_contiguous() and (Cn == 1 or H * W == 1 or cl.stride(1) == 1)
    return {"contiguous": x.to(DEV), "crop": crop, "channels_last": cl}


@pytest.mark.parametrize("name", db_cases())
def test_hip_blur_matches_the_reference_in_every_input_form(name):
    c, gt, taps, noise, lq32, lq64 = db_case(name)
    K = taps.shape[0]
    first = None
    for form, x in _forms(gt).items():
        if c["pad"] == "same":
            got = T.db_lq(x, taps.to(DEV), noise.to(DEV))
        else:
            got, center = T.blur(x, taps.to(DEV), "valid", add=noise.to(DEV), want_center=True)
            Ho, Wo = gt.shape[2] - K + 1, gt.shape[3] - K + 1
            assert center.is_contiguous() and torch.equal(center.cpu(), gt[..., K // 2 : K // 2 + Ho, K // 2 : K // 2 + Wo]), form
        assert got.is_cuda and got.is_contiguous()
        check_lq(got, name, f"hip {form}")
        first = got if first is None else first
        assert torch.equal(got, first), form                                   # the input's layout does not change a bit
    # the noise as a strided view, and broadcast over the batch
    wide = torch.zeros(noise.shape[:-1] + (noise.shape[-1] + 3,), device=DEV)
    wide[..., 2 : 2 + noise.shape[-1]] = noise.to(DEV)
    again = T.blur(gt.to(DEV), taps.to(DEV), c["pad"], add=wide[..., 2 : 2 + noise.shape[-1]])
    assert torch.equal(again, first)


# shapes the fixture does not hold: three tiles each way with ragged last tiles; N * C = 48 planes; the same two over the valid region
EXTRA = [("ragged_same", "gaussian", (1, 3, 2 * TH + 5, 2 * TW + 7), "same"), ("planes48_same", "real5", (16, 3, 32, 32), "same"),
         ("ragged_valid", "real5", (1, 3, 2 * TH + 5 + 12, 2 * TW + 7 + 12), "valid"), ("planes48_valid", "real4", (16, 3, 40, 33), "valid")]
_EXTRA = {}


def extra_case(name):
    """(x, taps, add, the CPU path's result) computed once."""
    if name not in _EXTRA:
        _, kernel, shape, pad = next(e for e in EXTRA if e[0] == name)
        g = torch.Generator().manual_seed(len(name))
        x = torch.randint(0, 256, shape, generator=g).float() / 255
        taps = golden("db")[1][f"taps_{kernel}"]
        K = taps.shape[0]
        oshape = shape if pad == "same" else shape[:2] + (shape[2] - K + 1, shape[3] - K + 1)
        add = torch.randn(oshape, generator=g) * (2 / 255)
        _EXTRA[name] = (x, taps, add, pad, T.blur(x, taps, pad, add=add))
    return _EXTRA[name]


@pytest.mark.parametrize("name", [e[0] for e in EXTRA])
def test_hip_blur_matches_the_cpu_path(name):
    x, taps, add, pad, want = extra_case(name)
    got = T.blur(x.to(DEV), taps.to(DEV), pad, add=add.to(DEV))
    err, b = float((got.cpu() - want).abs().max()), bound(taps.shape[0], x)
    print(f"{name}: |hip - cpu| {err:.3e}, bound {b:.3e}")
    assert got.shape == want.shape and err <= b
    assert torch.equal(T.blur(x.to(DEV), taps.to(DEV), pad, add=add.to(DEV)), got)          # two runs: bit-identical
    if pad == "valid":
        lq, center = T.blur(x.to(DEV), taps.to(DEV), "valid", want_center=True)
        K = taps.shape[0]
        Ho, Wo = lq.shape[-2:]
        inner = (Ellipsis, slice(K // 2, K // 2 + Ho), slice(K // 2, K // 2 + Wo))
        assert torch.equal(lq, T.blur(x.to(DEV), taps.to(DEV), "same")[inner])              # the reference's blur-then-crop, bitwise
        assert torch.equal(center.cpu(), x[inner])


def test_one_tap_and_small_kernels():
    x = torch.rand(2, 3, 37, 70)
    one = torch.ones(1, 1)
    assert torch.equal(T.blur(x.to(DEV), one.to(DEV)).cpu(), x)
    for K in (3, 31):
        taps = torch.rand(K, K)
        taps = (taps / taps.sum()).float()
        got = T.blur(x.to(DEV), taps.to(DEV)).cpu()
        assert float((got - T.blur(x, taps)).abs().max()) <= bound(K, x), K


def test_bad_arguments_raise_without_a_fault():
    x = torch.rand(1, 3, 20, 20, device=DEV)
    taps = lambda K: torch.full((K, K), 1.0 / (K * K), device=DEV)
    with pytest.raises(ValueError):
        T.blur(x, taps(4))                                                     # even K
    with pytest.raises(ValueError):
        T.blur(x, taps(33))
    with pytest.raises(ValueError):
        T.blur(x, taps(25), "valid")                                           # H < K
    with pytest.raises(ValueError):
        T.blur(x, taps(5), "same", want_center=True)
    with pytest.raises(TypeError):
        T.blur(x.half(), taps(5))
    # the same through the library itself
    for K, pad, center in ((4, 2, False), (33, 16, False), (25, 0, False), (5, 2, True), (5, 1, False)):
        with pytest.raises(RuntimeError, match="bad argument"):
            T.hip_blur(x, taps(K), pad, None, center)
    with pytest.raises(TypeError):
        T.hip_blur(x.half(), taps(5), 2)
    L = _lib.lib()
    out = torch.empty(1, 3, 20, 20, device=DEV)
    good = dict(x=x.data_ptr(), stride=(C.c_int64 * 4)(*x.stride()), N=1, C=3, H=20, W=20, taps=taps(5).data_ptr(), K=5, pad=2,
                out=out.data_ptr())
    call = lambda **kw: L.grl_blur_depthwise(_lib.stream_ptr(), C.byref(_lib.GrlBlurArgs(**dict(good, **kw))))
    assert call() == 0
    for kw in (dict(x=None), dict(taps=None), dict(out=None), dict(N=0), dict(C=0), dict(H=0), dict(W=-1), dict(K=0), dict(K=-3)):
        assert call(**kw) == -1, kw
    assert call(N=1 << 30, C=1 << 10) == -1                                     # beyond 2^31 - 1 workgroups
    assert L.grl_blur_depthwise(_lib.stream_ptr(), None) == -1
    torch.cuda.synchronize()


def test_replay_from_a_graph_follows_the_buffers():
    c, gt, taps, noise, lq32, lq64 = db_case("r4_40x56")
    x, add, t = torch.zeros_like(gt, device=DEV), torch.zeros_like(noise, device=DEV), taps.to(DEV)
    T.blur(x, t, "same", add=add)                                              # loads the library outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = T.blur(x, t, "same", add=add)
    x.copy_(gt)
    add.copy_(noise)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, T.blur(gt.to(DEV), t, "same", add=noise.to(DEV)))
    check_lq(out, "r4_40x56", "hip graph replay")


def test_db_sampler_on_a_cuda_store():
    """The CUDA store's batch against the CPU store's for one work list and one noise tensor: ``gt`` bitwise; ``lq`` bitwise against
    the device blur of the CPU store's enlarged patches (the sampler adds nothing of its own), and within the bound of the CPU
    sampler's ``lq`` -- the CPU path sums the taps in float64, so the two LQs differ by the fp32 chain's rounding."""
    from tests.test_blur import _store_images

    taps = golden("db")[1]["taps_real5"]
    K, P, B = taps.shape[0], 16, 5
    imgs = _store_images()
    work = [(1, 0, 0, 0), (1, 0, 22, 3), (0, 32, 42, 0), (0, 5, 7, 4), (0, 0, 0, 6)]
    noise = torch.randn(B, 3, P, P, generator=torch.Generator().manual_seed(2))
    cpu = PatchSampler("db", PatchStore(imgs), patch=P, batch=B, taps=taps, sigma=2)
    gpu = PatchSampler("db", PatchStore(imgs, DEV), patch=P, batch=B, taps=taps, sigma=2)
    want_lq, want_gt = cpu.next(work, noise=noise)
    lq, gt = gpu.next(work, noise=noise.to(DEV))
    assert lq.is_cuda and lq.shape == (B, 3, P, P) and torch.equal(gt.cpu(), want_gt)
    big = PatchStore(imgs).sample(torch.tensor(work, dtype=torch.int32), P + K - 1, 1)
    assert torch.equal(lq, T.blur(big.to(DEV), taps.to(DEV), "valid", add=noise.to(DEV) * (2 / 255)))
    assert float((lq.cpu() - want_lq).abs().max()) <= bound(K, big)
    a, b = gpu.next(), gpu.next()                                               # the generator lives on the device and advances
    assert a[0].shape == (B, 3, P, P) and not torch.equal(a[0], b[0])


def _folder(tmp_path):
    from PIL import Image

    raw = golden("db")[1]["g_40x56_b2__gt"]
    d = tmp_path / "set5"
    d.mkdir()
    for n in range(2):
        Image.fromarray(raw[n].permute(1, 2, 0).numpy()).save(d / f"im{n}.png")
    return d


def test_evaluate_cli_db(tmp_path, capsys):
    c, gt, taps, noise, lq32, lq64 = db_case("g_40x56_b2")
    cfg = make_config("tiny", "dn_df4")
    model = GRL(**cfg).eval()
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1)
    model.load_state_dict(sd, strict=True)
    ck = tmp_path / "db.ckpt"
    torch.save({"params": sd}, ck)
    d = _folder(tmp_path)
    want = EV.evaluate_pairs(model.to(DEV), [(lq32[n : n + 1], gt[n : n + 1]) for n in range(2)], 1, device=DEV)
    got = EV.main(["--task", "db", "--model", "tiny", "--geometry", "dn_df4", "--ckpt", str(ck), "--gt", str(d)])
    out = capsys.readouterr().out
    assert "im0.png" in out and "im1.png" in out and "mean over 2 images" in out
    print(f"evaluate --task db: mean PSNR-Y {got:.4f} dB, on the reference's LQ {sum(want) / 2:.4f} dB")
    assert abs(got - sum(want) / 2) <= 0.01
    items = list(EV.task_inputs(str(d), "db", device=DEV))
    for n, (_, lq, g) in enumerate(items):
        assert lq.is_cuda and torch.equal(g, gt[n : n + 1])
        assert float((lq.cpu().double() - lq64[n : n + 1]).abs().max()) <= bound(25, gt)


def test_train_cli_db(tmp_path, capsys):
    d = _folder(tmp_path)
    args = ["--task", "db", "--model", "tiny", "--geometry", "yaml", "--depths", "1+1", "--patch", "16", "--batch", "2", "--gt", str(d),
            "--lr", "2e-4"]
    torch.manual_seed(0)
    r = train.main(args + ["--steps", "3", "--eager", "--out", str(tmp_path / "eager")])
    assert r["steps"] == [0, 1, 2] and all(np.isfinite(r["losses"]))
    assert r["checkpoint"] == str(tmp_path / "eager" / "step_3.ckpt")
    obj = torch.load(r["checkpoint"], map_location="cpu", weights_only=False)
    assert obj["step"] == 3 and obj["args"]["task"] == "db" and obj["sampler_rng"]["noise"] is not None
    assert all(x <= 40 - 40 and y <= 56 - 40 for w in r["work"] for _, x, y, _ in w)          # the draws use P' = 16 + 24
    torch.manual_seed(0)
    c = train.main(args + ["--steps", "3", "--out", str(tmp_path / "graph")])              # the captured step fed by the sampler
    assert c["steps"] == [0, 1, 2] and all(np.isfinite(c["losses"])) and c["work"] == r["work"]
    assert c["losses"][0] == pytest.approx(r["losses"][0], rel=1e-3)                       # step 0 is the same eager step
    assert c["checkpoint"] == str(tmp_path / "graph" / "step_3.ckpt")
    obj = torch.load(c["checkpoint"], map_location="cpu", weights_only=False)
    assert all(bool(torch.isfinite(v).all()) for v in obj["state_dict"].values())
    capsys.readouterr()
