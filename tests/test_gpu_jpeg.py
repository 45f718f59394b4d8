"""The JPEG round trip on the MI355X (csrc/jpeg.hip through tasks.hip_jpeg) -- needs the GPU.  Everything is integer arithmetic,
so every comparison is ``torch.equal``: against the CPU restatement ``tasks._torch_jpeg`` (int64) and against
tests/golden/tasks/jpeg_roundtrip.npz (Pillow's libjpeg-turbo).  The 0 / 255 checkerboards at quality 100 and 1 are where an int32
overflow of the kernel would show against the int64 restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, PatchSampler, PatchStore, _lib, evaluate as EV, make_config, tasks as T, train
from oracle import grl_oracle as O
from tests.test_jpeg import WORK, jpeg_case, jpeg_cases, levels, pattern, store_images

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", jpeg_cases())
def test_hip_jpeg_equals_the_cpu_restatement_and_the_fixture(name):
    """A batch of three images with three qualities in one call."""
    c, x, quality, want = jpeg_case(name)
    got = T.jpeg_roundtrip(x.to(DEV), quality)
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == x.shape
    cpu = T._torch_jpeg(x, torch.tensor(quality, dtype=torch.int32))
    assert torch.equal(got.cpu(), cpu), (name, int((got.cpu() != cpu).sum()))
    assert torch.equal(levels(got.cpu()), want), name
    q = torch.tensor(quality, dtype=torch.int32, device=DEV)
    assert torch.equal(T.jpeg_roundtrip(x.to(DEV), q), got)                    # the qualities as a device tensor


def test_many_workgroups_and_clamped_qualities():
    """Four 72 x 136 images (153 Y blocks and 90 chroma blocks each: eight workgroups per sample, the last one partly filled) with
    qualities outside 1 .. 100, and inputs that are not exact 8-bit levels."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4, 3, 72, 136, generator=g) * 1.2 - 0.1                      # also below 0 and above 1: clamped by the loader
    q = [-3, 30, 100, 250]
    got = T.jpeg_roundtrip(x.to(DEV), q).cpu()
    assert torch.equal(got, T._torch_jpeg(x, torch.tensor(q, dtype=torch.int32)))
    assert torch.equal(got, T.jpeg_roundtrip(x.to(DEV), [1, 30, 100, 100]).cpu())
    gray = T.jpeg_roundtrip(x[:, :1].contiguous().to(DEV), q).cpu()
    assert torch.equal(gray, T._torch_jpeg(x[:, :1].contiguous(), torch.tensor(q, dtype=torch.int32)))


def test_bad_arguments_raise_without_a_fault():
    x = torch.rand(2, 3, 20, 20, device=DEV)
    q = torch.tensor([10, 20], dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError):
        T.hip_jpeg(x.half(), q)
    with pytest.raises(TypeError):
        T.hip_jpeg(x, q.long())
    with pytest.raises(ValueError):
        T.hip_jpeg(x, q[:1])
    with pytest.raises(ValueError):
        T.hip_jpeg(x, q.cpu())
    L = _lib.lib()
    assert L.grl_jpeg_workspace_bytes(2, 3, 20, 20) == 2 * (9 * 64 + 2 * 4 * 64)
    assert L.grl_jpeg_workspace_bytes(1, 1, 1, 1) == 64
    for bad in ((0, 3, 8, 8), (1, 2, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1)):
        assert L.grl_jpeg_workspace_bytes(*bad) == -1, bad
    out = torch.empty_like(x)
    ws = torch.empty(int(L.grl_jpeg_workspace_bytes(2, 3, 20, 20)) + 8, dtype=torch.uint8, device=DEV)
    good = dict(x=x.data_ptr(), quality=q.data_ptr(), N=2, C=3, H=20, W=20, workspace=ws.data_ptr(), out=out.data_ptr())
    call = lambda **kw: L.grl_jpeg_roundtrip(_lib.stream_ptr(), C.byref(_lib.GrlJpegArgs(**dict(good, **kw))))
    assert call() == 0
    for kw in (dict(x=None), dict(quality=None), dict(workspace=None), dict(out=None), dict(N=0), dict(C=2), dict(C=4), dict(H=0),
               dict(W=-1), dict(out=out.data_ptr() + 2), dict(workspace=ws.data_ptr() + 4)):
        assert call(**kw) == -1, kw
    assert call(N=1 << 30, H=1 << 10, W=1 << 10) == -1                          # beyond 2^31 - 1 workgroups
    assert L.grl_jpeg_roundtrip(_lib.stream_ptr(), None) == -1
    torch.cuda.synchronize()
    assert torch.equal(out, T.jpeg_roundtrip(x, q))


def test_replay_from_a_graph_follows_the_quality_tensor():
    _, x, quality, _ = jpeg_case("37x53_c3_a")
    xd = x.to(DEV)
    q = torch.tensor(quality, dtype=torch.int32, device=DEV)
    first = T.hip_jpeg(xd, q)                                                  # loads the library outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = T.hip_jpeg(xd, q)
    new = [90, 5, 33]
    q.copy_(torch.tensor(new, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    eager = T.jpeg_roundtrip(xd, new)
    assert torch.equal(out, eager) and not torch.equal(out, first)
    assert torch.equal(out.cpu(), T._torch_jpeg(x, torch.tensor(new, dtype=torch.int32)))


def test_jpeg_sampler_on_a_cuda_store():
    """Both modes against the CPU store's batches for one work list, bitwise."""
    imgs = store_images()
    P, B = 16, len(WORK)
    cpu = PatchSampler("jpeg", PatchStore(imgs), patch=P, batch=B, quality=10)
    gpu = PatchSampler("jpeg", PatchStore(imgs, DEV), patch=P, batch=B, quality=10)
    for n in range(2):
        assert torch.equal(gpu.lq_store.image(n).cpu(), cpu.lq_store.image(n))
    (lq, gt), (want_lq, want_gt) = gpu.next(WORK), cpu.next(WORK)
    assert lq.is_cuda and torch.equal(lq.cpu(), want_lq) and torch.equal(gt.cpu(), want_gt)
    quals = [10, 25, 40, 33, 17]
    cpu = PatchSampler("jpeg", PatchStore(imgs), patch=P, batch=B, quality_range=(10, 40), seed=3)
    gpu = PatchSampler("jpeg", PatchStore(imgs, DEV), patch=P, batch=B, quality_range=(10, 40), seed=3)
    (lq, gt), (want_lq, want_gt) = gpu.next(WORK, quals), cpu.next(WORK, quals)
    assert lq.is_cuda and gpu.qualities.is_cuda and gpu.qualities.tolist() == quals
    assert torch.equal(lq.cpu(), want_lq) and torch.equal(gt.cpu(), want_gt)
    for _ in range(2):                                                         # fresh draws: the same stream on both
        (lq, gt), (want_lq, want_gt) = gpu.next(), cpu.next()
        assert torch.equal(lq.cpu(), want_lq) and torch.equal(gt.cpu(), want_gt)


def _folder(tmp_path):
    from PIL import Image

    rng = np.random.RandomState(8)
    d = tmp_path / "live1"
    d.mkdir()
    imgs = [pattern("noise", 37, 53, 3, rng) // 4 + pattern("ramp", 37, 53, 3, rng) // 2, pattern("ramp", 40, 48, 3, rng)]
    for n, im in enumerate(imgs):
        Image.fromarray(im).save(d / f"im{n}.png")
    return d, imgs


def test_evaluate_folder_jpeg(tmp_path, capsys):
    d, imgs = _folder(tmp_path)
    model = GRL(**make_config("tiny", "dm", depths=[1], num_heads_window=[2], num_heads_stripe=[2])).eval()
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    gts = [torch.from_numpy(im).permute(2, 0, 1)[None].float().div(255) for im in imgs]
    pairs = [(T.jpeg_roundtrip(gt.to(DEV), 10), gt) for gt in gts]
    with torch.no_grad():
        want = EV.evaluate_pairs(model, pairs, 1, device=DEV)
        got = EV.evaluate_folder(model, None, str(d), 1, device=DEV, task="jpeg", quality=10)
        grp = EV.evaluate_folder(model, None, str(d), 1, device=DEV, task="jpeg", quality=10, metric_group="restorer_jpeg",
                                 verbose=False)
    assert "im0.png" in capsys.readouterr().out
    assert got == sum(want) / 2
    assert set(grp) >= {"val_psnrb", "val_psnrb_y"} and all(np.isfinite(v) for v in grp.values())
    for (_, lq, gt), (want_lq, want_gt) in zip(EV.task_inputs(str(d), "jpeg", quality=10, device=DEV), pairs):
        assert lq.is_cuda and torch.equal(lq, want_lq) and torch.equal(gt, want_gt)


def test_train_cli_jpeg_eager_and_captured(tmp_path, capsys):
    """``--quality-range 10 40`` for three steps, eager and through the captured step: the same draws, finite losses, and the same
    loss at the first step (which both runs take eagerly from the same weights and the same batch)."""
    d, _ = _folder(tmp_path)
    args = ["--task", "jpeg", "--quality-range", "10", "40", "--model", "tiny", "--geometry", "yaml", "--depths", "1+1", "--patch", "16",
            "--batch", "2", "--gt", str(d), "--lr", "2e-4", "--steps", "3"]
    torch.manual_seed(0)
    r = train.main(args + ["--eager", "--out", str(tmp_path / "eager")])
    torch.manual_seed(0)
    c = train.main(args + ["--out", str(tmp_path / "graph")])
    capsys.readouterr()
    print("eager", r["losses"], "captured", c["losses"])
    assert r["steps"] == c["steps"] == [0, 1, 2] and r["work"] == c["work"]
    assert all(np.isfinite(r["losses"])) and all(np.isfinite(c["losses"]))
    assert c["losses"][0] == r["losses"][0]
    obj = torch.load(c["checkpoint"], map_location="cpu", weights_only=False)
    assert obj["step"] == 3 and obj["args"]["task"] == "jpeg" and obj["args"]["quality_range"] == [10, 40]
    assert all(bool(torch.isfinite(v).all()) for v in obj["state_dict"].values())


def test_jpeg_geometry_preset_matches_the_oracle():
    """presets.GEOMETRIES["jpeg"] (window 36, stripes 72 x 144, anchors / 4; jpeg/grl/grl_p288.yaml) on a depth-1 tiny-width model
    and a 144 x 144 input against the pinned CPU oracle, at the bar of tests/test_gpu_model.py."""
    cfg = make_config("tiny", "jpeg", upscale=1, img_size=144, depths=[1], num_heads_window=[2], num_heads_stripe=[2])
    assert cfg["window_size"] == 36 and cfg["stripe_size"] == [72, 144] and cfg["anchor_window_down_factor"] == 4
    m = GRL(**cfg).eval()
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, 0)
    m.load_state_dict(sd, strict=True)
    lq, _ = O.synthetic_pair("dn", (144, 144), 1, batch=1, seed=1)
    with torch.no_grad():
        want = O.grl_forward(lq, cfg, sd)
        got = m.to(DEV)(lq.to(DEV)).float().cpu()
    err = (got - want).abs().max().item()
    print(f"tiny jpeg geometry 144x144: max|hip - oracle| = {err:.3e}")
    assert got.shape == want.shape and err < 1e-3, err
