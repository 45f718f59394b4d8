"""GPU tests of grl_sample_patches (csrc/patches.hip) and of the training command fed by it: bitwise equality with the CPU path and
the reference chain on the stores, work list and shapes of tests/test_patches.py, ragged tiles, bad arguments, replay from a
captured graph with a changing work list, and the train CLI end to end (eager and captured)."""
import ctypes as C

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import PatchSampler, PatchStore, _lib
from test_patches import B, P, reference_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("scale,patch", [(1, P), (2, P), (1, 33)])      # S = 24, 48 (two tiles a side, ragged) and 33 (scalar stores)
def test_kernel_equals_cpu_path_and_reference(channels, scale, patch):
    lq_imgs, gt_imgs, work, want_lq, want_gt = reference_case(channels, scale, patch)
    cpu = PatchSampler("sr", PatchStore(gt_imgs), PatchStore(lq_imgs), patch=patch, batch=B, scale=scale)
    gpu = PatchSampler("sr", PatchStore(gt_imgs, "cuda:0"), PatchStore(lq_imgs).to("cuda:0"), patch=patch, batch=B, scale=scale)
    lq_c, gt_c = cpu.next(work)
    lq_g, gt_g = gpu.next(work)
    assert lq_g.is_cuda and gt_g.shape == (B, channels, patch * scale, patch * scale)
    assert torch.equal(lq_g.cpu(), lq_c) and torch.equal(gt_g.cpu(), gt_c)
    assert torch.equal(lq_g.cpu(), want_lq) and torch.equal(gt_g.cpu(), want_gt)


def test_bad_arguments_are_rejected_without_a_launch():
    L = _lib.lib()
    st = PatchStore([np.zeros((8, 8, 3), dtype=np.uint8)], "cuda:0")
    work = torch.zeros(1, 4, dtype=torch.int32, device="cuda:0")
    out = torch.full((1, 3, 4, 4), 7.0, device="cuda:0")
    good = dict(store=st.data.data_ptr(), offsets=st.offsets.data_ptr(), dims=st.dims_t.data_ptr(), N=1, C=3, work=work.data_ptr(),
                B=1, P=4, scale=1, out=out.data_ptr())
    call = lambda **kw: L.grl_sample_patches(_lib.stream_ptr(), C.byref(_lib.GrlPatchArgs(**dict(good, **kw))))
    for kw in (dict(C=2), dict(P=0), dict(scale=0), dict(B=0), dict(N=0), dict(store=None), dict(offsets=None), dict(dims=None),
               dict(work=None), dict(out=None), dict(out=out.data_ptr() + 4)):
        assert call(**kw) == -1, kw
    assert L.grl_sample_patches(_lib.stream_ptr(), None) == -1
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0                       # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0
    with pytest.raises(ValueError):
        st.sample(work.cpu(), 4)


def test_replay_from_a_graph_follows_the_work_list():
    _, gt_imgs, work, _, _ = reference_case(3, 2)
    st = PatchStore(gt_imgs, "cuda:0")
    lists = [torch.tensor(w, dtype=torch.int32) for w in (work, work[::-1], work[3:] + work[:3])]
    want = [st.sample(w.cuda(), P, 2).clone() for w in lists]
    wl = lists[0].cuda()
    out = torch.zeros(B, 3, 2 * P, 2 * P, device="cuda:0")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                            # the sampler launch alone: a straight line
        st.sample(wl, P, 2, out=out)
    for i in (1, 2):
        wl.copy_(lists[i])                               # in place: the captured launch reads this address
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[i]), i
    assert not torch.equal(want[1], want[2])


def test_train_cli_end_to_end(tmp_path, capsys):
    from PIL import Image

    from grl_image_restoration_amd import GRL, make_config, train
    from grl_image_restoration_amd.evaluate import evaluate_folder, load_checkpoint

    gt = tmp_path / "gt"
    gt.mkdir()
    g = np.random.RandomState(1)
    for i in range(4):
        smooth = np.kron(g.randint(0, 256, (12, 12, 3)), np.ones((8, 8, 1))).astype(np.uint8)
        Image.fromarray(smooth).save(gt / f"im{i}.png")
    args = ["--task", "sr_bicubic", "--scale", "2", "--model", "tiny", "--geometry", "sr_ckpt_df4", "--depths", "2", "--patch", "32",
            "--batch", "2", "--gt", str(gt), "--lr", "2e-4", "--warmup-iter", "2", "--warmup-init-lr", "1e-5", "--milestones", "3"]
    torch.manual_seed(0)
    r = train.main(args + ["--steps", "4", "--eager", "--out", str(tmp_path / "eager")])
    assert r["steps"] == [0, 1, 2, 3] and all(np.isfinite(r["losses"]))
    model = GRL(**make_config("tiny", "sr_ckpt_df4", upscale=2, img_size=32, depths=[2], num_heads_window=[2], num_heads_stripe=[2]))
    res = load_checkpoint(model, r["checkpoint"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    psnr = evaluate_folder(model.cuda().eval(), None, str(gt), 2, verbose=False, task="sr_bicubic")
    assert np.isfinite(psnr)

    torch.manual_seed(0)
    c = train.main(args + ["--steps", "3", "--out", str(tmp_path / "graph")])          # the captured step fed by the sampler
    assert c["steps"] == [0, 1, 2] and all(np.isfinite(c["losses"]))
    assert c["work"] == r["work"][:3] and c["lrs"] == r["lrs"][:3]
    assert c["losses"][0] == pytest.approx(r["losses"][0], rel=1e-3)                   # step 0 is the same eager step
    obj = torch.load(c["checkpoint"], map_location="cpu", weights_only=False)
    assert obj["step"] == 3 and {int(s["step"]) for s in obj["optimizer"]["state"].values()} == {3}
    assert all(bool(torch.isfinite(v).all()) for v in obj["state_dict"].values())
    capsys.readouterr()
