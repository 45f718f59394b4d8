"""GPU tests of dual-pixel defocus deblurring: grl_sample_patch_views (csrc/patches.hip) bit for bit against three
``PatchStore.sample`` launches plus ``torch.cat`` and against the CPU restatement, its argument errors and its replay from a captured
graph; and ``GRL(in_channels=6, out_channels=3)`` on the HIP path -- inference in every precision mode, tiled evaluation, the training
graph's gradients and the captured step fed by the new sampler -- against the real reference (tests/golden/tasks/dual_pixel.npz)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, PatchSampler, PatchStore, _lib
from grl_image_restoration_amd.data import sample_views
from test_dual_pixel import fixture, fixture_gradients, fixture_input, fixture_model, make_views, reference_batch, step_batch, work_list
from test_patches import B as PB, P as PP, reference_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_MAXABS = 1e-3       # the project's bar on the network output (tests/test_gpu_model.py), every mode


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
_STORES = {}


def stores(device):
    if device not in _STORES:
        _STORES[device] = tuple(PatchStore(v, device) for v in make_views())
    return _STORES[device]


# patches: scalar stores; a tile smaller than T; one tile; a ragged second tile; 3 x 3 tiles.  Batch 10 carries all eight flag values;
# batches 1 and 3 run at the ragged and at the largest shape
@pytest.mark.parametrize("patch,batch", [(p, 10) for p in (5, 31, 32, 33, 96)] + [(33, 1), (33, 3), (96, 1), (96, 3)])
def test_views_equal_three_launches_and_the_cpu_path(patch, batch):
    """The dual-pixel batch: left -> lq[:, 0:3], right -> lq[:, 3:6], gt -> gt, all eight flag values (batch 10), images smaller than
    the patch in either direction (SIZES: 20 rows, 20 columns)."""
    left, right, gt, work, want_lq, want_gt = reference_batch(patch, batch)
    L_, R, G = stores(DEV)
    wl = torch.tensor(work, dtype=torch.int32, device=DEV)
    lq = torch.full((batch, 6, patch, patch), 7.0, device=DEV)
    g = torch.full((batch, 3, patch, patch), 7.0, device=DEV)
    outs = sample_views([(L_, 1, lq, 0), (R, 1, lq, 3), (G, 1, g, 0)], wl, patch)
    assert outs[0] is lq and outs[2] is g
    three = torch.cat([L_.sample(wl, patch, 1), R.sample(wl, patch, 1)], dim=1)
    assert torch.equal(lq, three) and torch.equal(g, G.sample(wl, patch, 1))
    assert torch.equal(lq.cpu(), want_lq) and torch.equal(g.cpu(), want_gt)           # the reference's item by hand
    cl, cr, cg = stores("cpu")
    cpu = PatchSampler("sr", cg, cl, patch=patch, batch=batch, lq_r_store=cr)
    gpu = PatchSampler("sr", G, L_, patch=patch, batch=batch, lq_r_store=R)
    lq_c, gt_c = cpu.next(work)
    lq_g, gt_g = gpu.next(work)
    assert lq_g.is_cuda and lq_g.shape == (batch, 6, patch, patch)
    assert torch.equal(lq_g.cpu(), lq_c) and torch.equal(gt_g.cpu(), gt_c) and torch.equal(lq_g, lq)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("patch", [PP, 33])
def test_two_views_at_scales_1_and_2(channels, patch):
    """The paired sr shape in one launch -- the views differ in S, so one takes the float4 store and the other may not -- on the
    stores, work list and reference chain of tests/test_patches.py."""
    lq_imgs, gt_imgs, work, want_lq, want_gt = reference_case(channels, 2, patch)
    lq_s, gt_s = PatchStore(lq_imgs, DEV), PatchStore(gt_imgs, DEV)
    wl = torch.tensor(work, dtype=torch.int32, device=DEV)
    lq = torch.empty(PB, channels, patch, patch, device=DEV)
    gt = torch.empty(PB, channels, 2 * patch, 2 * patch, device=DEV)
    sample_views([(lq_s, 1, lq, 0), (gt_s, 2, gt, 0)], wl, patch)
    assert torch.equal(lq.cpu(), want_lq) and torch.equal(gt.cpu(), want_gt)
    assert torch.equal(lq, lq_s.sample(wl, patch, 1)) and torch.equal(gt, gt_s.sample(wl, patch, 2))


def test_channel_windows_four_views_and_an_index_outside_the_store():
    L_, R, G = stores(DEV)
    gray = PatchStore([im[:, :, 1] for im in make_views()[0]], DEV)
    patch = 33
    work = work_list(patch, 3) + [(3, 0, 0, 0), (-1, 2, 2, 5)]                          # the last two name no image of a store of 3
    wl = torch.tensor(work, dtype=torch.int32, device=DEV)
    n = len(work)
    # one view into channels 3 .. 5 of 6: the others keep what they held
    six = torch.full((n, 6, patch, patch), 7.0, device=DEV)
    sample_views([(R, 1, six, 3)], wl, patch)
    ok = torch.tensor(work[:3], dtype=torch.int32, device=DEV)
    assert float(six[:, :3].min()) == 7.0 and torch.equal(six[:3, 3:], R.sample(ok, patch, 1))
    assert float(six[3:, 3:].abs().max()) == 0.0                                       # outside the store: zeros, in that view's window
    # four views, C = 3 and C = 1 mixed, two outputs shared
    six.fill_(7.0)
    two = torch.full((n, 2, patch, patch), 7.0, device=DEV)
    sample_views([(L_, 1, six, 0), (R, 1, six, 3), (gray, 1, two, 1), (gray, 1, two, 0)], wl, patch)
    assert torch.equal(six[:3], torch.cat([L_.sample(ok, patch, 1), R.sample(ok, patch, 1)], dim=1))
    assert torch.equal(two[:3, :1], gray.sample(ok, patch, 1)) and torch.equal(two[:, 0], two[:, 1])
    assert float(six[3:].abs().max()) == 0.0 and float(two[3:].abs().max()) == 0.0
    cpu_gray = PatchStore([im[:, :, 1] for im in make_views()[0]])
    assert torch.equal(two[:3, :1].cpu(), cpu_gray.sample(ok.cpu(), patch, 1))
    with pytest.raises(ValueError):
        sample_views([(L_, 1, six, 4)], wl, patch)                                     # channels 4 .. 6 of 6
    with pytest.raises(ValueError):
        sample_views([(L_, 1, six, 0)] * 5, wl, patch)
    with pytest.raises(ValueError):
        sample_views([(L_, 1, six, 0)], wl.cpu(), patch)


def test_bad_arguments_are_rejected_without_a_launch():
    L = _lib.lib()
    st = PatchStore([np.zeros((8, 8, 3), dtype=np.uint8)], DEV)
    work = torch.zeros(1, 4, dtype=torch.int32, device=DEV)
    out = torch.full((1, 6, 4, 4), 7.0, device=DEV)
    view = dict(store=st.data.data_ptr(), offsets=st.offsets.data_ptr(), dims=st.dims_t.data_ptr(), N=1, C=3, scale=1, Ctot=6, c0=0,
                out=out.data_ptr())
    shared = dict(work=work.data_ptr(), B=1, P=4, V=2)

    def call(view_kw=None, which=1, **kw):
        args = _lib.GrlPatchViewsArgs(**dict(shared, **kw))
        args.view[0] = _lib.GrlPatchView(**dict(view, c0=3))
        args.view[1] = _lib.GrlPatchView(**view)
        args.view[which] = _lib.GrlPatchView(**dict(view, **(view_kw or {})))
        return L.grl_sample_patch_views(_lib.stream_ptr(), C.byref(args))

    for kw in (dict(C=2), dict(scale=0), dict(N=0), dict(store=None), dict(offsets=None), dict(dims=None), dict(out=None),
               dict(out=out.data_ptr() + 4), dict(c0=-1), dict(c0=4), dict(Ctot=2), dict(C=1, c0=6)):
        assert call(kw) == -1, kw
        assert call(kw, which=0) == -1, kw
    for kw in (dict(P=0), dict(B=0), dict(V=0), dict(V=5), dict(V=-1), dict(work=None), dict(work=work.data_ptr() + 4)):
        assert call(**kw) == -1, kw
    assert L.grl_sample_patch_views(_lib.stream_ptr(), None) == -1
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0                       # nothing was launched
    assert call(dict(C=2), V=1) == 0                     # view[V ..] is ignored: only view 0 (channels 3 .. 5) runs
    torch.cuda.synchronize()
    assert float(out[:, 3:].abs().max()) == 0.0 and float(out[:, :3].min()) == 7.0
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0


def test_replay_from_a_graph_follows_the_work_list():
    L_, R, G = stores(DEV)
    patch = 33
    work = work_list(patch, 10)
    lists = [torch.tensor(w, dtype=torch.int32) for w in (work, work[::-1], work[3:] + work[:3])]
    want = []
    for w in lists:
        wd = w.to(DEV)
        want.append((torch.cat([L_.sample(wd, patch, 1), R.sample(wd, patch, 1)], dim=1), G.sample(wd, patch, 1)))
    wl = lists[0].to(DEV)
    lq, gt = torch.zeros(10, 6, patch, patch, device=DEV), torch.zeros(10, 3, patch, patch, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                            # the one launch alone: a straight line
        sample_views([(L_, 1, lq, 0), (R, 1, lq, 3), (G, 1, gt, 0)], wl, patch)
    for i in (1, 2):
        wl.copy_(lists[i])                               # in place: the captured launch reads this address
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(lq, want[i][0]) and torch.equal(gt, want[i][1]), i
    assert not torch.equal(want[1][0], want[2][0])


# ---- the 6-in / 3-out network ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["96x96", "100x90"])
@pytest.mark.parametrize("precision", ["fast", "high", "auto"])
def test_inference_matches_the_reference(precision, tag):
    meta, z = fixture()
    m = fixture_model(meta)
    m2 = GRL(**meta["cfg"], precision=precision).eval()
    m2.load_state_dict(m.state_dict(), strict=True)
    m2 = m2.to(DEV)
    x = fixture_input(z, tag).to(DEV)
    with torch.no_grad():
        y = m2(x)
        m2.enable_graph()
        yg = m2(x)                                       # graph mode: the same launches, captured
    want = torch.from_numpy(z["output64_" + tag])
    assert y.shape == want.shape and y.shape[1] == 3
    err = (y.double().cpu() - want).abs().max().item()
    print(f"dual-pixel {tag} [{precision} -> {m2.precision}]: max|hip - reference fp64| = {err:.3e}")
    assert err < TOL_MAXABS, err
    assert torch.equal(y, yg)


def test_auto_calibration_probe_runs_at_six_channels():
    """``plan.calibrated_plan`` with its probe forced (a Tiny-width model resolves `auto` without it): the probe image has the model's
    6 input channels, the plan it returns holds the bar on the fixture."""
    from grl_image_restoration_amd import plan as P

    meta, z = fixture()
    m = GRL(**meta["cfg"], precision="fast").eval()
    m.load_state_dict(fixture_model(meta).state_dict(), strict=True)
    m = m.to(DEV)
    assert P.probe_input(m, 96, 96, DEV).shape == (1, 6, 96, 96)
    with torch.no_grad():
        plan = P.calibrated_plan(m, (96, 96), torch.device(DEV), force=True)
        y = m._forward_eager(fixture_input(z, "96x96").to(DEV), plan)
    cal = m.calibration
    assert cal is not None and cal["blocks"] == 4 and "bar_max" in cal
    err = (y.double().cpu() - torch.from_numpy(z["output64_96x96"])).abs().max().item()
    print(f"dual-pixel forced calibration: {cal}; max|hip - reference fp64| = {err:.3e}")
    assert err < TOL_MAXABS, err


def test_tiled_evaluation_on_the_ragged_input():
    """The 100 x 90 input with tile 96, the path the released checkpoint is evaluated on: a 3-channel canvas for a 6-channel input.
    ``evaluate_pairs`` tiles an image only when the tile is smaller than its smaller side, so at tile 96 it runs this image whole;
    ``forward_tiled`` itself clamps the tile to 90 and stitches two tiles; ``evaluate_pairs`` at tile 80 stitches four.  The stitched
    outputs equal the reference's E / W loop (engines/base.py:100-116) over this model's own per-tile outputs bit for bit: the
    tiles run as one batch there and one by one here, and no kernel of the inference path depends on the batch or uses atomics."""
    from grl_image_restoration_amd import tiling
    from grl_image_restoration_amd.evaluate import evaluate_pairs, psnr_y

    meta, z = fixture()
    m = fixture_model(meta).to(DEV)
    x = fixture_input(z, "100x90")
    want = torch.from_numpy(z["output64_100x90"])
    gt = want.float().clamp(0, 1)

    def stitched(tile, rows, cols):
        E, W = torch.zeros(1, 3, 100, 90, device=DEV), torch.zeros(1, 3, 100, 90, device=DEV)
        with torch.no_grad():
            for hi in rows:
                for wi in cols:
                    E[..., hi : hi + tile, wi : wi + tile] += m(x[..., hi : hi + tile, wi : wi + tile].to(DEV))
                    W[..., hi : hi + tile, wi : wi + tile] += 1
        return E / W

    got = {}
    keep = lambda i, lq, sr, g: got.update(sr=sr.clone(), lq=lq)
    vals = evaluate_pairs(m, [(x, gt)], 1, tile=96, overlap=16, device=DEV, on_result=keep)
    assert got["lq"].shape == (1, 6, 100, 90) and got["sr"].shape == (1, 3, 100, 90) and np.isfinite(vals[0])
    assert (got["sr"].double().cpu() - want).abs().max().item() < TOL_MAXABS
    with torch.no_grad():
        direct = tiling.forward_tiled(m, x.to(DEV), 96, 16, 1, out_channels=m.out_channels)
    assert direct.shape == (1, 3, 100, 90)
    e2 = (direct - stitched(90, (0, 10), (0,))).abs().max().item()
    vals = evaluate_pairs(m, [(x, gt)], 1, tile=80, overlap=16, device=DEV, on_result=keep)
    ref4 = stitched(80, (0, 20), (0, 10))
    e4 = (got["sr"] - ref4).abs().max().item()
    print(f"dual-pixel tiled 100x90: two tiles of 90 max|d| = {e2:.3e}, four tiles of 80 max|d| = {e4:.3e}")
    assert got["sr"].shape == (1, 3, 100, 90) and e2 == 0.0 and e4 == 0.0
    assert vals[0] == pytest.approx(float(psnr_y(ref4, gt.to(DEV))), abs=0.01)


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm().clamp_min(1e-30)).item()


def test_training_step_gradients_match_the_reference():
    """One L1 step (eval mode, as the fixture) on the training graph: the loss and every parameter gradient against the real reference,
    at the bars of tests/test_gpu_train_step.py -- 2e-4 on the loss, 1e-2 relative on a gradient's norm, 2e-2 norm-wise on the
    gradients compared element by element (the whole small ones; here also the fixed samples of the large ones)."""
    meta, z = fixture()
    m = fixture_model(meta).to(DEV)
    lq, gt = step_batch(meta)
    loss = (m(lq.to(DEV)) - gt.to(DEV)).abs().mean()
    loss.backward()
    assert abs(loss.item() - meta["loss"]) < 2e-4, (loss.item(), meta["loss"])
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    worst = ("", 0.0)
    for k, (a, b) in fixture_gradients(z, meta, grads).items():
        e = _rel(a, b)
        worst = max(worst, (k, e), key=lambda t: t[1])
        print(f"  {k}: {e:.2e}")
        assert e < 2e-2, (k, e)
        if "norm::" + k in z.files:
            n = float(z["norm::" + k])
            assert abs(grads[k].norm().item() - n) / max(n, 1e-12) < 1e-2, k
    print(f"dual-pixel training step: loss {loss.item():.6f} (reference {meta['loss']:.6f}); worst gradient error {worst}")


def test_graphed_train_step_on_batches_of_the_new_sampler(tmp_path):
    """Three replays of ``GraphedTrainStep`` on (2, 6, 96, 96) batches cut by grl_sample_patch_views: finite losses, the optimizer's
    step count on the host, and -- one batch repeated, as tests/test_gpu_train_graph.py's captured-step test repeats its batch -- a
    loss that does not rise."""
    from grl_image_restoration_amd import FusedAdamW, GraphedTrainStep

    meta, z = fixture()
    m = GRL(**dict(meta["cfg"], drop_path_rate=0.0))
    m.load_state_dict(fixture_model(meta).state_dict(), strict=True)
    m = m.to(DEV).train()
    g = np.random.RandomState(9)
    imgs = [np.kron(g.randint(0, 256, (16, 18, 3)), np.ones((8, 8, 1))).astype(np.uint8) for _ in range(9)]      # 128 x 144
    sampler = PatchSampler("sr", PatchStore(imgs[:3], DEV), PatchStore(imgs[3:6], DEV), patch=96, batch=2, seed=3,
                           lq_r_store=PatchStore(imgs[6:], DEV))
    opt = FusedAdamW(m.parameters(), lr=2e-4, weight_decay=1e-4)
    loss_fn = lambda y, t: (y - t).abs().mean()
    lq, gt = sampler.next()
    assert lq.shape == (2, 6, 96, 96) and gt.shape == (2, 3, 96, 96) and lq.is_cuda
    step = GraphedTrainStep(m, opt, loss_fn, lq, gt, warmup=1)
    same = [float(step(lq, gt).detach()) for _ in range(3)]
    fresh = []
    for _ in range(2):
        lq2, gt2 = sampler.next()
        fresh.append(float(step(lq2, gt2).detach()))
    step.finish()
    print(f"captured dual-pixel step: repeated batch {same}, fresh batches {fresh}")
    assert all(np.isfinite(same + fresh)) and same[-1] <= same[0]
    assert opt.state[next(iter(m.parameters()))]["step"] == 1 + 3 + 2
    with torch.no_grad():
        y = m.eval()(lq)
    assert y.shape == (2, 3, 96, 96) and bool(torch.isfinite(y).all())


def test_command_lines_end_to_end(tmp_path, capsys):
    """train --lq-r (the captured step fed by the one-launch sampler), then evaluate --lq-r on its checkpoint, tiled, with
    --save-dir, and restore --lq-r: the commands a user of the dual-pixel checkpoint runs, on three small folders."""
    from PIL import Image

    from grl_image_restoration_amd import evaluate, restore, train

    g = np.random.RandomState(4)
    for name in ("left", "right", "target"):
        (tmp_path / name).mkdir()
        for i, (h, w) in enumerate([(120, 112), (96, 100)]):
            smooth = np.kron(g.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)), np.ones((8, 8, 1)))[:h, :w].astype(np.uint8)
            Image.fromarray(smooth).save(tmp_path / name / f"im{i}.png")
    L_, R, G = (str(tmp_path / n) for n in ("left", "right", "target"))
    model = ["--task", "sr", "--scale", "1", "--model", "tiny", "--geometry", "defocus"]
    torch.manual_seed(0)
    r = train.main(model + ["--gt", G, "--lq", L_, "--lq-r", R, "--patch", "96", "--batch", "2", "--steps", "3", "--lr", "2e-4",
                            "--out", str(tmp_path / "run")])
    assert r["steps"] == [0, 1, 2] and all(np.isfinite(r["losses"]))
    obj = torch.load(r["checkpoint"], map_location="cpu", weights_only=False)
    assert obj["state_dict"]["model.conv_first.weight"].shape[1] == 6 and obj["state_dict"]["model.conv_last.weight"].shape[0] == 3
    assert all(bool(torch.isfinite(v).all()) for v in obj["state_dict"].values())
    v = evaluate.main(model + ["--lq", L_, "--lq-r", R, "--gt", G, "--tile", "96", "--overlap", "16", "--ckpt", r["checkpoint"],
                               "--metric", "restorer", "--save-dir", str(tmp_path / "results")])
    assert all(np.isfinite(x) for x in v.values())
    saved = tmp_path / "results" / "target"                     # straight under the data set's name: no X1 level
    assert sorted(os.listdir(saved)) == ["im0_HQ.png", "im0_LQ.png", "im1_HQ.png", "im1_LQ.png"]
    for i in (0, 1):
        left = np.asarray(Image.open(os.path.join(L_, f"im{i}.png")).convert("RGB"))
        assert np.asarray(Image.open(saved / f"im{i}_LQ.png")).tobytes() == left.tobytes()
        assert np.asarray(Image.open(saved / f"im{i}_HQ.png")).shape == left.shape
    paths = restore.main(["--model", "tiny", "--geometry", "defocus", "--ckpt", r["checkpoint"], "--lq", L_, "--lq-r", R,
                          "--out", str(tmp_path / "restored"), "--tile", "96", "--overlap", "16"])
    assert [os.path.basename(p) for p in paths] == ["im0_HQ.png", "im1_HQ.png"]
    assert np.asarray(Image.open(paths[0])).tobytes() == np.asarray(Image.open(saved / "im0_HQ.png")).tobytes()
    capsys.readouterr()
