"""Dual-pixel defocus deblurring on the CPU: the sampler's right store against a by-hand numpy restatement of the reference's item
(data/datasets/restoration_paired_dataset.py:144-162 over base_image.py:276-293, 356-372, 397-402), the draw stream, the refusals, the
ABI entry, the parsers, the preset, the 6-in / 3-out network against the real reference (tests/golden/tasks/dual_pixel.npz, written by
tools/make_golden_dual_pixel.py), the folder runs whole and tiled, and the train command line.  The GPU side is
tests/test_gpu_dual_pixel.py, which shares the helpers below."""
import json
import os
import random
import re
import warnings
import zlib

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, PatchSampler, PatchStore, _lib, make_config, presets, task_rules
from oracle import grl_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(40, 52), (20, 64), (33, 20)]      # the second is shorter, the third narrower than the patch
P, B = 24, 10


# ---- three small stores and the reference's steps by hand ------------------------------------------------------------------------
def make_views(seed=5):
    """(left, right, gt) lists of uint8 H x W x 3 images of SIZES; the three views of an image differ everywhere."""
    g = np.random.RandomState(seed)
    return tuple([g.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES] for _ in range(3))


def work_list(patch=P, batch=B):
    w = []
    for b in range(batch):
        n = b % 3
        H, W = max(SIZES[n][0], patch), max(SIZES[n][1], patch)
        w.append((n, [0, H - patch, (H - patch) // 2][b % 3], [W - patch, 0, (W - patch) // 3][(b // 3) % 3], b % 8))
    return w


def reference_item(left, right, gt, x, y, flags, patch):
    """One item of the reference's dual-pixel data set at a given position and flips: (lq (6, P, P), gt (3, P, P))."""
    imgs = [left, right, gt]
    h, w = imgs[0].shape[:2]
    if h < patch or w < patch:                                                       # _pad_images: zeros at the bottom / right
        imgs = [np.pad(i, ((0, max(0, patch - h)), (0, max(0, patch - w)), (0, 0)), "constant", constant_values=0) for i in imgs]
    imgs = [i[x : x + patch, y : y + patch] for i in imgs]                            # _sample_patches: ONE position
    if flags & 1:                                                                    # _augment: ONE set of flips for the three
        imgs = [i[::-1] for i in imgs]
    if flags & 2:
        imgs = [i[:, ::-1] for i in imgs]
    if flags & 4:
        imgs = [np.swapaxes(i, 0, 1) for i in imgs]
    ts = [torch.from_numpy(np.ascontiguousarray(i)).permute(2, 0, 1).contiguous().to(torch.float32).div(255) for i in imgs]   # to_tensor
    return torch.cat([ts[0], ts[1]], dim=0), ts[2]                                   # engines/base.py:119-120: left first


_REF = {}


def reference_batch(patch=P, batch=B):
    """(left, right, gt images, work list, reference lq, reference gt): computed once per shape, shared with the GPU tests."""
    if (patch, batch) not in _REF:
        left, right, gt = make_views()
        work = work_list(patch, batch)
        items = [reference_item(left[n], right[n], gt[n], x, y, f, patch) for n, x, y, f in work]
        _REF[patch, batch] = (left, right, gt, work, torch.stack([i[0] for i in items]), torch.stack([i[1] for i in items]))
    return _REF[patch, batch]


def test_sampler_equals_the_reference_item():
    left, right, gt, work, want_lq, want_gt = reference_batch()
    assert {w[3] for w in work} == set(range(8))
    s = PatchSampler("sr", PatchStore(gt), PatchStore(left), patch=P, batch=B, scale=1, lq_r_store=PatchStore(right))
    lq, g = s.next(work)
    assert lq.shape == (B, 6, P, P) and g.shape == (B, 3, P, P) and lq.dtype == torch.float32
    assert torch.equal(lq, want_lq) and torch.equal(g, want_gt)
    assert not torch.equal(lq[:, :3], lq[:, 3:])
    assert float((lq[1] == 0).float().mean()) > 0.1 and float((g[1] == 0).float().mean()) > 0.1     # the 20-row image is padded with zeros


def test_same_seed_gives_the_same_work_list_with_and_without_the_right_store():
    left, right, gt = make_views()
    a = PatchSampler("sr", PatchStore(gt), PatchStore(left), patch=P, batch=B, seed=7)
    b = PatchSampler("sr", PatchStore(gt), PatchStore(left), patch=P, batch=B, seed=7, lq_r_store=PatchStore(right))
    for _ in range(3):
        assert a.draw() == b.draw()
    sa, sb = a.rng_state(), b.rng_state()
    assert sa["draws"] == sb["draws"] and set(sa) == set(sb) and sb["noise"] is None
    lq_a, gt_a = a.next()
    lq_b, gt_b = b.next()
    assert torch.equal(lq_a, lq_b[:, :3]) and torch.equal(gt_a, gt_b)
    # and the draws are the reference's: image, _random_index on the padded first LQ view, three flips
    random.seed(11)
    want = []
    for _ in range(B):
        n = random.randrange(3)
        H, W = max(SIZES[n][0], P), max(SIZES[n][1], P)
        x, y = random.randrange(0, H - P + 1), random.randrange(0, W - P + 1)
        want.append((n, x, y, sum(bit for bit in (1, 2, 4) if random.random() < 0.5)))
    c = PatchSampler("sr", PatchStore(gt), PatchStore(left), patch=P, batch=B, seed=0, lq_r_store=PatchStore(right))
    c.rng.seed(11)
    assert c.draw() == (want, None)


def test_sampler_refusals():
    left, right, gt = make_views()
    G, L_, R = PatchStore(gt), PatchStore(left), PatchStore(right)
    ok = dict(patch=P, batch=2, scale=1, lq_r_store=R)
    PatchSampler("sr", G, L_, **ok)
    for kw in (dict(usm=True), dict(usm=True, plain_gt=True), dict(plain_gt=True), dict(degrade=True), dict(jitter=True), dict(scale=2)):
        with pytest.raises(ValueError):
            PatchSampler("sr", G, L_, **dict(ok, **kw))
    with pytest.raises(ValueError):
        PatchSampler("sr", G, None, **ok)                                            # no left view
    with pytest.raises(ValueError):
        PatchSampler("dn", G, None, sigma=25, **ok)                                   # another task
    gray = PatchStore([im[:, :, 0] for im in right])
    with pytest.raises(ValueError):
        PatchSampler("sr", G, L_, **dict(ok, lq_r_store=gray))                        # channel count
    with pytest.raises(ValueError):
        PatchSampler("sr", G, L_, **dict(ok, lq_r_store=PatchStore(right[:2])))       # image count
    with pytest.raises(ValueError):
        PatchSampler("sr", G, L_, **dict(ok, lq_r_store=PatchStore([right[0], right[1], right[2][:-1]])))     # sizes
    with pytest.raises(ValueError):
        PatchSampler("sr", PatchStore([im[:, :, 0] for im in gt]), PatchStore([im[:, :, 0] for im in left]), **dict(ok, lq_r_store=gray))


def test_rule_keyword():
    assert tuple(task_rules.RULES) == ("sr", "dn", "dm", "sr_bicubic", "bsr", "db", "jpeg")      # an option of sr, not a task
    o = task_rules.resolve("sr", "train", scale=1, channels=3, lq=True, dual_pixel=True)
    assert o.scale == 1 and o.rule is task_rules.RULES["sr"]
    assert task_rules.resolve("sr", "train", scale=4, lq=True).scale == 4              # default off: nothing changes
    for kw in (dict(scale=2), dict(scale=None), dict(channels=1), dict(lq=False), dict(usm=True), dict(val_usm=True), dict(gan=True)):
        with pytest.raises(ValueError):
            task_rules.resolve("sr", "train", **dict(dict(scale=1, channels=3, lq=True, dual_pixel=True), **kw))
    with pytest.raises(ValueError):
        task_rules.resolve("sr", "train", scale=2, channels=3, lq=False, degrade=True, dual_pixel=True)
    for task in ("dn", "dm", "db", "jpeg", "sr_bicubic"):
        with pytest.raises(ValueError):
            task_rules.resolve(task, "evaluate", scale=1, sigma=25, quality=10, dual_pixel=True)


def test_abi_entry():
    """The struct layouts and the prototype are compared with the header by tests/test_abi.py, like every entry's."""
    assert "grl_sample_patch_views" in _lib.EXPORTS and _lib.ABI_VERSION >= 39
    assert _lib.SIGNATURES["grl_sample_patch_views"][1][1]._type_ is _lib.GrlPatchViewsArgs
    assert [f[0] for f in _lib.GrlPatchView._fields_] == ["store", "offsets", "dims", "N", "C", "scale", "Ctot", "c0", "reserved0", "out"]
    assert [f[0] for f in _lib.GrlPatchViewsArgs._fields_] == ["view", "work", "B", "P", "V", "reserved0"]
    assert _lib.GrlPatchViewsArgs.view.size == 4 * _lib.C.sizeof(_lib.GrlPatchView)
    header = open(os.path.join(ROOT, "include", "grl_hip.h")).read()
    assert "int grl_sample_patch_views(void* stream, const GrlPatchViewsArgs* args);" in header
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef struct GrlPatchView \{", header, re.S)
    for cite in ("restoration_paired_dataset.py:144-162", "base_image.py:276-293", "base_image.py:356-372", "NOT checked"):
        assert cite in m.group(1), cite
    assert int(re.search(r"#define GRL_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION
    from grl_image_restoration_amd import ops

    assert callable(ops.sample_patch_views)
    assert "grl_sample_patch_views" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_parser_options_and_refusals(tmp_path, capsys):
    from grl_image_restoration_amd import evaluate, restore, train

    a = evaluate._parser().parse_args(["--task", "sr", "--scale", "1", "--lq", "L", "--lq-r", "R", "--gt", "G"])
    assert a.lq_r == "R" and evaluate._parser().parse_args(["--gt", "G"]).lq_r is None
    evaluate._check(evaluate._parser(), a)
    assert a.scale == 1
    a = train._parser().parse_args(["--gt", "G", "--lq", "L", "--lq-r", "R", "--val-lq-r", "VR", "--steps", "1", "--scale", "1"])
    assert (a.lq_r, a.val_lq_r) == ("R", "VR")
    assert restore._parser().parse_args(["--lq", "L", "--lq-r", "R", "--out", "O", "--geometry", "defocus"]).lq_r == "R"

    ev = ["--lq", "L", "--lq-r", "R", "--gt", "G"]
    for extra in (["--task", "sr"], ["--task", "sr", "--scale", "2"], ["--task", "sr", "--scale", "1", "--channels", "1"],
                  ["--task", "sr", "--scale", "1", "--usm-gt"], ["--task", "bsr", "--scale", "1"]):
        with pytest.raises(SystemExit) as e:
            evaluate.main(ev + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--task", "dn", "--sigma", "25", "--lq-r", "R", "--gt", "G"])
    assert e.value.code == 2
    tr = ["--gt", "G", "--lq", "L", "--lq-r", "R", "--steps", "1", "--device", "cpu"]
    for extra in (["--scale", "2"], [], ["--scale", "1", "--channels", "1"], ["--scale", "1", "--gan"], ["--scale", "1", "--usm"],
                  ["--scale", "1", "--val-every", "1", "--val-gt", "V", "--val-lq", "VL"]):
        with pytest.raises(SystemExit) as e:
            train.main(tr + extra)
        assert e.value.code == 2, extra
    for args in (["--gt", "G", "--lq-r", "R", "--steps", "1", "--scale", "2", "--degrade"],
                 ["--gt", "G", "--lq", "L", "--val-lq-r", "R", "--steps", "1", "--scale", "1"],
                 ["--task", "dn", "--sigma", "25", "--gt", "G", "--lq-r", "R", "--steps", "1"]):
        with pytest.raises(SystemExit) as e:
            train.main(args + ["--device", "cpu"])
        assert e.value.code == 2, args
    for extra in (["--scale", "2"], ["--channels", "1"]):
        with pytest.raises(SystemExit) as e:
            restore.main(["--lq", "L", "--lq-r", "R", "--out", str(tmp_path / "o"), "--geometry", "defocus"] + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()


def test_preset():
    assert presets.GEOMETRIES["defocus"] == dict(window_size=16, stripe_size=[48, 96], stripe_groups=[None, None], anchor_window_down_factor=4)
    cfg = make_config("base", "defocus", upscale=1, in_channels=6, out_channels=3)
    assert (cfg["in_channels"], cfg["out_channels"], cfg["window_size"], cfg["upsampler"]) == (6, 3, 16, "")


# ---- the network against the real reference ---------------------------------------------------------------------------------------
def fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "tasks", "dual_pixel.npz"), allow_pickle=False)
    return json.loads(str(z["meta"])), z


def fixture_model(meta):
    """The product module with the fixture's weights: the constructor's under seed 0, perturbed (oracle/make_golden_pins.py's recipe)."""
    torch.manual_seed(0)
    m = GRL(**meta["cfg"]).eval()
    m.load_state_dict(O.perturb_state_dict(m.state_dict(), meta["weight_seed"]), strict=True)
    return m


def fixture_input(z, tag):
    return torch.from_numpy(z["input_" + tag]).to(torch.float32).div(255)


def step_batch(meta):
    """The training step's (lq, gt), rebuilt from the seed as tools/make_golden_dual_pixel.py builds them."""
    import torch.nn.functional as F

    def views8(seed, channels):
        g = torch.Generator().manual_seed(seed)
        x = F.avg_pool2d(torch.rand(2, channels, 100, 100, generator=g), 5, 1)
        return (((x - 0.5) * 3.0 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8)

    lq8, gt8 = views8(meta["step_seed"], 6), views8(meta["step_seed"] + 1, 3)
    crc = zlib.crc32(gt8.numpy().tobytes(), zlib.crc32(lq8.numpy().tobytes()))
    assert crc == meta["step_crc32"], "the seeded batch of the fixture's training step is not rebuilt bit for bit"
    return lq8.to(torch.float32).div(255), gt8.to(torch.float32).div(255)


def sample_index(n, k, seed):
    return np.unique(np.random.RandomState(seed).randint(0, n, size=min(k, n)))


def fixture_gradients(z, meta, grads):
    """{name: (got, want)} as flat tensors: whole for the small gradients, the fixture's sample for the large ones."""
    out = {}
    for k, g in grads.items():
        if "grad::" + k in z.files:
            out[k] = (g.detach().cpu().reshape(-1), torch.from_numpy(z["grad::" + k]).reshape(-1))
        else:
            idx = sample_index(g.numel(), meta["grad_sample"], zlib.crc32(k.encode()))
            out[k] = (g.detach().cpu().reshape(-1)[torch.from_numpy(idx)], torch.from_numpy(z["sample::" + k]))
    assert len(out) == sum(f.startswith(("grad::", "sample::")) for f in z.files)
    return out


@pytest.mark.parametrize("tag", ["96x96", "100x90"])
def test_cpu_composite_matches_the_reference(tag):
    meta, z = fixture()
    assert meta["cfg"]["in_channels"] == 6 and meta["cfg"]["out_channels"] == 3 and meta["cfg"]["depths"] == [2, 2]
    m = fixture_model(meta)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            y = m(fixture_input(z, tag))
    want = torch.from_numpy(z["output64_" + tag])
    assert y.shape == want.shape and y.shape[1] == 3
    err = (y.double() - want).abs().max().item()
    print(f"dual-pixel {tag}: max|composite - reference fp64| = {err:.3e} (reference fp32 - fp64: {meta['max_abs_ref32_minus_fp64']:.1e})")
    assert err < 2e-5, err                                   # the bar of tests/test_cpu_composite.py


def test_cpu_composite_gradients_match_the_reference():
    meta, z = fixture()
    m = fixture_model(meta)
    lq, gt = step_batch(meta)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = (m(lq) - gt).abs().mean()
    loss.backward()
    assert abs(loss.item() - meta["loss"]) < 1e-6, (loss.item(), meta["loss"])
    pairs = fixture_gradients(z, meta, {k: p.grad for k, p in m.named_parameters()})
    rel = {k: ((a - b).abs().max() / (b.abs().max() + 1e-30)).item() for k, (a, b) in pairs.items()}
    big = {k: v for k, v in rel.items() if "cpb_mlp" not in k and "logit_scale" not in k}
    worst = max(rel, key=rel.get)
    print(f"dual-pixel step: loss {loss.item():.7f}; worst relative gradient difference {rel[worst]:.2e} ({worst}); without the CPB-MLP / "
          f"scales {max(big.values()):.2e}")
    assert max(big.values()) < 1e-4 and rel[worst] < 1e-3     # the gradient bar of tests/test_cpu_composite.py


# ---- folder runs ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """Three folders (left, right, gt) with two small PNGs each, 120 x 112 and 96 x 100; names sort the same way in all three."""
    from PIL import Image

    root = tmp_path_factory.mktemp("dpdd")
    g = np.random.RandomState(3)
    for name in ("left", "right", "gt"):
        (root / name).mkdir()
        for i, (h, w) in enumerate([(120, 112), (96, 100)]):
            smooth = np.kron(g.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)), np.ones((8, 8, 1)))[:h, :w].astype(np.uint8)
            Image.fromarray(smooth).save(root / name / f"im{i}.png")
    return root


def _small_model():
    torch.manual_seed(0)
    cfg = make_config("tiny", "defocus", upscale=1, img_size=96, in_channels=6, out_channels=3, depths=[1], num_heads_window=[2],
                      num_heads_stripe=[2])
    return GRL(**cfg).eval()


def test_folder_runs_whole_and_tiled(folders, tmp_path):
    from PIL import Image

    from grl_image_restoration_amd import tiling
    from grl_image_restoration_amd.evaluate import _read_image, evaluate_folder, psnr_y
    from grl_image_restoration_amd.restore import restore_folder

    m = _small_model()
    L_, R, G = (str(folders / n) for n in ("left", "right", "gt"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        whole = evaluate_folder(m, L_, G, 1, device="cpu", verbose=False, lq_r_dir=R, save_dir=str(tmp_path / "whole"))
        tiled = evaluate_folder(m, L_, G, 1, tile=96, overlap=16, device="cpu", verbose=False, lq_r_dir=R, save_dir=str(tmp_path / "tiled"),
                                save_gt=True)
        x = torch.cat([_read_image(os.path.join(L_, "im0.png")), _read_image(os.path.join(R, "im0.png"))], dim=1)
        with torch.no_grad():
            y_whole = m(x)
            y_tiled = tiling.forward_tiled(m, x, 96, 16, 1, out_channels=m.out_channels)
            # the reference's stitch (engines/base.py:90-116) by hand: E / W over the tile origins
            E, W = torch.zeros(1, 3, 120, 112), torch.zeros(1, 3, 120, 112)
            for hi in (0, 24):
                for wi in (0, 16):
                    o = m(x[..., hi : hi + 96, wi : wi + 96])
                    E[..., hi : hi + 96, wi : wi + 96] += o
                    W[..., hi : hi + 96, wi : wi + 96] += 1
        assert x.shape == (1, 6, 120, 112) and y_whole.shape == y_tiled.shape == (1, 3, 120, 112)
        # (forward_tiled runs the four tiles as one batch, the loop above one by one: fp32 round-off, the bar of tests/test_cpu_composite.py)
        assert (y_tiled - E / W).abs().max().item() < 2e-5
        # where one tile alone covers a pixel, the stitched output is that tile's output; the top-left tile's input is the image's own
        # corner, and its rows / columns 0 .. 15 lie in no other tile
        with torch.no_grad():
            corner = m(x[..., :96, :96])
        assert (y_tiled[..., :16, :16] - corner[..., :16, :16]).abs().max().item() < 2e-5
        want_whole = float(psnr_y(y_whole, _read_image(os.path.join(G, "im0.png"))))
        paths = restore_folder(m, L_, str(tmp_path / "restored"), 1, tile=96, overlap=16, device="cpu", lq_r_dir=R)
        plain = restore_folder(m, L_, str(tmp_path / "restored_whole"), 1, device="cpu", lq_r_dir=R)
    assert np.isfinite(whole) and np.isfinite(tiled)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            x1 = torch.cat([_read_image(os.path.join(L_, "im1.png")), _read_image(os.path.join(R, "im1.png"))], dim=1)
            want1 = float(psnr_y(m(x1), _read_image(os.path.join(G, "im1.png"))))
    assert whole == pytest.approx((want_whole + want1) / 2, abs=1e-4)
    # saved images: straight under the data set's name, _LQ is the LEFT view's pixels, _HQ has three channels
    for run in ("whole", "tiled"):
        d = tmp_path / run / "gt"
        assert sorted(os.listdir(d))[:2] == ["im0_GT.png", "im0_HQ.png"] if run == "tiled" else sorted(os.listdir(d)) == [
            "im0_HQ.png", "im0_LQ.png", "im1_HQ.png", "im1_LQ.png"]
        for i in (0, 1):
            lq_saved = np.asarray(Image.open(d / f"im{i}_LQ.png"))
            assert lq_saved.tobytes() == np.asarray(Image.open(os.path.join(L_, f"im{i}.png")).convert("RGB")).tobytes()
            assert lq_saved.tobytes() != np.asarray(Image.open(os.path.join(R, f"im{i}.png")).convert("RGB")).tobytes()
            assert np.asarray(Image.open(d / f"im{i}_HQ.png")).shape == lq_saved.shape and lq_saved.shape[2] == 3
    assert [os.path.basename(p) for p in paths] == ["im0_HQ.png", "im1_HQ.png"]
    hq = np.asarray(Image.open(paths[0]))
    assert hq.shape == (120, 112, 3)
    assert hq.tobytes() == np.asarray(Image.open(tmp_path / "tiled" / "gt" / "im0_HQ.png")).tobytes()
    assert np.asarray(Image.open(plain[0])).tobytes() == np.asarray(Image.open(tmp_path / "whole" / "gt" / "im0_HQ.png")).tobytes()
    with pytest.raises(ValueError):
        evaluate_folder(m, L_, G, 2, device="cpu", verbose=False, lq_r_dir=R)
    with pytest.raises(ValueError):
        restore_folder(m, L_, str(tmp_path / "bad"), 2, device="cpu", lq_r_dir=R)


def test_train_cli_two_eager_steps_on_cpu_stores(folders, tmp_path, capsys):
    from grl_image_restoration_amd import train
    from grl_image_restoration_amd.evaluate import load_checkpoint

    L_, R, G = (str(folders / n) for n in ("left", "right", "gt"))
    args = ["--task", "sr", "--scale", "1", "--model", "tiny", "--geometry", "defocus", "--depths", "1", "--patch", "96", "--batch", "2",
            "--gt", G, "--lq", L_, "--lq-r", R, "--eager", "--device", "cpu", "--lr", "1e-3", "--steps", "2",
            "--val-every", "2", "--val-gt", G, "--val-lq", L_, "--val-lq-r", R, "--out", str(tmp_path / "run")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(0)
        r = train.main(args)
        torch.manual_seed(0)
        plain = train.main([a for a in args[: args.index("--val-every")] if a not in ("--lq-r", R)])     # the same run without the right view
    assert r["steps"] == [0, 1] and all(np.isfinite(r["losses"])) and len(r["val"]) == 1 and np.isfinite(r["val"][0][1])
    assert r["work"] == plain["work"]                                   # the draws do not know about the right store
    obj = torch.load(r["checkpoint"], map_location="cpu", weights_only=False)
    assert obj["step"] == 2 and obj["state_dict"]["model.conv_first.weight"].shape[1] == 6
    assert obj["state_dict"]["model.conv_last.weight"].shape[0] == 3 and set(obj["sampler_rng"]) == {"draws", "noise"}
    m = GRL(**make_config("tiny", "defocus", upscale=1, img_size=96, in_channels=6, out_channels=3, depths=[1], num_heads_window=[2],
                          num_heads_stripe=[2]))
    res = load_checkpoint(m, r["checkpoint"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    capsys.readouterr()
