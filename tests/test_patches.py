"""CPU tests of the training data path (data.py) and the pieces of train.py that need no model: the patch sampler against a numpy
restatement of the reference's chain (_pad_images, _random_index, _sample_patches, _augment of data/datasets/base_image.py and
torchvision's to_tensor), the draw order, the learning-rate schedule against the reference's class and recorded values, the
Charbonnier loss, the ABI entry, and the four tasks' batches."""
import os
import random

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import PatchSampler, PatchStore, _lib, charbonnier, multistep_warmup_lr, tasks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(37, 53), (64, 40), (20, 20)]          # LQ-side sizes; with P = 24 the last one is padded in both directions
P, B = 24, 11


def make_images(channels, scale=1, seed=3):
    """uint8 images of SIZES x scale; every level 0..255 occurs in the first one."""
    g = np.random.RandomState(seed + 10 * channels + scale)
    imgs = [g.randint(0, 256, (h * scale, w * scale, channels)).astype(np.uint8) for h, w in SIZES]
    imgs[0].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return imgs


def work_list():
    """B = 11 entries over the three images, all eight flag values, origins including the last valid one."""
    w = []
    for b in range(B):
        n = b % 3
        H, W = max(SIZES[n][0], P), max(SIZES[n][1], P)
        x = [0, H - P, (H - P) // 2][b % 3 if b < 9 else 1]
        y = [W - P, 0, (W - P) // 3][(b // 3) % 3]
        w.append((n, x, y, b % 8))
    return w


# ---- the reference's chain, restated in numpy --------------------------------------------------------------------------------
def _pad_images(imgs, patch, scale):
    h, w = imgs[0].shape[:2]
    if h < patch * scale or w < patch * scale:
        padding = ((0, max(0, patch * scale - h)), (0, max(0, patch * scale - w)), (0, 0))
        imgs = [np.pad(i, padding, "constant", constant_values=0) for i in imgs]
    return imgs


def _random_index(img, patch):
    h, w = img.shape[:2]
    return random.randrange(0, h - patch + 1), random.randrange(0, w - patch + 1)


def _sample_patches(imgs, x, y, patch, scale):
    return [i[x * scale : x * scale + patch * scale, y * scale : y * scale + patch * scale] for i in imgs]


def _augment(images, flags=None):
    """base_image.py:356-372; ``flags`` replaces the three draws."""
    f = [random.random() < 0.5 for _ in range(3)] if flags is None else [bool(flags & 1), bool(flags & 2), bool(flags & 4)]
    if f[0]:
        images = [x[::-1] for x in images]
    if f[1]:
        images = [x[:, ::-1] for x in images]
    if f[2]:
        images = [np.swapaxes(x, 0, 1) for x in images]
    return images, f[0] * 1 + f[1] * 2 + f[2] * 4


def to_tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def reference_pair(lq_imgs, gt_imgs, work, patch, scale):
    lqs, gts = [], []
    for n, x, y, flags in work:
        (lq,), (gt,) = _pad_images([lq_imgs[n]], patch, 1), _pad_images([gt_imgs[n]], patch, scale)
        (lq,), (gt,) = _sample_patches([lq], x, y, patch, 1), _sample_patches([gt], x, y, patch, scale)
        (lq, gt), _ = _augment([lq, gt], flags)
        lqs.append(to_tensor(lq)); gts.append(to_tensor(gt))
    return torch.stack(lqs), torch.stack(gts)


_REF = {}


def reference_case(channels, scale, patch=P):
    """(lq images, gt images, work list, reference lq, reference gt), computed once per case and shared with the GPU tests."""
    key = (channels, scale, patch)
    if key not in _REF:
        lq_imgs, gt_imgs = make_images(channels, 1), make_images(channels, scale)
        work = [(n, min(x, max(SIZES[n][0], patch) - patch), min(y, max(SIZES[n][1], patch) - patch), f) for n, x, y, f in work_list()]
        _REF[key] = (lq_imgs, gt_imgs, work) + reference_pair(lq_imgs, gt_imgs, work, patch, scale)
    return _REF[key]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("scale", [1, 2])
def test_sampler_equals_the_reference_chain(channels, scale):
    lq_imgs, gt_imgs, work, want_lq, want_gt = reference_case(channels, scale)
    assert {w[3] for w in work} == set(range(8)) and len(work) == B
    s = PatchSampler("sr", PatchStore(gt_imgs), PatchStore(lq_imgs), patch=P, batch=B, scale=scale)
    lq, gt = s.next(work)
    assert lq.shape == (B, channels, P, P) and gt.shape == (B, channels, P * scale, P * scale) and gt.dtype == torch.float32
    assert torch.equal(lq, want_lq) and torch.equal(gt, want_gt)
    lq_t, _ = s.next(torch.tensor(work, dtype=torch.int32))           # the list as a tensor
    assert torch.equal(lq_t, want_lq)
    assert float(gt[2].abs().max()) > 0 and float((gt[2] == 0).float().mean()) > 0.2      # the 20 x 20 image: zero padding


@pytest.mark.parametrize("k", [0, 7])
def test_draw_order_is_the_reference(k):
    imgs = make_images(3)
    s = PatchSampler("sr", PatchStore(imgs), PatchStore(imgs), patch=P, batch=B, scale=1, seed=k)
    got, _ = s.draw()
    random.seed(k)
    want = []
    for _ in range(B):
        n = random.randrange(len(imgs))
        (img,) = _pad_images([imgs[n]], P, 1)
        x, y = _random_index(img, P)
        _, flags = _augment([img])
        want.append((n, x, y, flags))
    assert got == want


CASE = dict(base_lr=2e-4, milestones=[30, 50, 65, 70, 75], gamma=0.5, warmup_iter=10, warmup_init_lr=1e-5)


def test_schedule_equals_the_recorded_values():
    z = np.load(os.path.join(ROOT, "tests", "golden", "train", "lr_schedule.npz"))
    want = z["lr"].tolist()
    assert len(want) == 80 and z["milestones"].tolist() == CASE["milestones"]
    got = [multistep_warmup_lr(n, **CASE) for n in range(80)]
    assert got == want                                                   # exact float equality
    assert got[0] == 1e-5 and got[29] != got[30] and got[79] < got[10] / 16


def test_schedule_equals_the_reference_class():
    from oracle.refshim import REFERENCE_ROOT

    if not os.path.isfile(os.path.join(REFERENCE_ROOT, "optim", "multi_steplr.py")):
        pytest.skip("reference tree not present")
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden_train import reference_schedule

    cases = [dict(CASE, steps=80), dict(base_lr=1e-3, milestones=[3, 3, 5], gamma=0.1, warmup_iter=-1, warmup_init_lr=0, steps=8),
             dict(base_lr=1e-3, milestones=[0, 2, 4], gamma=0.3, warmup_iter=3, warmup_init_lr=1e-4, steps=8)]
    for c in cases:
        want = reference_schedule(REFERENCE_ROOT, **c)
        c = dict(c)
        steps = c.pop("steps")
        assert [multistep_warmup_lr(n, **c) for n in range(steps)] == want, c


def test_charbonnier_value_and_gradient():
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(2, 3, 16, 16, generator=g), torch.rand(2, 3, 16, 16, generator=g)
    x[0, 0, 0, :4] = y[0, 0, 0, :4]                                       # zero differences: the eps term alone
    x.requires_grad_(True)
    loss = charbonnier(x, y)
    loss.backward()
    d = x.detach().double() - y.double()
    r = torch.sqrt(d * d + 1e-3 ** 2)
    assert abs(float(loss.detach()) - float(r.mean())) < 1e-7
    assert float((x.grad.double() - d / r / d.numel()).abs().max()) < 1e-7
    assert abs(float(charbonnier(y, y, eps=0.5)) - 0.5) < 1e-7


def test_patch_args_layout_matches_header_and_abi():
    """The layout of GrlPatchArgs is compared with the header in tests/test_abi.py, like every struct's;
    what is particular to this entry point stays here."""
    assert _lib.ABI_VERSION >= 27
    assert "grl_sample_patches" in _lib.EXPORTS


def _on_grid(t):
    return bool((((t * 255).round() / 255) == t).all()) and float(t.min()) >= 0 and float(t.max()) <= 1


def test_tasks_on_the_cpu():
    gt_imgs = [np.random.RandomState(i).randint(0, 256, (72 + 8 * i, 96, 3)).astype(np.uint8) for i in range(2)]
    work = [(0, 3, 5, 0), (1, 10, 2, 5), (0, 0, 0, 7)]
    # sr: paired stores
    lq_imgs = [np.ascontiguousarray(g[::2, ::2]) for g in gt_imgs]
    lq, gt = PatchSampler("sr", PatchStore(gt_imgs), PatchStore(lq_imgs), patch=16, batch=3, scale=2).next(work)
    assert lq.shape == (3, 3, 16, 16) and gt.shape == (3, 3, 32, 32) and _on_grid(gt) and _on_grid(lq)
    assert torch.equal(gt[0, :, ::2, ::2], lq[0])
    with pytest.raises(ValueError):
        PatchSampler("sr", PatchStore(gt_imgs), None, patch=16, batch=3, scale=2)
    with pytest.raises(ValueError):
        PatchSampler("sr", PatchStore(gt_imgs), PatchStore(gt_imgs), patch=16, batch=3, scale=2)      # not a x2 pair
    # sr_bicubic: the LQ patch is the crop of tasks.sr_lq of the whole image
    odd = [g[:-1, :-1] for g in gt_imgs]                                   # 71 x 95: cropped to 70 x 94 first
    s = PatchSampler("sr_bicubic", PatchStore(odd), patch=16, batch=3, scale=2)
    lq, gt = s.next([(0, 3, 5, 0), (1, 10, 2, 0), (0, 19, 31, 0)])
    assert lq.shape == (3, 3, 16, 16) and gt.shape == (3, 3, 32, 32) and _on_grid(gt) and _on_grid(lq)
    whole = torch.from_numpy(np.ascontiguousarray(odd[1])).permute(2, 0, 1).unsqueeze(0).float().div(255)
    want_lq, want_gt = tasks.sr_lq(whole, 2)
    assert torch.equal(lq[1], want_lq[0, :, 10:26, 2:18]) and torch.equal(gt[1], want_gt[0, :, 20:52, 4:36])
    assert s.lq_store.dims[0] == (35, 47) and s.gt_store.dims[0] == (70, 94)
    # dm
    lq, gt = PatchSampler("dm", PatchStore(gt_imgs), patch=16, batch=3).next(work)
    assert lq.shape == gt.shape == (3, 3, 16, 16) and _on_grid(gt)
    assert torch.equal(lq, tasks.demosaic_gt(gt)) and torch.equal(lq[:, 0, ::2, ::2], gt[:, 0, ::2, ::2])
    with pytest.raises(ValueError):
        PatchSampler("dm", PatchStore(gt_imgs), patch=15, batch=3)
    # dn: the asked standard deviation, fixed and per sample
    big = [np.random.RandomState(5).randint(0, 256, (80, 80, 3)).astype(np.uint8)]
    s = PatchSampler("dn", PatchStore(big), patch=64, batch=8, sigma=25, seed=1)
    lq, gt = s.next()
    assert lq.shape == gt.shape == (8, 3, 64, 64) and _on_grid(gt)
    assert abs(float((lq - gt).std()) / (25 / 255) - 1) < 0.05
    s = PatchSampler("dn", PatchStore(big), patch=64, batch=8, sigma_range=(5, 50), seed=1)
    work, sigmas = s.draw()
    lq, gt = s.next(work, sigmas)
    assert len(sigmas) == 8 and all(5 <= v <= 50 for v in sigmas) and len(set(sigmas)) == 8
    for b in range(8):
        assert abs(float((lq[b] - gt[b]).std()) / (sigmas[b] / 255) - 1) < 0.05
    with pytest.raises(ValueError):
        PatchSampler("dn", PatchStore(big), patch=64, batch=8)
    # one channel, the rng state round trip
    grey = [g[:, :, 0] for g in gt_imgs]
    s = PatchSampler("dn", PatchStore(grey), patch=16, batch=2, sigma=15, seed=4)
    assert s.gt_store.channels == 1 and len(s.gt_store) == 2 and s.gt_store.dims == [(72, 96), (80, 96)]
    state = s.rng_state()
    a = s.next()
    s.set_rng_state(state)
    b = s.next()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape == (2, 1, 16, 16)


def test_store_from_folder_reads_like_evaluate(tmp_path):
    from PIL import Image

    from grl_image_restoration_amd.evaluate import _read_image

    g = np.random.RandomState(0)
    for i, (h, w) in enumerate([(12, 9), (7, 15)]):
        Image.fromarray(g.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(tmp_path / f"im{i}.png")
    (tmp_path / "notes.txt").write_text("not an image")
    for ch, mode in ((3, "RGB"), (1, "L")):
        st = PatchStore.from_folder(str(tmp_path), ch)
        assert len(st) == 2 and st.channels == ch and st.dims == [(12, 9), (7, 15)]
        for i in range(2):
            want = _read_image(str(tmp_path / f"im{i}.png"), mode)[0]
            assert torch.equal(st.image(i).permute(2, 0, 1).float().div(255), want)
    with pytest.raises(TypeError):
        PatchStore([np.zeros((4, 4, 3), dtype=np.float32)])
