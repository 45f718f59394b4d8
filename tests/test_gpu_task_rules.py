"""The training LQ of every trainable task through ``PatchSampler`` on a CUDA store against the same store on the CPU: one work
list with a padded crop and all three flags, the per-task builders of ``tasks.TRAIN_STORE_LQ`` / ``tasks.TRAIN_PAIR`` behind the rule
table.  ``gt`` is bitwise equal for every task; ``lq`` is bitwise equal where the front end documents it (sr: the patch kernel; dm:
dyadic filter weights; jpeg: integer arithmetic), within the existing GPU tests' bounds for sr_bicubic (tests/test_gpu_resize.py's
BAR on the resize before its 8-bit rounding) and db (tests/test_blur.py's ``bound``), and a matter of statistics for dn, whose device
generator has its own stream.  The sampler's work list and quality list keep their addresses."""
import numpy as np
import pytest
import torch

from grl_image_restoration_amd import PatchSampler, PatchStore, tasks as T
from tests.test_blur import bound
from tests.test_gpu_resize import BAR
from tests.test_tasks import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, B = 16, 2
FLAGS = 7                                                        # rows reversed, columns reversed, axes swapped
# (image, x, y, flags): the second crop runs over the bottom and right edges of its image on the side the draws are made on
WORK = {"lq 20 x 24": [(0, 1, 2, FLAGS), (1, 10, 12, 1)], "40 x 48": [(0, 1, 2, FLAGS), (1, 30, 40, 1)]}
QUALITIES = [10, 37]

_IMAGES = []


def images():
    if not _IMAGES:
        g = np.random.RandomState(8)
        _IMAGES.extend(g.randint(0, 256, (40, 48, 3)).astype(np.uint8) for _ in range(2))
    return _IMAGES


def taps13():
    taps = golden("db")[1]["taps_real5"]
    assert taps.shape == (13, 13)
    return taps


def samplers(task, **kw):
    gt, kw = images(), dict(kw)
    if task == "sr":                                             # an LQ store of half the size; its content is free
        kw["lq_store"] = [im[::2, ::2].copy() for im in gt]
    out = []
    for dev in ("cpu", DEV):
        k = dict(kw)
        if "lq_store" in k:
            k["lq_store"] = PatchStore(k["lq_store"], dev)
        out.append(PatchSampler(task, PatchStore(gt, dev), patch=P, batch=B, seed=3, **k))
    return out


CASES = {
    "sr": ("sr", dict(scale=2), "lq 20 x 24"),
    "sr_bicubic": ("sr_bicubic", dict(scale=2), "lq 20 x 24"),
    "dm": ("dm", {}, "40 x 48"),
    "jpeg_fixed": ("jpeg", dict(quality=10), "40 x 48"),
    "jpeg_range": ("jpeg", dict(quality_range=(10, 40)), "40 x 48"),
    "db": ("db", dict(taps=None), "40 x 48"),
    "dn": ("dn", dict(sigma=25), "40 x 48"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_cuda_store_against_cpu_store(case):
    task, kw, where = CASES[case]
    if "taps" in kw:
        kw = dict(kw, taps=taps13())
    cpu, gpu = samplers(task, **kw)
    work = WORK[where]
    extra = {}
    if case == "jpeg_range":
        extra["sigmas"] = QUALITIES
    if task == "db":
        extra["noise"] = torch.randn(B, 3, P, P, generator=torch.Generator().manual_seed(2))
    work_ptr = gpu.work.data_ptr()
    q_ptr = gpu.qualities.data_ptr() if gpu.qualities is not None else None
    lq_c, gt_c = cpu.next(work, **extra)
    lq_g, gt_g = gpu.next(work, **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in extra.items()})
    assert gpu.work.data_ptr() == work_ptr and gpu.work.tolist() == [list(w) for w in work]
    assert (case == "jpeg_range") == (q_ptr is not None)
    if q_ptr is not None:
        assert gpu.qualities.data_ptr() == q_ptr and gpu.qualities.tolist() == QUALITIES

    assert lq_g.is_cuda and gt_g.is_cuda and lq_g.shape == lq_c.shape == (B, 3, P, P) and gt_g.shape == gt_c.shape
    assert torch.equal(gt_g.cpu(), gt_c)
    assert float(gt_c[1][..., 0, :].abs().max()) == 0.0 and float(gt_c[0][..., 0, :].abs().max()) > 0.0   # the second crop is padded
    lq_g = lq_g.cpu()
    if case in ("sr", "dm", "jpeg_fixed", "jpeg_range"):
        assert torch.equal(lq_g, lq_c)
    elif case == "sr_bicubic":
        # the batch is the patch kernel's crop of the 8-bit LQ store ...
        back = PatchStore([gpu.lq_store.image(n).cpu() for n in range(2)])
        assert torch.equal(lq_g, back.sample(torch.tensor(work, dtype=torch.int32), P, 1))
        # ... and every level of that store is the 8-bit rounding of a resize within BAR of the CPU path's float64 one
        for n in range(2):
            assert torch.equal(gpu.gt_store.image(n).cpu(), cpu.gt_store.image(n))
            gt = cpu.gt_store.image(n).permute(2, 0, 1).unsqueeze(0).float() / 255
            exact = T.sr_lq(gt, 2, quantize=False)[0].clamp(0, 1)
            got = gpu.lq_store.image(n).cpu().permute(2, 0, 1).unsqueeze(0).float() / 255
            err = float((got - exact).abs().max())
            print(f"sr_bicubic image {n}: |8-bit hip LQ - cpu resize| {err:.3e}, half a level {0.5 / 255:.3e}, BAR {BAR:.1e}; "
                  f"levels that differ from the CPU store: {int((gpu.lq_store.image(n).cpu() != cpu.lq_store.image(n)).sum())}")
            assert err <= 0.5 / 255 + BAR
    elif case == "db":
        K = kw["taps"].shape[0]
        big = cpu.gt_store.sample(torch.tensor(work, dtype=torch.int32), P + K - 1, 1)
        err, b = float((lq_g - lq_c).abs().max()), bound(K, big)
        print(f"db: |hip - cpu| {err:.3e}, bound {b:.3e}")
        assert err <= b
    else:
        # 2 * 3 * 16 * 16 = 1536 samples: the standard error of the estimate is 1 / sqrt(2 * 1536) = 0.018
        ratio = float((lq_g - gt_c).std()) * 255 / 25
        print(f"dn: std(lq - gt) * 255 / sigma = {ratio:.4f}")
        assert abs(ratio - 1) <= 0.1
