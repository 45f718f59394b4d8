"""Writes tests/golden/tasks/db.npz: what the reference's non-blind deblurring front end (data module ``db``) produces.

Everything comes from the UNMODIFIED reference, imported from its tree (GRL_REFERENCE_ROOT, as for oracle/refshim.py):
  * utils/utils_deblur.py (``fspecial``, ``get_blur_kernel``) and the Levin09 kernels it reads at run time from
    utils/blur_kernels/Levin09.npy.  Its ``fspecial_gaussian`` calls ``scipy.finfo``, an alias of ``numpy.finfo`` that scipy removed
    (1.12); the stand-in ``scipy.finfo = np.finfo`` is installed before the call and is the ONLY thing changed around the reference;
  * the validation noise is made by ``DeblurDataset.__getitem__`` (data/datasets/restoration_db.py:29-50) itself, on an instance
    built with ``object.__new__`` whose loading hooks hand over a given image (tools/make_golden_tasks.py's stand-ins);
  * the engine's six lines (engines/base.py:131-142) are restated in ``engine_db``: ``input_ += F.conv2d(target, blur_kernel,
    groups=3, padding=(bkh, bkw))`` and, for training, the crop by (bkh, bkw) of input and target -- once in fp32 as the engine runs
    it, once with every operand cast to float64.

The file holds (plus a JSON ``meta`` that lists the cases and the kernel of each):
  levin_1 .. levin_8      the eight Levin09 kernels, float64 (19, 17, 15, 27, 13, 21, 23, 23 pixels square)
  gaussian                ``fspecial('gaussian', 25, 1.6)``, float64
  taps_<kernel>           ``get_blur_kernel(kernel)[0, 0]``: the fp32 correlation taps, for gaussian, real4 (27 x 27), real5 (13 x 13)
  <case>__gt              uint8 (N, 3, H, W) ground truth
  <case>__noise           fp32, the LQ's shape: DeblurDataset's validation noise (sigma 2, seed 0 for every image); for the training
                          cases ``normal(0, 2 / 255)`` from a seeded generator at the enlarged size, cropped like the LQ
  <case>__lq32 / __lq64   the engine's LQ in fp32 and in float64
  <case>__target          training cases: the cropped target, uint8
Validation cases (zero padding): 8 x 9 and 25 x 25 (gaussian), 13 x 40 (real5), 40 x 56 as a batch of 2 (gaussian), 40 x 56 (real4).
Training cases (the valid region): one (2, 3, 16 + K - 1, 16 + K - 1) batch per kernel, and 27 x 27 under real4 (a 1 x 1 output).

    python tools/make_golden_db.py [--reference DIR] [--out tests/golden/tasks]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402
from tools.make_golden_tasks import OUT, _dataset, _install_stubs, _texture, _to_tensor  # noqa: E402

SIGMA = 2
KERNELS = ("gaussian", "real4", "real5")
VAL_CASES = [("g_8x9", "gaussian", 1, 8, 9), ("g_25x25", "gaussian", 1, 25, 25), ("r5_13x40", "real5", 1, 13, 40),
             ("g_40x56_b2", "gaussian", 2, 40, 56), ("r4_40x56", "real4", 1, 40, 56)]
TRAIN_PATCH = 16


def engine_db(noise, target, blur_kernel, training, dtype):
    """engines/base.py:131-142 on a batch: returns (input_, target)."""
    input_, target = noise.to(dtype).clone(), target.to(dtype)
    bkh, bkw = [s // 2 for s in blur_kernel.shape[2:]]
    input_ += F.conv2d(target, blur_kernel.to(input_.device, input_.dtype), groups=3, padding=(bkh, bkw))
    if training:
        input_ = input_[:, :, bkh:-bkh, bkw:-bkw]
        target = target[:, :, bkh:-bkh, bkw:-bkw]
    return input_, target


def _images(g, N, H, W):
    """N seeded 8-bit images (HWC): a texture where there is room for one, plain noise below that."""
    if min(H, W) >= 32:
        return [_texture(g, H, W) for _ in range(N)]
    return [g.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(N)]


def build(DB, U):
    arrays, cases = {}, []
    levin = np.load(os.path.join(os.path.dirname(U.__file__), "blur_kernels", "Levin09.npy"), allow_pickle=True)
    for i in range(8):
        arrays[f"levin_{i + 1}"] = np.ascontiguousarray(levin[0, i], dtype=np.float64)
    arrays["gaussian"] = U.fspecial("gaussian", 25, 1.6)
    kern = {k: U.get_blur_kernel(k) for k in KERNELS}
    for k in KERNELS:
        arrays[f"taps_{k}"] = kern[k][0, 0].numpy()
    g = np.random.RandomState(11)
    for name, k, N, H, W in VAL_CASES:
        imgs = _images(g, N, H, W)
        items = [_dataset(DB.DeblurDataset, im, stage="val", noise_sigma=SIGMA / 255.0, img_info=[("set5/x.png",)])[0] for im in imgs]
        noise = torch.stack([it["img_lq"] for it in items])
        gt = torch.stack([it["img_gt"] for it in items])
        assert torch.equal(gt, torch.stack([_to_tensor(im) for im in imgs]))
        arrays[f"{name}__gt"] = np.stack([im.transpose(2, 0, 1) for im in imgs])
        arrays[f"{name}__noise"] = noise.numpy()
        arrays[f"{name}__lq32"] = engine_db(noise, gt, kern[k], False, torch.float32)[0].numpy()
        arrays[f"{name}__lq64"] = engine_db(noise, gt, kern[k], False, torch.float64)[0].numpy()
        cases.append(dict(name=name, kernel=k, pad="same", shape=[N, 3, H, W]))
    for name, k, N, S in [(f"v_{k}", k, 2, TRAIN_PATCH + kern[k].shape[2] - 1) for k in KERNELS] + [("v_real4_27", "real4", 1, 27)]:
        imgs = _images(g, N, S, S)
        gt = torch.stack([_to_tensor(im) for im in imgs])
        # restoration_db.py:42-43 in the training stage (np.random unseeded there; seeded here so the file can be rewritten)
        noise = torch.from_numpy(np.random.RandomState(5).normal(0, SIGMA / 255.0, tuple(gt.shape)).astype(np.float32))
        lq32, tgt = engine_db(noise, gt, kern[k], True, torch.float32)
        lq64, _ = engine_db(noise, gt, kern[k], True, torch.float64)
        b = kern[k].shape[2] // 2
        arrays[f"{name}__gt"] = np.stack([im.transpose(2, 0, 1) for im in imgs])
        arrays[f"{name}__noise"] = noise[:, :, b:-b, b:-b].contiguous().numpy()
        arrays[f"{name}__lq32"] = lq32.contiguous().numpy()
        arrays[f"{name}__lq64"] = lq64.contiguous().numpy()
        arrays[f"{name}__target"] = (tgt * 255).round().to(torch.uint8).numpy()
        cases.append(dict(name=name, kernel=k, pad="valid", shape=[N, 3, S, S]))
    meta = dict(cases=cases, sigma=SIGMA, kernels=list(KERNELS), levin_sizes=[int(arrays[f"levin_{i + 1}"].shape[0]) for i in range(8)],
                source="utils/utils_deblur.py get_blur_kernel / fspecial; DeblurDataset.__getitem__ (stage val); engines/base.py:131-142")
    return arrays, meta


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=refshim.REFERENCE_ROOT)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args(argv)
    if a.reference != refshim.REFERENCE_ROOT:
        refshim.REFERENCE_ROOT = a.reference
    _install_stubs(a.reference)
    import scipy

    if not hasattr(scipy, "finfo"):
        scipy.finfo = np.finfo                      # the alias fspecial_gaussian was written against (module docstring)
    from data.datasets import restoration_db as DB
    from utils import utils_deblur as U

    arrays, meta = build(DB, U)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "db.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
