"""Checkpoint loading and PSNR-Y evaluation without Lightning / Hydra.

Restates, for the MI355X module, the three pieces of the reference's evaluation command
(``scripts/grl/grl_test.md:73-79``) that sit around ``model(x)``:

  load_checkpoint   tools/trainer.py:93-115    Lightning ``{"state_dict": {"model.<key>": ...}}``, ``{"params": ...}`` or a
                                               plain state dict; geometry buffers dropped by ``convert_checkpoint``
  psnr_y            engines/base.py:256-268    tensor_round -> shave(scale) for SR -> PSNR on the matlab-style Y channel
                    utils/utils_image.py:8-11,30-33,43-79; utils/metrics/psnr.py:44-48
  evaluate_folder   the validation loop over an LQ / GT image folder pair (whole image, or the reference's tiled
                    inference through ``tiling.forward_tiled``); with ``metric_group`` one of the reference's metric groups
                    (config/metric/*.yaml, ``metrics.image_metrics``) instead of PSNR-Y alone
  task_inputs       the tasks whose LQ the reference builds from the GT, on the device, the whole image before any tiling.  The
                    tasks, their options and the reference's definition of each: ``task_rules.RULES``; the LQ of each:
                    ``tasks.VAL_LQ``.  "bsr" reads LQ images only and is scored by NIQE (``metrics.niqe``) against the pristine model
                    the user names with ``--niqe-params`` or the environment variable GRL_NIQE_PARAMS

    python -m grl_image_restoration_amd.evaluate --model base --geometry sr_ckpt_df2 --scale 4 \\
        --ckpt sr_grl_base_c3x4.ckpt --lq Set5/LRbicx4 --gt Set5/GTmod12 [--tile 256 --overlap 32] [--metric restorer]
    python -m grl_image_restoration_amd.evaluate --task dm --model small --geometry dm --ckpt dm_grl_small.ckpt \\
        --gt kodak24 --metric restorer
    python -m grl_image_restoration_amd.evaluate --task dn --sigma 25 --model small --geometry dn_df4 \\
        --ckpt dn_grl_small_c3s25.ckpt --gt kodak24 --noise-prefix Kodak24 --metric restorer
    python -m grl_image_restoration_amd.evaluate --task sr_bicubic --scale 4 --model base --geometry sr_ckpt_df2 \\
        --ckpt sr_grl_base_c3x4.ckpt --gt Set5/original --metric restorer
    python -m grl_image_restoration_amd.evaluate --task db --model small --geometry dn_df4 --ckpt runs/db/step_400000.ckpt \\
        --gt Set5/original [--blur-kernel real4 --blur-kernel-file Levin09.npy]
    python -m grl_image_restoration_amd.evaluate --task jpeg --quality 10 --model small --geometry jpeg --ckpt jpeg_grl_small_c3q10.ckpt \\
        --gt LIVE1 --metric restorer_jpeg
    python -m grl_image_restoration_amd.evaluate --task bsr --model base --geometry bsr --upsampler nearest+conv \\
        --ckpt bsr_grl_base.ckpt --lq RealSRSet --niqe-params niqe_pris_params.npz
    python -m grl_image_restoration_amd.evaluate --model base --geometry bsr --upsampler nearest+conv --scale 4 --ckpt bsr_grl_base.ckpt \\
        --lq DIV2K_val/LRbicx4 --gt DIV2K_val/HR --metric restorer_perceptual --lpips-vgg vgg16-397923af.pth --lpips-lin vgg.pth \\
        --niqe-params niqe_pris_params.npz
    python -m grl_image_restoration_amd.evaluate --model base --geometry bsr_psnr --upsampler nearest+conv --scale 4 \\
        --ckpt bsr_psnr.ckpt --lq Set5/LRbicx4 --gt Set5/GTmod12 --usm-gt      scores against the USM-sharpened GT (val.use_usm: True)
    python -m grl_image_restoration_amd.evaluate --task sr --scale 1 --model base --geometry defocus --tile 480 --overlap 48 \\
        --ckpt db_defocus_dual_pixel_grl_base.ckpt --lq DPDD/test/inputL --lq-r DPDD/test/inputR --gt DPDD/test/target
                                                  dual-pixel defocus deblurring: the two views side by side, a 6-in / 3-out model
    ... --self-ensemble                   the x8 geometric self-ensemble (ensemble.py): the "+" rows of the tables
    ... --save-dir results [--save-gt]    also writes results/X4/<data set>/<stem>_{LQ,HQ,GT}.png (image8.py), as the reference does
"""
import argparse
import contextlib
import os
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from .task_rules import RULES, TASKS, add_task_arguments, load_taps, resolve, resolve_arguments  # noqa: F401

_METRIC_KEYS = ("current_val_metric", "best_val_metric", "best_iter")


def extract_state_dict(obj: Dict, ema: bool = False) -> Dict[str, torch.Tensor]:
    """The parameter dictionary inside whatever ``torch.load`` returned (tools/trainer.py:97-104): a Lightning checkpoint
    (``state_dict`` with ``model.`` prefixes and the trainer's metric entries), a BasicSR-style ``params`` dictionary,
    or already a plain state dict.  ``ema``: the averaged weights instead -- ``state_dict_ema`` (what ``train --ema-decay`` writes,
    same key layout as ``state_dict``) or BasicSR's ``params_ema``; a checkpoint with neither is refused by name."""
    sd = obj
    if ema:
        if isinstance(sd, dict) and "state_dict_ema" in sd:
            return dict(sd["state_dict_ema"])
        if isinstance(sd, dict) and "params_ema" in sd:
            return sd["params_ema"]
        raise KeyError("the checkpoint has no averaged weights: neither 'state_dict_ema' (train --ema-decay) nor BasicSR's 'params_ema'")
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = dict(sd["state_dict"])
        for k in _METRIC_KEYS:
            sd.pop(k, None)
    if isinstance(sd, dict) and "params" in sd:
        sd = sd["params"]
    if not isinstance(sd, dict):
        raise TypeError(f"not a checkpoint dictionary: {type(obj).__name__}")
    return sd


def load_checkpoint(model, path_or_obj, strict: bool = True, ema: bool = False):
    """Load a reference checkpoint into ``model`` (a ``grl_image_restoration_amd.GRL``).  Mirrors tools/trainer.py:93-115:
    geometry buffers (``table_*/index_*/mask_*``, ``relative_*``, ``attn_mask``) are dropped, the Lightning module prefix
    ``model.`` is removed, and -- as trainer.py:106-108 does -- the checkpoint is merged INTO the module's current state before
    the strict load: a partial checkpoint keeps the current values of the keys it lacks, an unknown key still fails.
    (The other direction: ``GRL.state_dict()`` has no ``table_/index_/mask_`` buffers, so loading it into the reference module
    needs ``strict=False`` or the reference's own buffers merged in the same way.)  ``ema=True`` loads the averaged weights
    (``state_dict_ema`` / ``params_ema``, see ``extract_state_dict``) and raises KeyError when the checkpoint has none."""
    obj = torch.load(path_or_obj, map_location="cpu") if isinstance(path_or_obj, (str, os.PathLike)) else path_or_obj
    sd = _gan_part(extract_state_dict(obj, ema=ema), "model_g.", "model.")
    sd = model.convert_checkpoint(dict(sd))           # needs the un-stripped "model.table_*" names (grl.py:556-569)
    sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}
    cur = dict(model.state_dict())
    cur.update(sd)
    return model.load_state_dict(cur, strict=strict)


def _gan_part(sd, part: str, prefix: str):
    """A GAN-stage checkpoint (engines/base_gan.py: ``model.model_g.<k>`` / ``model.model_d.<k>``, or bare ``model_g.`` / ``model_d.``)
    -> its ``part`` ("model_g." / "model_d.") keys as ``prefix + <k>``; any other state dict is returned as it is."""
    if not any(k.startswith(("model.model_g.", "model_g.", "model.model_d.", "model_d.")) for k in sd):
        return sd
    out = {}
    for k, v in sd.items():
        bare = k[len("model."):] if k.startswith("model.model_") else k
        if bare.startswith(part):
            out[prefix + bare[len(part):]] = v
    return out


def load_discriminator_checkpoint(model_d, path_or_obj, strict: bool = True):
    """The ``model_d.`` keys of a GAN-stage checkpoint (the reference's ``bsr_discriminator_checkpoint``, engines/base_gan.py:71-84, or
    one written by ``train --gan``) into a ``discriminator.UNetDiscriminatorSN``; a bare discriminator state dict loads as it is."""
    obj = torch.load(path_or_obj, map_location="cpu") if isinstance(path_or_obj, (str, os.PathLike)) else path_or_obj
    return model_d.load_state_dict(_gan_part(extract_state_dict(obj), "model_d.", ""), strict=strict)


# ---- metric (restated here: the product does not depend on the test infrastructure) -------------------------------
def tensor_round(img: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """utils/utils_image.py:30-33 (out of place)."""
    return (img.clamp(0.0, data_range) * 255.0 / data_range).round() * data_range / 255.0


def shave(img: torch.Tensor, border: int) -> torch.Tensor:
    """utils/utils_image.py:8-11."""
    return img[..., border:-border, border:-border] if border > 0 else img


def rgb_to_y(img: torch.Tensor) -> torch.Tensor:
    """Y channel of matlab ``rgb2ycbcr`` for float RGB in [0, 1] (utils/utils_image.py:43-79): (B,1,H,W) in [0,1]."""
    w = torch.tensor([65.481, 128.553, 24.966], dtype=img.dtype, device=img.device) / 255.0
    y = (img * 255.0).permute(0, 2, 3, 1) @ w + 16.0
    return (y.round() / 255.0).unsqueeze(1)


def psnr_y(restored: torch.Tensor, target: torch.Tensor, scale: int = 1) -> torch.Tensor:
    """PSNR-Y as the reference's validation step computes it (engines/base.py:256-268, utils/metrics/psnr.py:44-48):
    quantise the output to 8 bit, shave ``scale`` pixels for SR, compare the Y channels.  Grey inputs are compared as is."""
    border = scale if scale > 1 else 0
    out, tgt = shave(tensor_round(restored.float()), border), shave(target.float(), border)
    if out.shape[1] == 3:
        out, tgt = rgb_to_y(out), rgb_to_y(tgt)
    return -10.0 * (out - tgt).pow(2).mean(dim=(-3, -2, -1)).log10()


# ---- folder evaluation ---------------------------------------------------------------------------------------------
_IMG_EXT = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")


def _read_image(path: str, mode: str = "RGB") -> torch.Tensor:
    """(1, C, H, W) fp32 in [0, 1]; ``mode`` "RGB" (C = 3) or "L" (C = 1, the grayscale checkpoints)."""
    import numpy as np
    from PIL import Image

    a = np.asarray(Image.open(path).convert(mode), dtype=np.float32) / 255.0
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(a).permute(2, 0, 1).unsqueeze(0).contiguous()


def _list_images(folder: str) -> List[str]:
    return sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.lower().endswith(_IMG_EXT))


def image_pairs(lq_dir: str, gt_dir: str) -> List[Tuple[str, str]]:
    """(lq, gt) paths matched by sorted order of the image files in the two folders (the dataset classes pair the same way,
    data/datasets/restoration_sr.py:134-141)."""
    lq, gt = _list_images(lq_dir), _list_images(gt_dir)
    if len(lq) != len(gt) or not lq:
        raise ValueError(f"{lq_dir}: {len(lq)} images, {gt_dir}: {len(gt)} images")
    return list(zip(lq, gt))


def image_triples(lq_dir: str, lq_r_dir: str, gt_dir: str) -> List[Tuple[str, str, str]]:
    """(left view, right view, gt) paths of a dual-pixel set, matched by sorted order like ``image_pairs`` (the reference lists
    the three folders the same way, data/datasets/restoration_paired_dataset.py)."""
    lq, lq_r, gt = _list_images(lq_dir), _list_images(lq_r_dir), _list_images(gt_dir)
    if not (len(lq) == len(lq_r) == len(gt)) or not lq:
        raise ValueError(f"{lq_dir}: {len(lq)} images, {lq_r_dir}: {len(lq_r)} images, {gt_dir}: {len(gt)} images")
    return list(zip(lq, lq_r, gt))


def _side_by_side(left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
    """The model input of a dual-pixel pair: ``torch.cat([img_lq_l, img_lq_r], dim=1)`` (engines/base.py:119-120)."""
    if left.shape != right.shape:
        raise ValueError(f"dual-pixel views differ in size: {tuple(left.shape[-2:])} (left) and {tuple(right.shape[-2:])} (right)")
    return torch.cat([left, right], dim=1)


@torch.no_grad()
def evaluate_pairs(model, pairs: Iterable[Tuple[torch.Tensor, torch.Tensor]], scale: int, tile: int = 0, overlap: int = 32,
                   device: str = "cuda:0", metric_group: Optional[str] = None, niqe_params=None, on_result=None, lpips_model=None,
                   self_ensemble: bool = False, blend: str = "uniform"):
    """PSNR-Y of ``model`` on (lq, gt) tensors in [0, 1], (1,3,h,w) / (1,3,h*scale,w*scale): a list, one value per pair.
    ``tile > 0`` uses the reference's tiled inference (engines/base.py:90-116) through ``tiling.forward_tiled``.
    With ``metric_group`` (a key of ``metrics.ALL_GROUPS`` or ``metrics.PERCEPTUAL_GROUPS``): {metric name: mean over the pairs} of
    that group instead.  ``gt`` may be None for the group "restorer_niqe", which scores the output alone against ``niqe_params``;
    "restorer_perceptual" takes ``lpips_model`` (an ``lpips.LPIPS`` on ``device``) alongside ``niqe_params``.  ``on_result(index, lq, sr, gt)`` is
    called for every pair with the tensors on ``device``, after ``sr`` and ``gt`` were cropped to each other and before the metrics:
    the images the reference saves (engines/base.py:259-264, before ``shave``).  ``self_ensemble``: every forward is the x8
    geometric self-ensemble of ``ensemble.SelfEnsemble`` -- of the whole image, or with ``tile`` of every tile on its own.
    ``blend``: how tiled inference mixes overlapping tiles (``tiling.BLENDS``; "uniform" is the reference's average)."""
    from . import tiling
    from .metrics import image_metrics

    if self_ensemble:
        from .ensemble import SelfEnsemble

        model = SelfEnsemble(model)

    out = []
    for index, (lq, gt) in enumerate(pairs):
        lq = lq.to(device)
        if tile and tile < min(lq.shape[-2:]):
            sr = tiling.forward_tiled(model, lq, tile, overlap, scale, out_channels=getattr(model, "out_channels", None), blend=blend)
        else:
            sr = model(lq)
        if gt is None:
            if metric_group != "restorer_niqe":
                raise ValueError(f"metric group {metric_group!r} needs a ground truth; without one only restorer_niqe can be scored")
        else:
            gt = gt.to(sr.device)[..., : sr.shape[-2], : sr.shape[-1]]
            sr = sr[..., : gt.shape[-2], : gt.shape[-1]]
        if on_result is not None:
            on_result(index, lq, sr, gt)
        if metric_group is None:
            out.append(float(psnr_y(sr, gt, scale)))
        else:
            out.append({k: float(v.mean()) for k, v in image_metrics(sr, gt, metric_group, scale, niqe_params, lpips_model).items()})
    if metric_group is None:
        return out
    return {k: sum(o[k] for o in out) / len(out) for k in out[0]}


def gt_images(gt_dir: str) -> List[str]:
    """The image files of a GT folder, sorted (the same listing as ``image_pairs``)."""
    paths = _list_images(gt_dir)
    if not paths:
        raise ValueError(f"{gt_dir}: no images")
    return paths


def task_inputs(gt_dir: str, task: str, channels: int = 3, sigma: Optional[float] = None, noise_prefix: Optional[str] = None,
                device: str = "cuda:0", scale: int = 1, taps: Optional[torch.Tensor] = None, quality: Optional[int] = None):
    """(file name, LQ, GT) for every image of ``gt_dir`` under a task that synthesises its input, as the reference's validation sets
    do: the GT read as 8 bit, cropped as the task's rule says (``task_rules.RULES``: to multiples of 8, of ``scale``, or not at all),
    and the LQ made by ``tasks.VAL_LQ[task]`` on ``device``.  "dn" keys its noise by ``noise_prefix/<file name>``: the reference's
    test-set name, by default the folder's base name matched to it case-insensitively by ``tasks.dn_test_set_name``, and the path
    that the set's test.json lists.  "db" blurs with ``taps`` (``tasks.blur_taps``; default: the Gaussian's) and adds noise at
    ``sigma`` (default 2); "jpeg" compresses at ``quality``; "sr_bicubic" downscales by ``scale``."""
    from . import tasks

    o = resolve(task, "task_inputs", scale=scale, channels=channels, sigma=sigma, quality=quality)
    if o.rule.taps:
        o.taps = (tasks.blur_taps(tasks.gaussian_blur_kernel()) if taps is None else taps).to(device)
    o.noise_prefix = tasks.dn_test_set_name(os.path.basename(os.path.normpath(gt_dir))) if noise_prefix is None else noise_prefix
    crop = int(o.scale) if o.rule.crop == "scale" else o.rule.crop
    mode = "L" if channels == 1 else "RGB"
    for p in gt_images(gt_dir):
        name = os.path.relpath(p, gt_dir)
        gt = _read_image(p, mode)
        if crop:
            gt = tasks.modcrop(gt, crop).contiguous()
        yield name, tasks.VAL_LQ[task](gt, name, o, device), gt


def evaluate_folder(model, lq_dir: Optional[str], gt_dir: Optional[str], scale: int, tile: int = 0, overlap: int = 32,
                    device: str = "cuda:0", verbose: bool = True, metric_group: Optional[str] = None, channels: int = 3,
                    task: str = "sr", sigma: Optional[float] = None, noise_prefix: Optional[str] = None, niqe_params=None,
                    taps: Optional[torch.Tensor] = None, quality: Optional[int] = None, save_dir: Optional[str] = None,
                    save_gt: bool = False, save_workers: int = 4, usm_gt: bool = False, lpips_model=None,
                    lq_r_dir: Optional[str] = None, self_ensemble: bool = False, blend: str = "uniform"):
    """Mean PSNR-Y over the image pairs of two folders; with ``metric_group``, {metric name: mean} of that group.  ``channels`` 1
    reads the images as grayscale.  A ``task`` that synthesises its input ignores ``lq_dir`` and builds the LQ from the GT
    (``task_inputs``, with ``sigma``, ``taps``, ``quality`` and ``scale`` as the task's rule takes them).  A task without a ground
    truth ("bsr") reads ``lq_dir`` alone (``gt_dir`` is not used) and returns {"val_niqe": mean}; ``niqe_params`` is the pristine
    model of ``metrics.niqe`` (also for "restorer_niqe" elsewhere, and for "restorer_perceptual", which takes ``lpips_model`` -- an
    ``lpips.LPIPS``, moved to ``device`` here -- as well).  With ``save_dir`` every image is also written as 8-bit PNG under
    the reference's layout (``image8.save_paths``): ``<stem>_HQ.png`` the restored image, ``<stem>_LQ.png`` the model's input
    (enlarged ``scale`` times by replication, as the reference saves it), and with ``save_gt`` ``<stem>_GT.png``; the files are complete
    when the call returns.  The metrics do not depend on it.  ``usm_gt`` (task "sr" only; ValueError elsewhere): every GT is cropped
    to a multiple of ``scale`` and sharpened by ``tasks.usm_sharp(..., quantise=True)`` on ``device`` before anything else sees it,
    as the reference's validation set does under ``use_usm`` (restoration_sr.py:94,105-109, base_image.py:404): the metrics are
    taken against the sharpened GT and ``save_gt`` writes it.  ``lq_r_dir`` (task "sr" at scale 1, RGB): dual-pixel defocus
    deblurring -- ``lq_dir`` holds the left views, ``lq_r_dir`` the right ones, matched to each other and to the GT by sorted order;
    the model (``GRL(in_channels=6, out_channels=3)``) gets the two side by side, ``<stem>_LQ.png`` is the LEFT view
    (engines/base.py:536-537) and the saved images go straight under the data set's name (engines/base.py:521-524).
    ``self_ensemble``: the model runs as ``ensemble.SelfEnsemble(model)``, the x8 geometric self-ensemble (per tile with ``tile``); it
    sits at the model boundary, after the task's front end, so every task, metric and saved image goes with it.  ``blend`` (with
    ``tile``; ValueError without): "linear" or "cosine" feathers the overlaps of tiled inference instead of averaging them uniformly."""
    from . import tiling

    if blend not in tiling.BLENDS:
        raise ValueError(f"blend is one of {', '.join(tiling.BLENDS)}, got {blend!r}")
    if blend != "uniform" and not tile:
        raise ValueError("blend belongs to tiled inference: give a tile size")
    if self_ensemble:
        from .ensemble import SelfEnsemble

        model = SelfEnsemble(model)
    dual = lq_r_dir is not None
    o = resolve(task, "evaluate_folder", scale=scale, channels=channels, sigma=sigma, quality=quality, usm=usm_gt,
                **(dict(dual_pixel=True, lq=lq_dir is not None) if dual else {}))
    rule = o.rule
    mode = "L" if channels == 1 else "RGB"
    if rule.lq_from == "gt":
        items = task_inputs(gt_dir, task, channels, sigma, noise_prefix, device, scale, taps, quality)
    elif dual:
        items = ((os.path.basename(l_p), _side_by_side(_read_image(l_p, mode), _read_image(r_p, mode)), _read_image(gt_p, mode))
                 for l_p, r_p, gt_p in image_triples(lq_dir, lq_r_dir, gt_dir))
    elif rule.has_gt:
        items = ((os.path.basename(lq_p), _read_image(lq_p, mode), _read_image(gt_p, mode)) for lq_p, gt_p in image_pairs(lq_dir, gt_dir))
        if usm_gt:
            from . import tasks

            items = ((name, lq, tasks.usm_sharp(tasks.modcrop(gt, int(scale)).contiguous().to(device), quantise=True))
                     for name, lq, gt in items)
    else:
        if metric_group not in (None, "restorer_niqe"):
            raise ValueError(f"task {task} has no ground truth: its metric group is restorer_niqe, not {metric_group!r}")
        metric_group = "restorer_niqe"
        items = ((os.path.relpath(p, lq_dir), _read_image(p, mode), None) for p in gt_images(lq_dir))
    if lpips_model is not None:
        lpips_model = lpips_model.to(device)
    vals, writer, save = [], contextlib.nullcontext(), None
    if save_dir is not None:
        from .image8 import ImageWriter, save_paths

        dataset = os.path.basename(os.path.normpath(gt_dir if rule.has_gt else lq_dir))
        writer = ImageWriter(save_workers)

        def save(name, lq, sr, gt):
            paths = save_paths(save_dir, task, name, scale, o.sigma, o.quality, dataset, flat=dual)
            os.makedirs(os.path.dirname(paths["HQ"]), exist_ok=True)
            writer.write(paths["HQ"], sr.float())
            writer.write(paths["LQ"], lq[:, :3] if dual else lq, rep=scale)
            if save_gt and gt is not None:
                writer.write(paths["GT"], gt)
    with writer:                                          # closed, every file in place, before the mean is returned
        for name, lq, gt in items:
            on_result = None if save is None else (lambda i, lq_, sr_, gt_, name=name: save(name, lq_, sr_, gt_))
            v = evaluate_pairs(model, [(lq, gt)], scale, tile, overlap, device, metric_group, niqe_params, on_result, lpips_model,
                               blend=blend)
            v = v[0] if metric_group is None else v
            vals.append(v)
            if verbose:
                print(f"{name:32s} {_columns(v)}")
    if metric_group is None:
        mean = sum(vals) / len(vals)
    else:
        mean = {k: sum(v[k] for v in vals) / len(vals) for k in vals[0]}
    if verbose:
        print(f"{'mean over ' + str(len(vals)) + ' images':32s} {_columns(mean)}")
    return mean


def _columns(v) -> str:
    if not isinstance(v, dict):
        return f"PSNR-Y {v:7.3f} dB"
    return "  ".join(f"{k} {x:7.4f}" if "ssim" in k else f"{k} {x:7.3f}" for k, x in v.items())


def _parser():
    from .metrics import ALL_GROUPS, PERCEPTUAL_GROUPS

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_task_arguments(ap, TASKS)
    ap.add_argument("--ckpt", default=None, help="reference checkpoint (.ckpt / .pth); random init without it")
    ap.add_argument("--ema", action="store_true",
                    help="load the averaged weights of --ckpt (state_dict_ema of train --ema-decay, or BasicSR's params_ema)")
    ap.add_argument("--lq", default=None, help="LQ folder (--task sr and bsr)")
    ap.add_argument("--lq-r", default=None,
                    help="--task sr --scale 1: folder of the RIGHT sub-aperture views of a dual-pixel set (--lq holds the left ones); the "
                         "model is built with 6 input and 3 output channels (db_defocus_dual_pixel_grl_base.ckpt)")
    ap.add_argument("--gt", default=None, help="GT folder (required, except with --task bsr)")
    ap.add_argument("--niqe-params", default=None,
                    help="restorer_niqe: the reference's utils/metrics/niqe_pris_params.npz (default: the environment variable "
                         "GRL_NIQE_PARAMS)")
    ap.add_argument("--lpips-vgg", default=None, metavar="PATH",
                    help="restorer_perceptual: torchvision's vgg16-397923af.pth, read with torch.load; nothing is downloaded")
    ap.add_argument("--lpips-lin", default=None, metavar="PATH",
                    help="restorer_perceptual: the lpips package's weights/v0.1/vgg.pth (the five 1x1 layers)")
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--blend", default=None, choices=["uniform", "linear", "cosine"],
                    help="with --tile: how overlapping tiles are mixed.  uniform (default): the reference's plain average; linear, "
                         "cosine: a ramp over the overlap that feathers the seams")
    ap.add_argument("--self-ensemble", action="store_true",
                    help="x8 geometric self-ensemble: restore the image under the eight flips and rotations and average the results "
                         "mapped back (with --tile: every tile on its own)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--metric", default=None, choices=sorted(ALL_GROUPS) + sorted(PERCEPTUAL_GROUPS),
                    help="report this metric group of the reference (config/metric/*.yaml) instead of PSNR-Y alone")
    ap.add_argument("--save-dir", default=None,
                    help="also write every restored image (<stem>_HQ.png) and the model's input (<stem>_LQ.png) as 8-bit PNG under "
                         "DIR/X<scale> | Sigma<sigma> | QF<quality>/<data set>/, the reference's layout")
    ap.add_argument("--save-gt", action="store_true", help="with --save-dir: also write <stem>_GT.png")
    ap.add_argument("--usm-gt", action="store_true",
                    help="--task sr: score against the USM-sharpened GT (the reference's val.use_usm: True of bsr/grl_psnr.yaml); the "
                         "GT is cropped to a multiple of --scale first, and --save-gt writes the sharpened image")
    ap.add_argument("--noise-prefix", default=None,
                    help="--task dn: the reference's test-set name (Set12, BSD68, CBSD68, Kodak24, McMaster, Urban100; case matters) "
                         "that starts the noise seed key '<prefix>/<file name>'; a different prefix draws different noise.  Default: "
                         "the --gt folder's name, matched case-insensitively to one of those")
    return ap


def check_blend(ap, a):
    """--blend (evaluate and restore) belongs to --tile; fills the default."""
    if a.blend is not None and not a.tile:
        ap.error("--blend belongs to tiled inference: give --tile")
    a.blend = a.blend or "uniform"


def _check(ap, a):
    """Checks the parsed arguments against the task's rule and fills ``a.scale``, ``a.sigma`` and, without a ground truth,
    ``a.metric``."""
    if RULES[a.task].has_gt:
        if a.gt is None:
            ap.error("the following arguments are required: --gt")
    else:
        if a.gt is not None:
            ap.error(f"--task {a.task} has no ground truth; --gt is not used")
        if a.metric not in (None, "restorer_niqe"):
            ap.error(f"--task {a.task} is scored by --metric restorer_niqe")
        a.metric = "restorer_niqe"
    check_blend(ap, a)
    o = resolve_arguments(ap, a, "evaluate", usm=a.usm_gt, dual_pixel=a.lq_r is not None)
    a.scale, a.sigma = o.scale, o.sigma


def load_lpips_arguments(ap, a, needed_by=None):
    """The ``lpips.LPIPS`` that ``--metric restorer_perceptual`` needs, from ``--lpips-vgg`` and ``--lpips-lin`` (evaluate and train);
    None for every other group -- unless ``needed_by`` names another option that takes the model (train's ``--lpips-weight``).  A
    missing option, file or key ends through ``ap.error``."""
    if a.metric != "restorer_perceptual" and needed_by is None:
        if a.lpips_vgg is not None or a.lpips_lin is not None:
            ap.error("--lpips-vgg and --lpips-lin belong to --metric restorer_perceptual")
        return None
    for opt, path in (("--lpips-vgg", a.lpips_vgg), ("--lpips-lin", a.lpips_lin)):
        if path is None:
            ap.error(f"{needed_by or '--metric restorer_perceptual'} needs {opt} (torchvision's vgg16-397923af.pth / the lpips package's vgg.pth)")
        if not os.path.isfile(path):
            ap.error(f"{opt}: file {path!r} not found")
    from .lpips import load_lpips

    try:
        return load_lpips(a.lpips_vgg, a.lpips_lin)
    except (KeyError, ValueError) as e:
        ap.error(f"--lpips-vgg / --lpips-lin: {e}")


def main(argv: Optional[List[str]] = None):
    from . import GRL, make_config

    ap = _parser()
    a = ap.parse_args(argv)
    _check(ap, a)
    taps = load_taps(ap, a)
    niqe_params, lpips_model = None, load_lpips_arguments(ap, a)
    if a.metric in ("restorer_niqe", "restorer_perceptual"):
        from .metrics import load_niqe_params

        try:
            niqe_params = load_niqe_params(a.niqe_params)
        except ValueError as e:
            ap.error(str(e))
    overrides = {"upsampler": a.upsampler} if a.upsampler and a.scale > 1 else {}
    # two views side by side: GRL(in_channels=6, out_channels=3) of db_defocus/grl_dual_p480
    channels = dict(in_channels=6, out_channels=3) if a.lq_r is not None else dict(in_channels=a.channels)
    model = GRL(**make_config(a.model, a.geometry, upscale=a.scale, **channels, **overrides)).eval()
    if a.ema and not a.ckpt:
        ap.error("--ema belongs to --ckpt")
    if a.ckpt:
        try:
            load_checkpoint(model, a.ckpt, ema=a.ema)
        except KeyError as e:
            ap.error(f"--ema: {e.args[0]}")
    model = model.to(a.device)
    return evaluate_folder(model, a.lq, a.gt, a.scale, a.tile, a.overlap, a.device, metric_group=a.metric, channels=a.channels,
                           task=a.task, sigma=a.sigma, noise_prefix=a.noise_prefix, niqe_params=niqe_params, taps=taps,
                           quality=a.quality, save_dir=a.save_dir, save_gt=a.save_gt, usm_gt=a.usm_gt, lpips_model=lpips_model,
                           lq_r_dir=a.lq_r, self_ensemble=a.self_ensemble, blend=a.blend)


if __name__ == "__main__":
    main()
