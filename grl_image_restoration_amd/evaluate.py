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
  task "dn" / "dm"  the tasks whose LQ the reference builds from the GT (``task_inputs``): the GT is cropped to multiples of 8
                    (data/datasets/base_image.py:419-425); denoising adds the reference's seeded validation noise
                    (restoration_dn.py:133-143), demosaicking mosaics the GT and demosaics it with ``dm_matlab`` on the device
                    (restoration_dm.py:25-35, engines/base.py:126-128), the whole image before any tiling
  task "sr_bicubic" classical SR scored from the GT folder alone: the GT is cropped to a multiple of the scale and the LQ is its
                    MATLAB-bicubic downscale, 8-bit quantised (``tasks.sr_lq``; restoration_sr.py:130-141,
                    utils/matlab_functions.py:91-188), made on the device
  task "db"         non-blind deblurring (config/data_module/db.yaml): the GT cropped to multiples of 8 and blurred on the device with
                    the Gaussian or a Levin09 kernel, zero padded (``tasks.db_lq``, one ``grl_blur_depthwise`` launch;
                    engines/base.py:131-139), plus the data set's noise at sigma 2, seeded 0 for every image (restoration_db.py:40-43)
  task "jpeg"       JPEG artifact removal (config/data_module/jpeg.yaml): the GT, NOT cropped (the validation branch samples at scale 1,
                    base_image.py:403-404), compressed and decompressed on the device at ``quality`` (``tasks.jpeg_roundtrip``:
                    libjpeg's arithmetic bit for bit; data/datasets/restoration_jpeg.py:62-79)
  task "bsr"        blind / real-world SR (config/experiment/bsr/grl.yaml): LQ images only, no GT (``with_gt: False``); the metric is
                    NIQE of the output (``metrics.niqe``, config/metric/restorer_niqe.yaml), against the pristine model the user
                    names with ``--niqe-params`` or the environment variable GRL_NIQE_PARAMS

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
"""
import argparse
import os
from typing import Dict, Iterable, List, Optional, Tuple

import torch

_METRIC_KEYS = ("current_val_metric", "best_val_metric", "best_iter")


def extract_state_dict(obj: Dict) -> Dict[str, torch.Tensor]:
    """The parameter dictionary inside whatever ``torch.load`` returned (tools/trainer.py:97-104): a Lightning checkpoint
    (``state_dict`` with ``model.`` prefixes and the trainer's metric entries), a BasicSR-style ``params`` dictionary,
    or already a plain state dict."""
    sd = obj
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = dict(sd["state_dict"])
        for k in _METRIC_KEYS:
            sd.pop(k, None)
    if isinstance(sd, dict) and "params" in sd:
        sd = sd["params"]
    if not isinstance(sd, dict):
        raise TypeError(f"not a checkpoint dictionary: {type(obj).__name__}")
    return sd


def load_checkpoint(model, path_or_obj, strict: bool = True):
    """Load a reference checkpoint into ``model`` (a ``grl_image_restoration_amd.GRL``).  Mirrors tools/trainer.py:93-115:
    geometry buffers (``table_*/index_*/mask_*``, ``relative_*``, ``attn_mask``) are dropped, the Lightning module prefix
    ``model.`` is removed, and -- as trainer.py:106-108 does -- the checkpoint is merged INTO the module's current state before
    the strict load: a partial checkpoint keeps the current values of the keys it lacks, an unknown key still fails.
    (The other direction: ``GRL.state_dict()`` has no ``table_/index_/mask_`` buffers, so loading it into the reference module
    needs ``strict=False`` or the reference's own buffers merged in the same way.)"""
    obj = torch.load(path_or_obj, map_location="cpu") if isinstance(path_or_obj, (str, os.PathLike)) else path_or_obj
    sd = extract_state_dict(obj)
    sd = model.convert_checkpoint(dict(sd))           # needs the un-stripped "model.table_*" names (grl.py:556-569)
    sd = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}
    cur = dict(model.state_dict())
    cur.update(sd)
    return model.load_state_dict(cur, strict=strict)


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


def image_pairs(lq_dir: str, gt_dir: str) -> List[Tuple[str, str]]:
    """(lq, gt) paths matched by sorted order of the image files in the two folders (the dataset classes pair the same way,
    data/datasets/restoration_sr.py:134-141)."""
    ls = lambda d: sorted(os.path.join(d, f) for f in os.listdir(d) if f.lower().endswith(_IMG_EXT))
    lq, gt = ls(lq_dir), ls(gt_dir)
    if len(lq) != len(gt) or not lq:
        raise ValueError(f"{lq_dir}: {len(lq)} images, {gt_dir}: {len(gt)} images")
    return list(zip(lq, gt))


@torch.no_grad()
def evaluate_pairs(model, pairs: Iterable[Tuple[torch.Tensor, torch.Tensor]], scale: int, tile: int = 0, overlap: int = 32,
                   device: str = "cuda:0", metric_group: Optional[str] = None, niqe_params=None):
    """PSNR-Y of ``model`` on (lq, gt) tensors in [0, 1], (1,3,h,w) / (1,3,h*scale,w*scale): a list, one value per pair.
    ``tile > 0`` uses the reference's tiled inference (engines/base.py:90-116) through ``tiling.forward_tiled``.
    With ``metric_group`` (a key of ``metrics.ALL_GROUPS``): {metric name: mean over the pairs} of that group instead.  ``gt`` may be
    None for the group "restorer_niqe", which scores the output alone against ``niqe_params``."""
    from . import tiling
    from .metrics import image_metrics

    out = []
    for lq, gt in pairs:
        lq = lq.to(device)
        if tile and tile < min(lq.shape[-2:]):
            sr = tiling.forward_tiled(model, lq, tile, overlap, scale)
        else:
            sr = model(lq)
        if gt is None:
            if metric_group != "restorer_niqe":
                raise ValueError(f"metric group {metric_group!r} needs a ground truth; without one only restorer_niqe can be scored")
        else:
            gt = gt.to(sr.device)[..., : sr.shape[-2], : sr.shape[-1]]
            sr = sr[..., : gt.shape[-2], : gt.shape[-1]]
        if metric_group is None:
            out.append(float(psnr_y(sr, gt, scale)))
        else:
            out.append({k: float(v.mean()) for k, v in image_metrics(sr, gt, metric_group, scale, niqe_params).items()})
    if metric_group is None:
        return out
    return {k: sum(o[k] for o in out) / len(out) for k in out[0]}


TASKS = ("sr", "dn", "dm", "sr_bicubic", "bsr", "db", "jpeg")


def gt_images(gt_dir: str) -> List[str]:
    """The image files of a GT folder, sorted (the same listing as ``image_pairs``)."""
    paths = sorted(os.path.join(gt_dir, f) for f in os.listdir(gt_dir) if f.lower().endswith(_IMG_EXT))
    if not paths:
        raise ValueError(f"{gt_dir}: no images")
    return paths


def task_inputs(gt_dir: str, task: str, channels: int = 3, sigma: Optional[float] = None, noise_prefix: Optional[str] = None,
                device: str = "cuda:0", scale: int = 1, taps: Optional[torch.Tensor] = None, quality: Optional[int] = None):
    """(file name, LQ, GT) for every image of ``gt_dir`` under a task that synthesises its input ("dn", "dm", "sr_bicubic", "db" or "jpeg"), as the reference's
    validation sets do: GT read as 8 bit and cropped to multiples of 8; "dn" adds ``tasks.dn_noise`` at ``sigma`` (keyed by
    ``noise_prefix/<file name>``: the reference's test-set name, by default the folder's base name matched to it case-insensitively by
    ``tasks.dn_test_set_name``, and the path that the set's test.json lists; on the CPU, in fp32, as the data set does), "dm"
    runs ``tasks.demosaic_gt`` on ``device`` (RGB only).  "sr_bicubic" crops the GT to a multiple of ``scale`` instead (the
    reference's ``modcrop(img_gt, self.scale)``, restoration_sr.py:130) and makes the LQ with ``tasks.sr_lq`` on ``device``.
    "db" (RGB only) blurs the GT on ``device`` with ``taps`` (``tasks.blur_taps``; default: the Gaussian's) and adds
    ``tasks.db_noise`` at ``sigma`` (default 2), made on the CPU and added by the blur kernel.  "jpeg" leaves the GT uncropped
    and makes the LQ with ``tasks.jpeg_roundtrip`` at ``quality`` on ``device``."""
    from . import tasks

    if task not in ("dn", "dm", "sr_bicubic", "db", "jpeg"):
        raise ValueError(f"task {task!r} reads its LQ from a folder; synthesised tasks: dn, dm, sr_bicubic, db, jpeg")
    if task == "jpeg" and (quality is None or not 1 <= int(quality) <= 100):
        raise ValueError(f"task jpeg needs a quality of 1 .. 100, got {quality}")
    if task == "sr_bicubic" and int(scale) < 2:
        raise ValueError(f"task sr_bicubic needs a scale above 1, got {scale}")
    if task == "dn" and sigma is None:
        raise ValueError("task dn needs a noise sigma")
    if task in ("dm", "db") and channels != 3:
        raise ValueError(f"task {task} works on RGB images")
    if task == "db":
        if taps is None:
            taps = tasks.blur_taps(tasks.gaussian_blur_kernel())
        taps = taps.to(device)
        sigma = 2.0 if sigma is None else sigma
    if noise_prefix is None:
        noise_prefix = tasks.dn_test_set_name(os.path.basename(os.path.normpath(gt_dir)))
    mode = "L" if channels == 1 else "RGB"
    for p in gt_images(gt_dir):
        name = os.path.relpath(p, gt_dir)
        if task == "sr_bicubic":
            gt = tasks.modcrop(_read_image(p, mode), int(scale)).contiguous()
            yield name, tasks.sr_lq(gt.to(device), int(scale))[0], gt
            continue
        if task == "jpeg":
            gt = _read_image(p, mode)
            yield name, tasks.jpeg_roundtrip(gt.to(device), int(quality)), gt
            continue
        gt = tasks.modcrop(_read_image(p, mode), 8).contiguous()
        if task == "dn":
            noise = tasks.dn_noise(gt.shape[1:], sigma, tasks.dn_noise_key(f"{noise_prefix}/{name}"))
            lq = gt + noise.unsqueeze(0)
        elif task == "db":
            lq = tasks.db_lq(gt.to(device), taps, tasks.db_noise(gt.shape[1:], sigma).unsqueeze(0).to(device))
        else:
            lq = tasks.demosaic_gt(gt.to(device))
        yield name, lq, gt


def evaluate_folder(model, lq_dir: Optional[str], gt_dir: Optional[str], scale: int, tile: int = 0, overlap: int = 32,
                    device: str = "cuda:0", verbose: bool = True, metric_group: Optional[str] = None, channels: int = 3,
                    task: str = "sr", sigma: Optional[float] = None, noise_prefix: Optional[str] = None, niqe_params=None,
                    taps: Optional[torch.Tensor] = None, quality: Optional[int] = None):
    """Mean PSNR-Y over the image pairs of two folders; with ``metric_group``, {metric name: mean} of that group.  ``channels`` 1
    reads the images as grayscale.  ``task`` "dn" / "dm" / "db" / "jpeg" ignores ``lq_dir`` and builds the LQ from the GT (``task_inputs``;
    ``scale`` must be 1; ``taps``: the blur taps of "db", the Gaussian's by default; ``quality``: the JPEG quality of "jpeg"); so does "sr_bicubic", at a ``scale`` above 1.  ``task`` "bsr" reads ``lq_dir`` alone (``gt_dir`` is not used)
    and returns {"val_niqe": mean}; ``niqe_params`` is the pristine model of ``metrics.niqe`` (also for "restorer_niqe" elsewhere)."""
    if task not in TASKS:
        raise ValueError(f"unknown task {task!r}: one of {TASKS}")
    mode = "L" if channels == 1 else "RGB"
    if task == "sr":
        items = ((os.path.basename(lq_p), _read_image(lq_p, mode), _read_image(gt_p, mode)) for lq_p, gt_p in image_pairs(lq_dir, gt_dir))
    elif task == "bsr":
        if metric_group not in (None, "restorer_niqe"):
            raise ValueError(f"task bsr has no ground truth: its metric group is restorer_niqe, not {metric_group!r}")
        metric_group = "restorer_niqe"
        items = ((os.path.relpath(p, lq_dir), _read_image(p, mode), None) for p in gt_images(lq_dir))
    elif task == "sr_bicubic":
        items = task_inputs(gt_dir, task, channels, device=device, scale=scale)
    else:
        if scale != 1:
            raise ValueError(f"task {task} restores at scale 1, got {scale}")
        items = task_inputs(gt_dir, task, channels, sigma, noise_prefix, device, taps=taps, quality=quality)
    vals = []
    for name, lq, gt in items:
        v = evaluate_pairs(model, [(lq, gt)], scale, tile, overlap, device, metric_group, niqe_params)
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


def main(argv: Optional[List[str]] = None):
    from . import GRL, make_config
    from .metrics import ALL_GROUPS

    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="base", choices=["tiny", "small", "base"])
    ap.add_argument("--geometry", default="sr_ckpt_df2", help="a key of presets.GEOMETRIES")
    ap.add_argument("--task", default="sr", choices=TASKS,
                    help="sr: LQ images from --lq (SR, deblurring, JPEG); dn / dm / sr_bicubic / db / jpeg: the LQ is made from --gt (denoising, "
                         "demosaicking, classical SR by MATLAB-bicubic downscaling at --scale, non-blind deblurring, JPEG compression at "
                         "--quality); bsr: LQ images from --lq, no --gt, "
                         "scored by NIQE")
    ap.add_argument("--scale", type=int, default=None, help="4 by default for --task sr / sr_bicubic / bsr; 1 for everything else")
    ap.add_argument("--upsampler", default=None, choices=["pixelshuffle", "pixelshuffledirect", "nearest+conv"],
                    help="the reconstruction tail; default: the model size's classical-SR tail (bsr_grl_base.ckpt: nearest+conv)")
    ap.add_argument("--ckpt", default=None, help="reference checkpoint (.ckpt / .pth); random init without it")
    ap.add_argument("--lq", default=None, help="LQ folder (--task sr and bsr)")
    ap.add_argument("--gt", default=None, help="GT folder (required, except with --task bsr)")
    ap.add_argument("--niqe-params", default=None,
                    help="restorer_niqe: the reference's utils/metrics/niqe_pris_params.npz (default: the environment variable "
                         "GRL_NIQE_PARAMS)")
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--metric", default=None, choices=sorted(ALL_GROUPS),
                    help="report this metric group of the reference (config/metric/*.yaml) instead of PSNR-Y alone")
    ap.add_argument("--channels", type=int, default=3, choices=[1, 3], help="1: grayscale model and images (dn_*_c1, jpeg_*_c1)")
    ap.add_argument("--sigma", type=float, default=None, help="--task dn: noise level on the 0..255 scale (15, 25, 50); --task db: the same, default 2")
    ap.add_argument("--blur-kernel", default="gaussian",
                    help="--task db: gaussian (25 x 25, sigma 1.6) or real1 .. real8 (the Levin09 motion kernels, from --blur-kernel-file)")
    ap.add_argument("--blur-kernel-file", default=None,
                    help="--task db with real1 .. real8: the reference's utils/blur_kernels/Levin09.npy, or a 2-D .npy of that kernel")
    ap.add_argument("--quality", type=int, default=None, help="--task jpeg: the JPEG quality factor, 1 .. 100 (10, 20, 30, 40)")
    ap.add_argument("--noise-prefix", default=None,
                    help="--task dn: the reference's test-set name (Set12, BSD68, CBSD68, Kodak24, McMaster, Urban100; case matters) "
                         "that starts the noise seed key '<prefix>/<file name>'; a different prefix draws different noise.  Default: "
                         "the --gt folder's name, matched case-insensitively to one of those")
    a = ap.parse_args(argv)
    if a.task != "bsr" and a.gt is None:
        ap.error("the following arguments are required: --gt")
    if a.task == "bsr":
        if a.lq is None:
            ap.error("--lq is required with --task bsr")
        if a.gt is not None:
            ap.error("--task bsr has no ground truth; --gt is not used")
        if a.metric not in (None, "restorer_niqe"):
            ap.error("--task bsr is scored by --metric restorer_niqe")
        a.metric = "restorer_niqe"
    if a.task == "sr" and a.lq is None:
        ap.error("--lq is required with --task sr")
    if a.task not in ("sr", "bsr") and a.lq is not None:
        ap.error(f"--task {a.task} builds its LQ from --gt; --lq is not used")
    if a.task == "dn" and a.sigma is None:
        ap.error("--task dn needs --sigma")
    if a.scale is None:
        a.scale = 4 if a.task in ("sr", "sr_bicubic", "bsr") else 1
    if a.task in ("dn", "dm", "db", "jpeg") and a.scale != 1:
        ap.error(f"--task {a.task} restores at --scale 1")
    if a.task == "jpeg" and (a.quality is None or not 1 <= a.quality <= 100):
        ap.error("--task jpeg needs --quality, 1 .. 100")
    if a.task != "jpeg" and a.quality is not None:
        ap.error(f"--quality belongs to --task jpeg, not {a.task}")
    if a.task == "sr_bicubic" and a.scale < 2:
        ap.error("--task sr_bicubic needs a --scale above 1")
    taps = None
    if a.task == "db":
        from . import tasks

        if a.channels != 3:
            ap.error("--task db works on RGB images")
        try:
            taps = tasks.blur_taps(tasks.load_blur_kernel(a.blur_kernel, a.blur_kernel_file))
        except (ValueError, OSError) as e:
            ap.error(f"--blur-kernel: {e}")
        if a.sigma is None:
            a.sigma = 2.0
    elif a.blur_kernel != "gaussian" or a.blur_kernel_file is not None:
        ap.error(f"--blur-kernel / --blur-kernel-file belong to --task db, not {a.task}")
    niqe_params = None
    if a.metric == "restorer_niqe":
        from .metrics import load_niqe_params

        try:
            niqe_params = load_niqe_params(a.niqe_params)
        except ValueError as e:
            ap.error(str(e))
    overrides = {"upsampler": a.upsampler} if a.upsampler and a.scale > 1 else {}
    model = GRL(**make_config(a.model, a.geometry, upscale=a.scale, in_channels=a.channels, **overrides)).eval()
    if a.ckpt:
        load_checkpoint(model, a.ckpt)
    model = model.to(a.device)
    return evaluate_folder(model, a.lq, a.gt, a.scale, a.tile, a.overlap, a.device, metric_group=a.metric, channels=a.channels,
                           task=a.task, sigma=a.sigma, noise_prefix=a.noise_prefix, niqe_params=niqe_params, taps=taps,
                           quality=a.quality)


if __name__ == "__main__":
    main()
