"""The rules of the restoration tasks, stated once: what ``evaluate``, ``train`` and ``data.PatchSampler`` accept for a task, what
they default, and where the task's LQ comes from.  ``RULES`` is the table, ``resolve`` checks a set of options against it,
``add_task_arguments`` declares the options both command lines share.  The LQ builders that go with a rule are in ``tasks.py``
(``VAL_LQ``, ``TRAIN_STORE_LQ``, ``TRAIN_PAIR``).  No torch at import time: the argument parsers read this module.
"""
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional


@dataclass(frozen=True)
class TaskRule:
    cite: str                           # where the reference defines the task
    lq_from: str = "gt"                 # "folder": LQ images are read; "gt": the LQ is made from the GT on the device
    has_gt: bool = True                 # False: scored without a ground truth (NIQE)
    trainable: bool = True
    default_scale: int = 1              # what the command lines take without --scale
    min_scale: int = 1
    max_scale: Optional[int] = 1        # 1: the task restores at scale 1
    crop: object = None                 # validation GT crop: 8, "scale" or None (base_image.py:419-425, restoration_sr.py:130)
    rgb_only: bool = False
    even_patch: bool = False            # training patches sit on the 2 x 2 Bayer lattice
    noise: bool = False                 # takes sigma
    sigma_default: Optional[float] = None   # None with ``noise``: sigma is required
    sigma_range: bool = False           # training may draw a sigma per sample
    taps: bool = False                  # takes a blur kernel
    quality: bool = False               # takes a JPEG quality, or for training a quality range
    usm: bool = False                   # the GT may be USM-sharpened (use_usm / use_usm_pixel: restoration_sr.py:94,105-109)
    degrade: bool = False               # training may make its LQ on the fly by the blind-SR degradation (restoration_bsr.py:83-110)
    gan: bool = False                   # training may run the GAN stage against the U-Net discriminator (engines/base_gan.py, bsr/grl.yaml)
    save_tag: Optional[str] = None      # saved images go under X<scale> ("scale"), Sigma<sigma> ("sigma"), QF<quality> ("quality") or
                                        # straight under the data set's name (None): engines/base.py:504-524


RULES = {
    "sr": TaskRule("classical SR from an LQ / GT folder pair (also deblurring and JPEG from folders): config/experiment/sr, "
                   "data/datasets/restoration_sr.py:97-123 with load_lr; USM-sharpened GT: config/experiment/bsr/grl_psnr.yaml:26-33",
                   lq_from="folder", default_scale=4, max_scale=None, usm=True, degrade=True, gan=True, save_tag="scale"),
    "dn": TaskRule("denoising: config/data_module/dn.yaml; training noise restoration_dn.py:126-143, seeded validation noise :133-143",
                   crop=8, noise=True, sigma_range=True, save_tag="sigma"),
    "dm": TaskRule("demosaicking: restoration_dm.py:25-35 (mosaic), engines/base.py:126-128 (dm_matlab before the model)",
                   crop=8, rgb_only=True, even_patch=True),
    "sr_bicubic": TaskRule("classical SR from the GT alone, LQ by MATLAB bicubic: restoration_sr.py:130-141, utils/matlab_functions.py:91-188",
                           default_scale=4, min_scale=2, max_scale=None, crop="scale", save_tag="scale"),
    "bsr": TaskRule("blind / real-world SR, LQ images only, NIQE: config/experiment/bsr/grl.yaml (with_gt: False), "
                    "config/metric/restorer_niqe.yaml", lq_from="folder", has_gt=False, trainable=False, default_scale=4, max_scale=None,
                    save_tag="scale"),
    "db": TaskRule("non-blind deblurring: config/data_module/db.yaml, restoration_db.py:19-21,40-43, engines/base.py:131-142",
                   crop=8, rgb_only=True, noise=True, sigma_default=2.0, taps=True),
    "jpeg": TaskRule("JPEG artifact removal: config/data_module/jpeg.yaml, restoration_jpeg.py:30-46,62-79; validation is not cropped "
                     "(base_image.py:403-404)", quality=True, save_tag="quality"),
}
TASKS = tuple(RULES)
# the order data.TASKS has had since the tasks were added: the SR tasks, then the tasks at scale 1
TRAIN_TASKS = tuple(sorted((t for t in RULES if RULES[t].trainable), key=lambda t: RULES[t].max_scale is not None))
SYNTHESISED = tuple(t for t in RULES if RULES[t].lq_from == "gt")


def resolve(task, where, *, scale=None, channels=3, lq=False, sigma=None, sigma_range=None, taps=False, quality=None,
            quality_range=None, patch=None, patchwise=True, val=False, val_lq=False, usm=False, val_usm=False, degrade=False,
            degrade_crop=None, gan=False, camera=False, jitter=False, dual_pixel=False):
    """Checks the options of one call against ``RULES[task]``, fills the defaults and returns them as a namespace (``rule``,
    ``scale``, ``sigma``, ``sigma_range``, ``quality``, ``quality_range``).  Raises ValueError.  ``where`` is the caller: "evaluate" /
    "train" (the command lines), "evaluate_folder", "task_inputs", "sampler".  ``lq`` / ``taps``: whether an LQ folder or store / a blur
    kernel was given; ``val`` / ``val_lq`` (train): validation is on / has an LQ folder; ``usm`` / ``val_usm``: the GT (of training:
    the targets; of evaluation and of train's validation: the scored GT) is sharpened by ``tasks.usm_sharp``.  Where the callers
    have always differed, the difference is a branch on ``where`` below, marked "kept".  ``degrade`` (training): the LQ is made per
    sample from a ``degrade_crop`` x ``degrade_crop`` GT crop (default 400) by ``bsr_degrade``; then no LQ folder or store is given,
    the scale is 2 or 4, the images have three channels, the crop is a multiple of 4 and at least 4 * scale, and ``patch`` is at
    most crop / scale.  The namespace also carries ``degrade_crop`` (None without ``degrade``).  ``gan`` (train): the GAN stage.
    ``camera`` (training with ``degrade``): stage 2 of the degradation, the camera-noise model, is on (camera profiles were given);
    the crop is then at least 32.  ``jitter`` (training with ``degrade``): the reference's ColorJitter on every GT crop.
    ``dual_pixel``: a second LQ folder or store, the right sub-aperture view, was given (--lq-r, lq_r_store; the reference's paired
    data module with ``dual_pixel: True``, config/data_module/paired.yaml, engines/base.py:119-120): task sr at scale 1 on RGB images
    with an LQ folder or store present, and none of usm, degrade, jitter, camera, gan.  It is an option of task sr, not a task.
    """
    training, library_eval = where in ("train", "sampler"), where in ("evaluate_folder", "task_inputs")
    r = RULES.get(task)
    if r is None or (training and not r.trainable):
        raise ValueError(f"unknown task {task!r}: one of {TRAIN_TASKS if training else TASKS}")
    if where == "task_inputs" and r.lq_from != "gt":
        raise ValueError(f"task {task!r} reads its LQ from a folder; synthesised tasks: {', '.join(SYNTHESISED)}")
    if dual_pixel:
        if task != "sr":
            raise ValueError(f"task {task} takes no right view (--lq-r, lq_r_store): dual-pixel inputs belong to task sr at scale 1")
        if (r.default_scale if scale is None else scale) != 1:
            raise ValueError(f"task sr with a right view (--lq-r, lq_r_store) restores at scale 1 (--scale 1), got "
                             f"{r.default_scale if scale is None else scale}")
        if channels != 3:
            raise ValueError("task sr with a right view (--lq-r, lq_r_store) works on RGB images: the model takes 6 channels and gives 3")
        if not lq:
            raise ValueError("task sr with a right view (--lq-r, lq_r_store) needs the left view as its LQ folder (--lq) or store")
        for on, what in ((usm or val_usm, "USM-sharpened targets (--usm, --usm-gt, --val-usm, usm)"), (degrade, "the on-the-fly degradation (--degrade, degrade)"),
                         (jitter, "the colour jitter (--jitter, jitter)"), (camera, "the camera-noise stage (--camera-profiles, camera)"),
                         (gan, "the GAN stage (--gan)")):
            if on:
                raise ValueError(f"task sr with a right view (--lq-r, lq_r_store) does not go with {what}")
    if gan and (not training or not r.gan):
        raise ValueError(f"task {task} has no GAN stage (--gan): only training of {', '.join(t for t in RULES if RULES[t].gan)} runs "
                         "against the discriminator")
    if degrade:
        if not training or not r.degrade:
            raise ValueError(f"task {task} has no on-the-fly degradation (--degrade, degrade): only training of "
                             f"{', '.join(t for t in RULES if RULES[t].degrade)} makes its LQ that way")
        if lq:
            raise ValueError(f"task {task} with degrade makes its LQ from the GT crops; an LQ folder (--lq) or store is not used")
    elif degrade_crop is not None:
        raise ValueError("degrade_crop (--degrade-crop) belongs to degrade (--degrade)")
    if camera and not (training and degrade):
        raise ValueError("the camera-noise stage (--camera-profiles, camera) is stage 2 of the on-the-fly degradation: it belongs to "
                         "training with degrade (--degrade)")
    if jitter and not (training and degrade):
        raise ValueError("the colour jitter (--jitter, jitter) acts on the GT crops of the on-the-fly degradation: it belongs to "
                         "training with degrade (--degrade)")
    # kept: evaluate_folder ignores an LQ folder that the evaluate command line refuses
    if not library_eval:
        if r.lq_from == "folder" and not lq and not degrade:
            raise ValueError(f"task {task} needs an LQ folder (--lq) or store")
        if r.lq_from == "gt" and (lq or val_lq):
            raise ValueError(f"task {task} builds its LQ from the GT; an LQ folder (--lq, --val-lq) or store is not used")
        if val and r.lq_from == "folder" and not val_lq:
            raise ValueError(f"task {task} validates on --val-lq / --val-gt")

    if (usm or val_usm) and not r.usm:
        raise ValueError(f"task {task} has no USM-sharpened GT (--usm-gt, --usm, --val-usm, usm, usm_gt): only "
                         f"{', '.join(t for t in RULES if RULES[t].usm)} reads a GT folder next to its LQ")

    if scale is None:
        scale = r.default_scale
    # kept: task_inputs reads the scale of sr_bicubic alone; evaluation never looked at the scale of the tasks that read an LQ folder
    checked = r.crop == "scale" if where == "task_inputs" else (training or r.lq_from == "gt")
    if checked and not r.min_scale <= scale <= (r.max_scale or scale):
        raise ValueError(f"task {task} restores at scale 1, got {scale}" if r.max_scale == 1 else
                         f"task {task} needs a scale of at least {r.min_scale}, got {scale}")
    if degrade:
        degrade_crop = 400 if degrade_crop is None else int(degrade_crop)
        if scale not in (2, 4):
            raise ValueError(f"task {task} with degrade is built for scales 2 and 4, got {scale}")
        if channels != 3:
            raise ValueError(f"task {task} with degrade works on RGB images (the correlated noise has a 3 x 3 covariance)")
        if degrade_crop % 4 or degrade_crop < 4 * scale:
            raise ValueError(f"task {task}: the degradation crop is a multiple of 4 and at least 4 * scale = {4 * scale}, got {degrade_crop}")
        if camera and degrade_crop < 32:
            raise ValueError(f"task {task}: with the camera-noise stage the degradation crop is at least 32, got {degrade_crop}: the "
                             "stage's demosaic reflects by 2 and needs sides of at least 3, and the stage can follow the initial "
                             "halving and a resize by up to 2 * scale")
        if patch is not None and patch > degrade_crop // scale:
            raise ValueError(f"task {task}: a patch of {patch} does not fit the degraded crop of {degrade_crop // scale}")
    # kept: the evaluate command line checks the channels of db alone; dm on gray images fails later, in task_inputs
    if r.rgb_only and channels != 3 and (where != "evaluate" or r.taps):
        raise ValueError(f"task {task} works on RGB images")
    # kept: the train command line accepts --patch 2 for dm, the sampler needs 4
    if r.even_patch and patch is not None and (patch % 2 or (where == "sampler" and patch < 4)):
        raise ValueError(f"task {task} works on patches with an even side of at least 4")

    if not r.noise:
        # kept: evaluation ignores a sigma that training refuses
        if training and (sigma is not None or sigma_range is not None):
            raise ValueError(f"task {task} adds no noise; sigma / sigma_range are not used")
    else:
        if sigma_range is not None and not r.sigma_range:
            raise ValueError(f"task {task} adds noise at one fixed sigma")
        if (sigma is not None and sigma_range is not None) or (sigma is None and sigma_range is None and r.sigma_default is None):
            raise ValueError(f"task {task} needs a noise sigma" + (" or sigma_range (one of them)" if training else ""))
        if r.sigma_default is not None:
            sigma = r.sigma_default if sigma is None else float(sigma)
        if val and sigma is None:
            raise ValueError(f"validation of task {task} needs a fixed sigma")

    # kept: evaluate_folder and task_inputs ignore taps and a quality that are not the task's
    if r.taps and where == "sampler" and not taps:
        raise ValueError(f"task {task} needs taps: the (K, K) fp32 table of tasks.blur_taps, K odd and at most 31")
    if not r.taps and taps and not library_eval:
        raise ValueError(f"task {task} does not blur; a blur kernel (--blur-kernel, --blur-kernel-file, taps) is not used")
    if not r.quality:
        if (quality is not None or quality_range is not None) and not library_eval:
            raise ValueError(f"task {task} does not compress; quality / quality_range are not used")
    else:
        # kept: next to a range, the train command line takes a quality (that of validation); the sampler takes one of the two
        if quality is None and quality_range is None or (where == "sampler" and quality is not None and quality_range is not None):
            raise ValueError(f"task {task} needs a quality" + (" or quality_range (one of them)" if training else ""))
        if quality_range is not None:
            if not patchwise:
                raise ValueError(f"task {task} with a quality per sample compresses the cropped patches (patchwise); whole-image "
                                 "compression would recompress an image for every sample and is not built")
            quality_range = tuple(int(v) for v in quality_range)
            if len(quality_range) != 2 or not 1 <= quality_range[0] <= quality_range[1] <= 100:
                raise ValueError(f"task {task}: quality_range is (lo, hi) with 1 <= lo <= hi <= 100, got {quality_range}")
        if quality is not None:
            quality = int(quality)
            if not 1 <= quality <= 100:
                raise ValueError(f"task {task}: quality is 1 .. 100, got {quality}")
        elif val:
            raise ValueError(f"validation of task {task} needs a quality next to the quality range")
    return SimpleNamespace(rule=r, scale=scale, sigma=sigma, sigma_range=sigma_range, quality=quality, quality_range=quality_range,
                           degrade_crop=degrade_crop)


# ---- the command lines ------------------------------------------------------------------------------------------------------------
def add_task_arguments(ap, tasks):
    """The task and model options that ``evaluate`` and ``train`` share; ``tasks``: the choices of --task."""
    ap.add_argument("--task", default="sr", choices=tasks,
                    help="sr: LQ images from --lq; bsr (evaluate): LQ images from --lq, no --gt, scored by NIQE; dn / dm / sr_bicubic / "
                         "db / jpeg: the LQ is made from --gt on the device (denoising, demosaicking, classical SR by MATLAB-bicubic "
                         "downscaling at --scale, non-blind deblurring, JPEG compression at --quality)")
    ap.add_argument("--model", default="base", choices=["tiny", "small", "base"])
    ap.add_argument("--geometry", default="sr_ckpt_df2", help="a key of presets.GEOMETRIES")
    ap.add_argument("--scale", type=int, default=None, help="4 by default for --task sr / sr_bicubic / bsr; 1 for everything else")
    ap.add_argument("--channels", type=int, default=3, choices=[1, 3], help="1: grayscale model and images (dn_*_c1, jpeg_*_c1)")
    ap.add_argument("--upsampler", default=None, choices=["pixelshuffle", "pixelshuffledirect", "nearest+conv"],
                    help="the reconstruction tail; default: the model size's classical-SR tail (bsr_grl_base.ckpt: nearest+conv)")
    ap.add_argument("--sigma", type=float, default=None, help="--task dn: noise level on the 0..255 scale (15, 25, 50); --task db: the same, default 2")
    ap.add_argument("--blur-kernel", default="gaussian",
                    help="--task db: gaussian (25 x 25, sigma 1.6) or real1 .. real8 (the Levin09 motion kernels, from --blur-kernel-file)")
    ap.add_argument("--blur-kernel-file", default=None,
                    help="--task db with real1 .. real8: the reference's utils/blur_kernels/Levin09.npy, or a 2-D .npy of that kernel")
    ap.add_argument("--quality", type=int, default=None,
                    help="--task jpeg: the JPEG quality factor, 1 .. 100 (10, 20, 30, 40).  Training compresses every image whole, once; "
                         "with --quality-range it is the quality of validation only")


def resolve_arguments(ap, a, where, **more):
    """``resolve`` for parsed arguments ``a`` of a command line; a refusal ends through ``ap.error`` (exit status 2)."""
    try:
        return resolve(a.task, where, scale=a.scale, channels=a.channels, lq=a.lq is not None, sigma=a.sigma, quality=a.quality,
                       taps=a.blur_kernel != "gaussian" or a.blur_kernel_file is not None, **more)
    except ValueError as e:
        ap.error(str(e))


def load_taps(ap, a):
    """The blur taps of --blur-kernel / --blur-kernel-file for a task that blurs, else None."""
    if not RULES[a.task].taps:
        return None
    from . import tasks

    try:
        return tasks.blur_taps(tasks.load_blur_kernel(a.blur_kernel, a.blur_kernel_file))
    except (ValueError, OSError) as e:
        ap.error(f"--blur-kernel: {e}")
