"""Training from an image folder without Lightning / Hydra: the reference's training command around this package's step.

Restates the pieces of the reference's training run that sit around ``model(x)``:

  multistep_warmup_lr   optim/multi_steplr.py:22-30    linear warm-up, then torch's MultiStepLR as the reference runs it
  charbonnier           losses/losses.py:53-56         (the default loss is L1, config/loss/l1.yaml)
  the step              engines/base.py:221-236        forward, loss, backward, optimizer step: ``GraphedTrainStep`` (one captured
                                                       HIP graph) with ``FusedAdamW``, or the same step eagerly with ``--eager``
  the batches           data/datasets/*.py             ``data.PatchSampler`` over device-resident ``data.PatchStore``s
  validation            engines/base.py:256-268        ``evaluate.evaluate_folder`` every ``--val-every`` steps
  checkpoints           tools/trainer.py:93-115        the Lightning layout ``{"state_dict": {"model.<key>": tensor}}`` that
                                                       ``evaluate.load_checkpoint`` and the reference read, plus ``step``,
                                                       ``optimizer``, ``sampler_rng`` and ``args`` for ``--resume``

    python -m grl_image_restoration_amd.train --task sr --scale 4 --model base --geometry sr_ckpt_df2 \\
        --gt DIV2K/HR --lq DIV2K/LR_bicubic/X4 --patch 64 --batch 8 --steps 500000 \\
        --milestones 250000+400000+450000+475000 --gamma 0.5 --out runs/sr_x4 --val-gt Set5/GTmod12 --val-lq Set5/LRbicx4
    python -m grl_image_restoration_amd.train --task sr --scale 4 --model base --geometry bsr_psnr --upsampler nearest+conv \\
        --usm --val-usm --weight-decay 0 --gt pairs/GT --lq pairs/LQ --val-gt Set5/GTmod12 --val-lq Set5/LRbicx4 ...
    python -m grl_image_restoration_amd.train --task sr --scale 4 --model base --geometry bsr_psnr --upsampler nearest+conv \\
        --degrade --usm --weight-decay 0 --gt DF2K/HR --val-gt frozen/GT --val-lq frozen/LQ ...      (no --lq: bsr_degrade makes it;
        with --camera-profiles DIR, the reference's utils/cameraprofile folder, a quarter of the samples get its camera-noise stage;
        with --jitter every GT crop first goes through the reference's ColorJitter)
    python -m grl_image_restoration_amd.train --task sr --scale 1 --model base --geometry defocus --patch 480 --batch 1 \\
        --gt DPDD/train/target --lq DPDD/train/inputL --lq-r DPDD/train/inputR --steps 80000 --milestones 20000+40000+60000+70000 \\
        --val-gt DPDD/val/target --val-lq DPDD/val/inputL --val-lq-r DPDD/val/inputR ...     (dual-pixel defocus deblurring: the two
        views side by side, a 6-in / 3-out model; one crop and one set of flips for the three images)
    python -m grl_image_restoration_amd.train --task sr_bicubic --scale 2 --model small --geometry sr_ckpt_df4 --gt DIV2K/HR ...
    python -m grl_image_restoration_amd.train --task dn --sigma 25 --model small --geometry dn_df4 --gt DFWB --ckpt dn_grl_small_c3s25.ckpt ...
    python -m grl_image_restoration_amd.train --task dm --model small --geometry dm --gt DFWB ...
    python -m grl_image_restoration_amd.train --task jpeg --quality 10 --model small --geometry jpeg --patch 288 --gt DFWB --val-gt LIVE1 ...
    python -m grl_image_restoration_amd.train --task db --blur-kernel real4 --blur-kernel-file Levin09.npy --model small \\
        --geometry dn_df4 --gt DFWB --val-gt Set5/original ...

Schedule.  ``multistep_warmup_lr(step, ...)`` is the learning rate of optimizer step ``step`` (0-based) when the reference's
``MultiStepLRWarmup`` is stepped once per iteration.  During warm-up it is the reference's linear ramp.  After it, torch's
``MultiStepLR.get_lr`` is the chained form -- the optimizer's CURRENT rate, times ``gamma`` at a milestone -- so the plateau is the
LAST WARM-UP value ``init + (base - init) (W - 1) / W``, not ``base``, and a milestone inside the warm-up never fires.  That is what
the reference trains with and what is restated here, value for value (tests/golden/train/lr_schedule.npz).  The rate is written
into ``param_groups[*]["lr"]`` before each step; a captured step reads it from there (FusedAdamW.refresh_capture_hyper).

Captured steps.  The first step is ``GraphedTrainStep``'s own eager warm-up step on the first batch (it updates the weights and
counts as step 0); every later step replays the graph on the sampler's next batch.  ``charbonnier`` passes a non-zero
``recalibrate_every``: its gradients shrink as the error does, and the captured step freezes the fp16 gradient operand scale
(train_graph.py's docstring).  Validation runs between replays with the module in ``eval()``; the captured step stays valid -- a
replay bumps the parameters' version counters, the inference plan keys on them, and the graph's own buffers are not touched by an
eval forward -- so it is neither finished nor re-captured.  ``step.finish()`` runs before the optimizer state is read for a checkpoint.

GAN stage.  ``--gan`` (``--task sr``) runs ``gan.GanStep`` per step: the generator's step on pixel loss + GAN loss, then the
discriminator's (``discriminator.UNetDiscriminatorSN``), eagerly; single-process, or with ``--data-parallel`` under ``torchrun`` one
replica per process (below).  The printed loss is the generator's total.
Checkpoints carry both networks (``model.model_g.`` / ``model.model_d.``, u / v included) and both optimizers; ``evaluate`` reads
the generator out of them.  ``--vgg vgg19-dcbb9e9d.pth`` adds the third term of config/loss/gan_training_loss.yaml, the VGG19
perceptual loss (``perceptual.PerceptualLoss``); the frozen VGG is not written into checkpoints, so ``--resume`` takes ``--vgg`` again.
``--style-weight W`` (W > 0) adds the style half of that criterion (losses/losses.py:147-187: L1 between the Gram matrices of the same
five features, ``perceptual.PerceptualStyleLoss``); its scalar ``loss_g_style`` joins the log line, and the weight is kept in the
checkpoint's ``args`` (``--resume`` takes ``--style-weight`` again, as it takes ``--vgg``).
``--lpips-weight W`` (W > 0, with ``--lpips-vgg`` and ``--lpips-lin``) adds W times LPIPS (``lpips.LPIPSLoss``, the VGG16 trunk the metric
group ``restorer_perceptual`` scores with) after the style term, against the sharpened GT under ``--usm-lpips``; its scalar is
``loss_g_lpips``.  One loaded model serves the loss and, with ``--metric restorer_perceptual``, the validation.  The reference's engine
has no such term.  The weight is kept in the checkpoint's ``args``; the frozen trunk is not written, ``--resume`` takes the files again.

    python -m grl_image_restoration_amd.train --task sr --scale 4 --model base --geometry bsr --upsampler nearest+conv --gan \\
        --vgg vgg19-dcbb9e9d.pth --usm-percep --degrade --usm --ckpt runs/psnr/step_N.ckpt --lr 1e-4 --gt DF2K/HR --out runs/gan ...

Progressive training and MixUp.  ``--stage-steps 1000+2000 --batch-sizes 8+4 --patch-sizes 32+64`` and ``--mixup [--mixup-after N]``
restate what the reference's engine does to a batch between the loader and the model (engines/base.py:144-169; the transform is
stated in include/grl_hip.h, ``grl_batch_remix``).  The sampler builds the full ``--batch`` x ``--patch`` batch as without them;
``remix.BatchRemix`` then picks the stage's mini-batch, cuts its mini-patch and blends, one launch for lq and gt, from two streams
of its own (``--seed`` + rank): the sampler's draws are those of the same run without the options.  A captured step has its shapes
baked in: at a stage change it is finished and dropped, and the next one is built on the new shapes like the first step of a run
(its warm-up step is that step's optimizer step); between replays the remix writes straight into the step's static buffers.
Checkpoints carry the two streams under ``remix_rng``; ``--resume`` derives the stage from the step.  The result gains ``"stages"``.
Not with ``--gan``.

Stabilisers.  ``--clip-grad-norm X`` clips by the global gradient norm and ``--ema-decay D`` keeps an exponential moving average
of the generator's weights, both inside the fused optimizer step (``optim.FusedAdamW(max_grad_norm=, ema_decay=)``: no extra pass
over the gradients or the weights, no host read, so the captured and data-parallel steps keep them).  With ``--gan`` both optimizers
clip, each over its own parameters; the average is the generator's only.  With ``--ema-decay`` validation scores the averaged
weights (``ema_applied``) and checkpoints gain ``state_dict_ema`` (``evaluate`` / ``restore --ema``); ``--resume`` restores the
averages through the optimizer state.  The step line and the result gain ``grad_norm`` / ``"grad_norms"`` under ``--clip-grad-norm``.

Data-parallel.  Under ``torchrun`` (torch.distributed initialised from the environment) the bare module goes to
``GraphedTrainStep``, which owns the gradient all-reduce; each rank's sampler is seeded ``seed + rank``; rank 0 validates and
writes checkpoints.  ``--eager`` is single-process only.  ``--gan --data-parallel`` (the reference's bsr/grl.yaml: ``gpus: 8``,
``batch_size: 1`` per GPU, ``strategy: ddp``) hands the default group to ``gan.GanStep``: both networks are broadcast from rank 0, and
every iteration all-reduces the generator's and then the discriminator's gradients, one flat buffer each.  ``--batch`` is per replica.
Its checkpoints gain ``sampler_rng_ranks``, the sampler states of all ranks (gathered inside ``checkpoint()``, which every rank
calls); ``--resume`` at the same world size gives every rank its own entry, so the replicas keep drawing different patches; at
another world size, or from a checkpoint without the key, every rank takes ``sampler_rng`` as before.

    torchrun --nproc-per-node 8 -m grl_image_restoration_amd.train --task sr --scale 4 --model base --geometry bsr \\
        --upsampler nearest+conv --gan --data-parallel --batch 1 --patch 128 --degrade --usm --ckpt runs/psnr/step_N.ckpt ...
"""
import argparse
import contextlib
import os
from collections import Counter
from typing import List, Optional, Sequence

import torch

from . import data as D
from .task_rules import add_task_arguments, load_taps, resolve_arguments


def multistep_warmup_lr(step: int, base_lr: float, milestones: Sequence[int], gamma: float, warmup_iter: int = -1,
                        warmup_init_lr: float = 0.0) -> float:
    """The reference's ``MultiStepLRWarmup`` (optim/multi_steplr.py:22-30) after ``step`` scheduler steps, in its operation order
    (module docstring: the plateau after a warm-up is the last warm-up value, as in the reference)."""
    step = int(step)
    if step < warmup_iter:
        return warmup_init_lr + (base_lr - warmup_init_lr) / warmup_iter * step
    lr = base_lr
    if warmup_iter > 0:
        lr = warmup_init_lr + (base_lr - warmup_init_lr) / warmup_iter * (warmup_iter - 1)
    counts = Counter(int(m) for m in milestones)
    for m in sorted(counts):                      # MultiStepLR.get_lr: lr * gamma ** (times m is listed) when last_epoch == m
        if max(warmup_iter, 0) <= m <= step:
            lr = lr * gamma ** counts[m]
    return lr


def charbonnier(x: torch.Tensor, y: torch.Tensor, eps: float = 1e-3) -> torch.Tensor:
    """losses/losses.py:53-56."""
    diff = x - y
    return torch.mean(torch.sqrt((diff * diff) + (eps * eps)))


def l1(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """torch.nn.L1Loss (config/loss/l1.yaml)."""
    return (x - y).abs().mean()


LOSSES = {"l1": l1, "charbonnier": charbonnier}
RECALIBRATE_EVERY = 200        # captured Charbonnier steps: eager re-measurement of the gradient scale (train_graph.py)


def save_checkpoint(path: str, model, optimizer, step: int, sampler: D.PatchSampler, args: dict, model_d=None, optimizer_d=None,
                    remix=None, sampler_rng_ranks=None):
    """``model_d`` / ``optimizer_d`` (--gan): the reference's GAN-stage layout -- ``model.model_g.<k>`` and ``model.model_d.<k>``, the
    u / v buffers of the spectral normalisation among them -- and the second optimizer under ``optimizer_d``.  An optimizer that
    keeps a weight average (``FusedAdamW(ema_decay=...)``) adds ``state_dict_ema``: the generator's keys of ``state_dict``, every
    optimized parameter replaced by its average (BasicSR's ``params_ema``); the averages themselves resume through ``optimizer``.
    ``sampler_rng_ranks`` (--gan --data-parallel): the sampler states of all ranks, rank 0's first, under the key of that name."""
    if model_d is None:
        sd = {"model." + k: v.detach().cpu() for k, v in model.state_dict().items()}
    else:
        sd = {"model.model_g." + k: v.detach().cpu() for k, v in model.state_dict().items()}
        sd.update({"model.model_d." + k: v.detach().cpu() for k, v in model_d.state_dict().items()})
    obj = {"state_dict": sd,
           "step": int(step), "optimizer": optimizer.state_dict(), "sampler_rng": sampler.rng_state(), "args": dict(args)}
    if any(g.get("ema_decay") is not None for g in optimizer.param_groups):
        prefix = "model." if model_d is None else "model.model_g."
        obj["state_dict_ema"] = {prefix + k: v.detach().cpu() for k, v in optimizer.ema_state_dict(model).items()}
    if optimizer_d is not None:
        obj["optimizer_d"] = optimizer_d.state_dict()
    if remix is not None:                               # the streams of remix.BatchRemix; the stage follows from the step
        obj["remix_rng"] = remix.rng_state()
    if sampler_rng_ranks is not None:
        obj["sampler_rng_ranks"] = list(sampler_rng_ranks)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(obj, path + ".tmp")
    os.replace(path + ".tmp", path)
    return path


def _parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    add_task_arguments(ap, D.TASKS)
    ap.add_argument("--gt", required=True, help="GT training folder")
    ap.add_argument("--lq", default=None, help="LQ training folder (--task sr)")
    ap.add_argument("--lq-r", default=None,
                    help="--task sr --scale 1: training folder of the RIGHT sub-aperture views of a dual-pixel set (--lq holds the left "
                         "ones); the model is built with 6 input and 3 output channels")
    ap.add_argument("--depths", default=None, help="blocks per stage as a+b+c instead of the model size's (short experiments)")
    ap.add_argument("--ckpt", default=None, help="start weights (a reference checkpoint); random init without it")
    ap.add_argument("--patch", type=int, default=64, help="LQ patch side")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, required=True, help="train until this many optimizer steps have been taken in total")
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--weight-decay", type=float, default=1e-4)
    ap.add_argument("--milestones", default="", help="a+b+c: steps at which the rate is multiplied by --gamma")
    ap.add_argument("--gamma", type=float, default=0.5)
    ap.add_argument("--warmup-iter", type=int, default=-1)
    ap.add_argument("--warmup-init-lr", type=float, default=0.0)
    ap.add_argument("--loss", default="l1", choices=sorted(LOSSES))
    ap.add_argument("--sigma-range", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="--task dn: a level per sample")
    ap.add_argument("--quality-range", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                    help="--task jpeg: a quality per sample, drawn after the crop; the patches are compressed, not the images")
    ap.add_argument("--usm", action="store_true",
                    help="--task sr: train against USM-sharpened targets (the reference's use_usm_pixel: True of bsr/grl_psnr.yaml); "
                         "every GT image is sharpened whole, once")
    ap.add_argument("--degrade", action="store_true",
                    help="--task sr at scale 2 or 4, without --lq: the LQ of every sample is made on the device from a GT crop by the "
                         "blind-SR degradation (bsr_degrade: the reference's degradation_sr2, a fresh one per draw); with --usm the "
                         "crop is sharpened first and is the target")
    ap.add_argument("--degrade-crop", type=int, default=None,
                    help="--degrade: side of the GT crop that is degraded (default 400, the reference's; a multiple of 4)")
    ap.add_argument("--camera-profiles", default=None,
                    help="--degrade: the reference's utils/cameraprofile folder (the user's copy); turns on stage 2 of the degradation, "
                         "the ISP camera-noise model, for a quarter of the samples (isp.CameraBank.load; --degrade-crop at least 32)")
    ap.add_argument("--jitter", action="store_true",
                    help="--degrade: the reference's ColorJitter (brightness, contrast, saturation 0.2, hue 0.05) on every GT crop, before "
                         "the sharpening and the degradation (jitter.py; the validation set has none)")
    ap.add_argument("--val-usm", action="store_true", help="--task sr: validate against the USM-sharpened GT (val.use_usm: True)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--val-gt", default=None)
    ap.add_argument("--val-lq", default=None)
    ap.add_argument("--val-lq-r", default=None, help="--lq-r: the right views of the validation set")
    ap.add_argument("--val-every", type=int, default=0)
    ap.add_argument("--metric", default=None, help="a metric group of metrics.ALL_GROUPS or metrics.PERCEPTUAL_GROUPS instead of PSNR-Y")
    ap.add_argument("--lpips-vgg", default=None, metavar="PATH",
                    help="--metric restorer_perceptual: torchvision's vgg16-397923af.pth, read with torch.load; nothing is downloaded")
    ap.add_argument("--lpips-lin", default=None, metavar="PATH",
                    help="--metric restorer_perceptual: the lpips package's weights/v0.1/vgg.pth (the five 1x1 layers)")
    ap.add_argument("--niqe-params", default=None,
                    help="--metric restorer_perceptual: the reference's utils/metrics/niqe_pris_params.npz (default: the environment "
                         "variable GRL_NIQE_PARAMS)")
    ap.add_argument("--out", default=None, help="checkpoint folder")
    ap.add_argument("--save-every", type=int, default=0)
    ap.add_argument("--resume", default=None, help="a checkpoint of this command: weights, optimizer, step and sampler state")
    ap.add_argument("--eager", action="store_true", help="no captured graph")
    ap.add_argument("--gan", action="store_true",
                    help="--task sr: the GAN stage of real-world SR (config/experiment/bsr/grl.yaml, engines/base_gan.py): --ckpt is the "
                         "PSNR-stage checkpoint; every step is one generator step (pixel loss + GAN loss) and one step of the "
                         "spectrally normalised U-Net discriminator.  Runs eagerly; single-process unless --data-parallel; both "
                         "optimizers are Adam (FusedAdamW with weight decay 0, whatever --weight-decay says) on the same schedule")
    ap.add_argument("--data-parallel", action="store_true",
                    help="--gan under torchrun (WORLD_SIZE > 1, or an initialised process group): one replica per process, the "
                         "reference's strategy: ddp of bsr/grl.yaml.  GanStep owns the two gradient all-reduces of an iteration; --batch "
                         "is per replica; rank 0 prints, validates and writes checkpoints, which carry every rank's sampler state")
    ap.add_argument("--disc-ckpt", default=None, help="--gan: start weights of the discriminator (the model_d keys of a GAN checkpoint)")
    ap.add_argument("--disc-feat", type=int, default=64, help="--gan: the discriminator's num_feat")
    ap.add_argument("--gan-weight", type=float, default=1.0, help="--gan: gan_loss_weight of the engine (base_gan.py:122)")
    ap.add_argument("--gan-loss-weight", type=float, default=0.1, help="--gan: loss_weight of the GAN loss itself (losses.py:293)")
    ap.add_argument("--pixel-weight", type=float, default=1.0, help="--gan: weight of the pixel loss (base_gan.py:101)")
    ap.add_argument("--usm-gan", action="store_true", help="--gan: the discriminator's real input is the USM-sharpened GT (use_usm_gan)")
    ap.add_argument("--vgg", default=None, metavar="PATH",
                    help="--gan: turns the VGG19 perceptual loss on (config/loss/gan_training_loss.yaml: conv1_2 .. conv5_4 before ReLU, "
                         "layer weights 0.1 / 0.1 / 1 / 1 / 1, L1).  PATH is torchvision's vgg19-dcbb9e9d.pth, read with torch.load; nothing "
                         "is downloaded.  The frozen VGG is not written into checkpoints: --resume takes --vgg again")
    ap.add_argument("--perceptual-weight", type=float, default=1.0, help="--gan --vgg: weight of the perceptual loss (base_gan.py:110)")
    ap.add_argument("--usm-percep", action="store_true", help="--gan --vgg: the perceptual target is the USM-sharpened GT (use_usm_percep)")
    ap.add_argument("--style-weight", type=float, default=0.0, metavar="W",
                    help="--gan --vgg: W > 0 turns the style loss on (style_weight of losses.py:147-187: L1 between the Gram matrices of "
                         "the five tapped features, times W); 0: exactly the perceptual loss alone")
    ap.add_argument("--lpips-weight", type=float, default=None, metavar="W",
                    help="--gan: W > 0 adds W times LPIPS (lpips.LPIPSLoss: the mean over the batch, VGG16 trunk) to the generator's loss, "
                         "after the style term; needs --lpips-vgg and --lpips-lin, which then also serve --metric restorer_perceptual. "
                         "The frozen trunk is not written into checkpoints: --resume takes the two files again")
    ap.add_argument("--usm-lpips", action="store_true", help="--gan --lpips-weight: the LPIPS target is the USM-sharpened GT")
    ap.add_argument("--stage-steps", default="", metavar="a+b",
                    help="progressive training (engines/base.py:144-169): optimizer steps of every stage; with --batch-sizes and "
                         "--patch-sizes, one entry per stage.  The sampler builds --batch x --patch; a stage trains on a drawn "
                         "mini-batch and a drawn window of it (remix.BatchRemix, one grl_batch_remix launch)")
    ap.add_argument("--batch-sizes", default="", metavar="a+b", help="--stage-steps: samples per step of every stage, at most --batch")
    ap.add_argument("--patch-sizes", default="", metavar="a+b", help="--stage-steps: LQ patch side of every stage, at most --patch")
    ap.add_argument("--mixup", action="store_true",
                    help="blend every sample of a batch with a permuted partner, weights from Beta(1.2, 1.2) (the reference's "
                         "MixUp_AUG, mixup: True of config/defaults.yaml)")
    ap.add_argument("--mixup-after", type=int, default=0, metavar="STEP",
                    help="--mixup: from this optimizer step on (the reference waits for its sixth epoch)")
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                    help="clip the gradients to this global norm inside the fused optimizer step (Restormer's use_grad_clip); with --gan "
                         "both optimizers clip, each over its own parameters.  The step line gains grad_norm")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D",
                    help="keep an exponential moving average of the generator's weights (0 <= D < 1; BasicSR's ema_decay is 0.999): "
                         "validation runs on the averaged weights and checkpoints gain state_dict_ema (evaluate / restore --ema)")
    ap.add_argument("--device", default="cuda:0")
    return ap


def _check(ap, a):
    if a.val_every and a.val_gt is None:
        ap.error("--val-every needs --val-gt")
    o = resolve_arguments(ap, a, "train", sigma_range=a.sigma_range, quality_range=a.quality_range, patch=a.patch,
                          val=bool(a.val_every), val_lq=a.val_lq is not None, usm=a.usm or a.usm_gan or a.usm_percep or a.usm_lpips,
                          val_usm=a.val_usm,
                          degrade=a.degrade, degrade_crop=a.degrade_crop, gan=a.gan, camera=a.camera_profiles is not None,
                          jitter=a.jitter, dual_pixel=a.lq_r is not None)
    a.scale, a.sigma, a.degrade_crop = o.scale, o.sigma, o.degrade_crop
    if a.val_lq_r is not None and a.lq_r is None:
        ap.error("--val-lq-r belongs to --lq-r")
    if a.lq_r is not None and a.val_every and a.val_lq_r is None:
        ap.error("--lq-r validates on --val-lq / --val-lq-r / --val-gt")
    if not a.gan and (a.disc_ckpt is not None or a.usm_gan):
        ap.error("--disc-ckpt and --usm-gan belong to --gan")
    if not a.gan and (a.vgg is not None or a.usm_percep or a.perceptual_weight != 1.0):
        ap.error("--vgg, --perceptual-weight and --usm-percep belong to --gan")
    if a.vgg is None and (a.usm_percep or a.perceptual_weight != 1.0):
        ap.error("--perceptual-weight and --usm-percep need --vgg")
    if a.style_weight != 0.0 and not (a.gan and a.vgg is not None):
        ap.error("--style-weight needs --gan --vgg")
    if a.style_weight < 0.0:
        ap.error("--style-weight must not be negative")
    if a.vgg is not None and a.patch * a.scale < 16:
        ap.error("--vgg: the GT patch side (--patch times --scale) must be at least 16 (VGG19 pools four times)")
    if a.lpips_weight is None:
        if a.usm_lpips:
            ap.error("--usm-lpips needs --lpips-weight")
    else:
        if not a.gan:
            ap.error("--lpips-weight belongs to --gan")
        if not a.lpips_weight > 0.0:
            ap.error("--lpips-weight must be positive")
        if a.lpips_vgg is None or a.lpips_lin is None:
            ap.error("--lpips-weight needs --lpips-vgg and --lpips-lin (torchvision's vgg16-397923af.pth / the lpips package's vgg.pth)")
        if a.patch * a.scale < 16:
            ap.error("--lpips-weight: the GT patch side (--patch times --scale) must be at least 16 (VGG16 pools four times)")
    import torch.distributed as dist

    many = int(os.environ.get("WORLD_SIZE", "1")) > 1
    if a.data_parallel and not a.gan:
        ap.error("--data-parallel belongs to --gan (the other modes run data-parallel through the captured step, by themselves)")
    if a.data_parallel and not many and not (dist.is_available() and dist.is_initialized()):
        ap.error("--data-parallel needs WORLD_SIZE > 1 (torchrun) or an initialised process group")
    if a.gan and many and not a.data_parallel:
        ap.error("--gan runs eagerly: --eager is single-process; the captured step owns the gradient all-reduce")
    if a.gan and (a.patch * a.scale) % 8:
        ap.error("--gan: the discriminator takes GT patches whose side (--patch times --scale) is a multiple of 8")
    if a.clip_grad_norm is not None and not a.clip_grad_norm > 0:
        ap.error("--clip-grad-norm must be positive")
    if a.ema_decay is not None and not 0 <= a.ema_decay < 1:
        ap.error("--ema-decay must be in [0, 1)")
    if a.patch < 1 or a.batch < 1 or a.steps < 0:
        ap.error("--patch and --batch must be positive")
    if a.save_every and a.out is None:
        ap.error("--save-every needs --out")
    try:
        a.milestone_list = [int(m) for m in a.milestones.split("+") if m != ""]
        a.depth_list = [int(d) for d in a.depths.split("+")] if a.depths else None
    except ValueError:
        ap.error("--milestones and --depths are integers joined by +")
    try:
        a.stage_lists = [[int(v) for v in t.split("+") if v != ""] for t in (a.stage_steps, a.batch_sizes, a.patch_sizes)]
    except ValueError:
        ap.error("--stage-steps, --batch-sizes and --patch-sizes are integers joined by +")
    stages, batches, patches = a.stage_lists
    if not len(stages) == len(batches) == len(patches):
        ap.error("--stage-steps, --batch-sizes and --patch-sizes take one entry per stage")
    if any(v < 1 for t in a.stage_lists for v in t):
        ap.error("--stage-steps, --batch-sizes and --patch-sizes hold positive integers")
    if any(b > a.batch for b in batches) or any(p > a.patch for p in patches):
        ap.error("--batch-sizes / --patch-sizes: a stage cannot exceed --batch / --patch, which the sampler builds")
    if stages and sum(stages) < a.steps:
        ap.error("--stage-steps must cover --steps: the reference would index past its lists")
    if a.mixup_after and not a.mixup:
        ap.error("--mixup-after belongs to --mixup")
    if a.mixup_after < 0:
        ap.error("--mixup-after is an optimizer step")
    a.remix = bool(stages) or a.mixup
    if a.remix and a.gan:
        ap.error("--stage-steps, --batch-sizes, --patch-sizes and --mixup do not go with --gan: the GAN step carries up to three "
                 "targets, the reference's engine remixes two")
    if a.metric is not None:
        from .metrics import ALL_GROUPS, PERCEPTUAL_GROUPS

        if a.metric not in ALL_GROUPS and a.metric not in PERCEPTUAL_GROUPS:
            ap.error(f"--metric: one of {sorted(ALL_GROUPS) + sorted(PERCEPTUAL_GROUPS)}")


def main(argv: Optional[List[str]] = None):
    """Returns {"steps", "losses", "lrs", "work", "val", "checkpoint"}: per step taken in this call its index, loss, rate and work
    list; (step, result) of every validation; the last checkpoint written.  With the progressive / MixUp options also "stages":
    (step, batch, patch) at the first step taken and at every change."""
    import torch.distributed as dist

    from . import GRL, FusedAdamW, GraphedTrainStep, make_config
    from .evaluate import evaluate_folder, load_checkpoint, load_discriminator_checkpoint, load_lpips_arguments

    ap = _parser()
    a = ap.parse_args(argv)
    _check(ap, a)
    taps = load_taps(ap, a)
    # one loaded model serves the loss (--lpips-weight) and, if asked, the metric
    lpips_model, niqe_params = load_lpips_arguments(ap, a, needed_by="--lpips-weight" if a.lpips_weight is not None else None), None
    if a.metric == "restorer_perceptual":
        from .metrics import load_niqe_params

        try:
            niqe_params = load_niqe_params(a.niqe_params)
        except ValueError as e:
            ap.error(str(e))
    elif a.niqe_params is not None:
        ap.error("--niqe-params belongs to --metric restorer_perceptual")

    rank, world = 0, 1
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not dist.is_initialized():
        dist.init_process_group("nccl" if a.device.startswith("cuda") else "gloo")
    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(), dist.get_world_size()
        if a.device.startswith("cuda"):
            a.device = f"cuda:{int(os.environ.get('LOCAL_RANK', rank))}"
        if a.eager and world > 1:
            ap.error("--eager is single-process; the captured step owns the gradient all-reduce")
    device = torch.device(a.device)
    if device.type == "cuda":
        torch.cuda.set_device(device)

    over = {"upsampler": a.upsampler} if a.upsampler and a.scale > 1 else {}
    if a.depth_list:
        heads = make_config(a.model, a.geometry)["num_heads_window"][0]
        over.update(depths=a.depth_list, num_heads_window=[heads] * len(a.depth_list), num_heads_stripe=[heads] * len(a.depth_list))
    # two views side by side: GRL(in_channels=6, out_channels=3) of db_defocus/grl_dual_p480
    channels = dict(in_channels=6, out_channels=3) if a.lq_r is not None else dict(in_channels=a.channels)
    model = GRL(**make_config(a.model, a.geometry, upscale=a.scale, img_size=a.patch, **channels, **over))
    resume = torch.load(a.resume, map_location="cpu", weights_only=False) if a.resume else None
    if resume is not None:
        load_checkpoint(model, resume)
    elif a.ckpt:
        load_checkpoint(model, a.ckpt)
    model = model.to(device).train()
    model_d = None
    if a.gan:
        from .discriminator import UNetDiscriminatorSN
        from .gan import GanStep

        model_d = UNetDiscriminatorSN(a.channels, a.disc_feat, True)
        if resume is not None:
            load_discriminator_checkpoint(model_d, resume)
        elif a.disc_ckpt:
            load_discriminator_checkpoint(model_d, a.disc_ckpt)
        model_d = model_d.to(device).train()
        percep = None
        if a.vgg is not None:
            from .perceptual import GAN_LAYER_WEIGHTS, PerceptualLoss, PerceptualStyleLoss, load_vgg19

            if a.style_weight > 0:
                percep = PerceptualStyleLoss(GAN_LAYER_WEIGHTS, load_vgg19(a.vgg), style_weight=a.style_weight).to(device)
            else:
                percep = PerceptualLoss(GAN_LAYER_WEIGHTS, load_vgg19(a.vgg)).to(device)
        lpips_loss = None
        if a.lpips_weight is not None:
            from .lpips import LPIPSLoss

            lpips_loss = LPIPSLoss(lpips_model).to(device)

    camera = None
    if a.camera_profiles is not None:
        from .isp import CameraBank

        camera = CameraBank.load(a.camera_profiles)
    # the targets that are the sharpened GT
    usm_flags = [a.usm, a.usm_gan] + ([a.usm_percep] if a.vgg is not None else []) + ([a.usm_lpips] if a.lpips_weight is not None else [])
    gt_store = D.PatchStore.from_folder(a.gt, a.channels, device)
    lq_store = D.PatchStore.from_folder(a.lq, a.channels, device) if a.lq is not None else None
    lq_r_store = D.PatchStore.from_folder(a.lq_r, a.channels, device) if a.lq_r is not None else None
    sampler = D.PatchSampler(a.task, gt_store, lq_store, patch=a.patch, batch=a.batch, scale=a.scale, sigma=a.sigma,
                             sigma_range=a.sigma_range, seed=a.seed + rank, taps=taps,
                             quality=a.quality if a.quality_range is None else None, quality_range=a.quality_range,
                             usm=any(usm_flags), **(dict(lq_r_store=lq_r_store) if lq_r_store is not None else {}),
                             **(dict(plain_gt=True) if any(usm_flags) and not all(usm_flags) else {}),
                             **(dict(degrade=True, degrade_crop=a.degrade_crop, camera=camera, jitter=a.jitter) if a.degrade else {}))

    remix = None
    if a.remix:
        from .remix import BatchRemix

        remix = BatchRemix(a.batch, a.patch, a.scale, *a.stage_lists, mixup=a.mixup, mixup_after=a.mixup_after, seed=a.seed + rank,
                           device=device)

    opt = FusedAdamW(model.parameters(), lr=a.lr, weight_decay=0.0 if a.gan else a.weight_decay, max_grad_norm=a.clip_grad_norm,
                     ema_decay=a.ema_decay)
    opt_d = FusedAdamW(model_d.parameters(), lr=a.lr, weight_decay=0.0, max_grad_norm=a.clip_grad_norm) if a.gan else None
    start = 0
    if resume is not None:
        opt.load_state_dict(resume["optimizer"])
        if opt_d is not None:
            opt_d.load_state_dict(resume["optimizer_d"])
        ranks = resume.get("sampler_rng_ranks")
        # (a --gan --data-parallel checkpoint read at the world size that wrote it: every replica goes on with ITS OWN stream;
        # otherwise rank 0's state, as ever)
        sampler.set_rng_state(ranks[rank] if ranks is not None and len(ranks) == world else resume["sampler_rng"])
        if remix is not None and resume.get("remix_rng") is not None:
            remix.set_rng_state(resume["remix_rng"])
        start = int(resume["step"])

    loss_fn = LOSSES[a.loss]
    seen = []                                           # losses of eager calls (the captured step's warm-up step reports here)

    def recorded(y, t):
        loss = loss_fn(y, t)
        if not seen:
            seen.append(loss.detach())
        return loss

    lr_at = lambda n: multistep_warmup_lr(n, a.lr, a.milestone_list, a.gamma, a.warmup_iter, a.warmup_init_lr)
    out = {"steps": [], "losses": [], "lrs": [], "work": [], "val": [], "checkpoint": None}
    if a.clip_grad_norm is not None:
        out["grad_norms"] = []                          # per step the generator's global gradient norm, before clipping
    step_fn = None
    gan_step = None
    sizes = None                                        # (batch, patch) of the stage the captured step was built for
    if remix is not None:
        out["stages"] = []                              # (step, batch, patch) at the first step taken and at every change
    if a.gan:
        out["gan"] = []                                 # per step the reference's logged scalars (base_gan.py:103-140)
        gan_step = GanStep(model, model_d, opt, opt_d, loss_fn, pixel_weight=a.pixel_weight, gan_weight=a.gan_weight,
                           gan_loss_weight=a.gan_loss_weight, usm_pixel=a.usm, usm_gan=a.usm_gan, perceptual=percep,
                           perceptual_weight=a.perceptual_weight, usm_percep=a.usm_percep, lpips=lpips_loss,
                           lpips_weight=a.lpips_weight if a.lpips_weight is not None else 1.0, usm_lpips=a.usm_lpips,
                           process_group=dist.group.WORLD if a.data_parallel else None)

    def checkpoint(n):
        if step_fn is not None:
            step_fn.finish()
        extra = {}
        if a.data_parallel:                             # every rank is here: the replicas' samplers run on streams of their own
            states = [None] * world
            dist.all_gather_object(states, sampler.rng_state())
            extra = dict(sampler_rng_ranks=states)
        if rank == 0 and a.out is not None:
            out["checkpoint"] = save_checkpoint(os.path.join(a.out, f"step_{n}.ckpt"), model, opt, n, sampler, vars(a), model_d, opt_d,
                                                remix, **extra)

    for n in range(start, a.steps):
        lr = lr_at(n)
        for g in opt.param_groups + (opt_d.param_groups if opt_d is not None else []):
            g["lr"] = lr
        work, sigmas = sampler.draw()
        batch = sampler.next(work, sigmas)
        lq, gt = batch[:2]
        if remix is not None:
            if remix.sizes(n) != sizes:
                # a new stage has new shapes, and a captured step has its shapes baked in: drop it; the branch below builds the
                # next one on this step's batch, exactly as the first step of a run is built
                if step_fn is not None:
                    step_fn.finish()
                    step_fn = None
                    seen.clear()
                sizes = remix.sizes(n)
                out["stages"].append((n,) + sizes)
            # between replays the remix writes straight into the captured step's static buffers (its __call__ then copies nothing)
            lq, gt = remix(n, lq, gt, out=(step_fn.lq, step_fn.gt) if step_fn is not None else None)
        if gan_step is not None:
            # (lq, sharpened, plain) when the two targets differ; else one target serves both roles
            plain, sharp = (batch[2], gt) if len(batch) == 3 else (gt, gt if any(usm_flags) else None)
            logged = gan_step(lq, plain, sharp)
            out["gan"].append({k: float(v) for k, v in logged.items()})
            loss = sum(logged[k] for k in ("loss_g_pix", "loss_g_percep", "loss_g_style", "loss_g_lpips", "loss_g_gan") if k in logged)
        elif a.eager:
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(model(lq), gt)
            loss.backward()
            opt.step()
        elif step_fn is None:
            step_fn = GraphedTrainStep(model, opt, recorded, lq, gt, warmup=1,
                                       recalibrate_every=RECALIBRATE_EVERY if a.loss == "charbonnier" else 0)
            loss = seen[0]
        else:
            loss = step_fn(lq, gt)
        loss = float(loss.detach())
        out["steps"].append(n); out["losses"].append(loss); out["lrs"].append(lr); out["work"].append(work)
        if a.clip_grad_norm is not None:
            out["grad_norms"].append(opt.last_grad_norm())
        if rank == 0:
            style = f"  loss_g_style {out['gan'][-1]['loss_g_style']:.6f}" if gan_step is not None and "loss_g_style" in out["gan"][-1] else ""
            if a.clip_grad_norm is not None:
                style += f"  grad_norm {out['grad_norms'][-1]:.6f}"
            print(f"step {n:8d}  lr {lr:.3e}  loss {loss:.6f}{style}", flush=True)
        done = n + 1
        if a.val_every and done % a.val_every == 0 and rank == 0:
            model.eval()
            # (--ema-decay: the averaged generator is what gets scored, as BasicSR validates params_ema)
            with torch.no_grad(), (opt.ema_applied(model) if a.ema_decay is not None else contextlib.nullcontext()):
                v = evaluate_folder(model, a.val_lq, a.val_gt, a.scale, device=a.device, verbose=False, metric_group=a.metric,
                                    channels=a.channels, task=a.task, sigma=a.sigma, taps=taps, quality=a.quality, usm_gt=a.val_usm,
                                    niqe_params=niqe_params, lpips_model=lpips_model, lq_r_dir=a.val_lq_r)
            model.train()
            out["val"].append((done, v))
            print(f"step {n:8d}  validation {v}", flush=True)
        if a.save_every and done % a.save_every == 0 and done != a.steps:
            checkpoint(done)
    if a.steps > start or resume is None:
        checkpoint(max(a.steps, start))
    return out


if __name__ == "__main__":
    main()
