"""The GAN stage of real-world SR (config/experiment/bsr/grl.yaml): the vanilla GAN loss and one iteration of the alternation.

  gan_loss   losses/losses.py:190-293, gan_type "vanilla": BCEWithLogitsLoss against constant labels 1 / 0; the loss weight applies
             to the generator's term only
  GanStep    engines/base_gan.py:86-147 as Lightning runs it with two optimizers: optimizer 0 (generator) with the discriminator's
             parameters toggled off, then optimizer 1 (discriminator) on a fresh forward of the updated generator

The perceptual (VGG19) loss of the reference's criterion is ``perceptual.PerceptualLoss``, handed in as ``perceptual=``; with the
style loss on it is ``perceptual.PerceptualStyleLoss`` (base_gan.py:113-116).
"""
from typing import Callable, Dict, Optional

import inspect

import torch
import torch.distributed as dist
import torch.nn.functional as F

from .ddp import broadcast_module_state


def gan_loss(logits: torch.Tensor, target_is_real: bool, is_disc: bool, weight: float = 0.1) -> torch.Tensor:
    """losses/losses.py:212, 267-268, 290-293 (vanilla)."""
    label = logits.new_ones(logits.size()) * (1.0 if target_is_real else 0.0)
    loss = F.binary_cross_entropy_with_logits(logits, label)
    return loss if is_disc else loss * weight


def _forward_in_training(G, lq: torch.Tensor) -> torch.Tensor:
    """The generator's second forward of an iteration, under ``no_grad``.  A GRL on the GPU takes the training launch sequence for it,
    as in the first forward: without gradients ``GRL.forward`` would go the inference way, which packs a plan of every weight (and
    opens the tile-group streams) for weights that the optimizer has just changed and changes again one step later."""
    from . import forward_train
    from .model import GRL

    if isinstance(G, GRL) and G.training and lq.is_cuda:
        return forward_train.forward(G, lq)
    return G(lq)


class GanStep:
    """One call = one Lightning iteration of the reference's GAN engine.  ``pixel_loss(restored, target)``; both optimizers step
    once; returns the reference's logged scalars (detached tensors).  ``perceptual``: a ``perceptual.PerceptualLoss`` (or any callable
    returning ``(percep_loss, style_loss)``); its term, times ``perceptual_weight``, joins the generator's loss between the pixel and
    the GAN term (base_gan.py:105-112) against ``gt_usm`` under ``usm_percep``, and ``loss_g_percep`` joins the scalars.  A style
    term that is not None is multiplied by ``perceptual_weight`` as well (base_gan.py:113-116), joins the loss after the perceptual
    term and the scalars as ``loss_g_style``.  With ``perceptual=None`` nothing of either exists.  ``lpips``: an ``lpips.LPIPSLoss`` (or
    any callable returning a scalar); its term, times ``lpips_weight``, joins the generator's loss after the style term and before the
    GAN term, against ``gt_usm`` under ``usm_lpips``, and ``loss_g_lpips`` joins the scalars in that position (the reference's engine has
    no such term: it only scores LPIPS).  With ``lpips=None`` nothing of it exists.

    ``process_group`` (None: no communication, whatever torch.distributed's state): data-parallel replicas, the reference's
    ``strategy: ddp`` of bsr/grl.yaml.  Pass the bare modules.  At construction the parameters and floating-point buffers of BOTH
    networks are broadcast from the group's rank 0; every iteration then runs two collectives, one flat all-reduce of the
    generator's gradients after its backward and one of the discriminator's (``collectives`` counts them; ``wire_bf16``: bf16 on the
    wire).  Every parameter of either optimizer must receive a gradient (RuntimeError naming it otherwise).  An optimizer whose
    ``step`` takes no ``grad_scale`` gets the summed buffer divided by the world size instead.  The returned scalars are the
    replica's own, as under DistributedDataParallel.  The perceptual, style and LPIPS terms have no trained parameters and need
    nothing.  ``weight_u`` / ``weight_v`` are NOT broadcast again: with identical weights the spectral-norm kernels (no atomics,
    csrc/spectral_norm.hip) and the torch chain on the CPU advance them identically on every replica.  Not built: capture as a HIP
    graph, overlap of the all-reduce with the backward, find_unused_parameters."""

    def __init__(self, model_g, model_d, opt_g, opt_d, pixel_loss: Callable, pixel_weight: float = 1.0, gan_weight: float = 1.0,
                 gan_loss_weight: float = 0.1, usm_pixel: bool = False, usm_gan: bool = False, perceptual=None,
                 perceptual_weight: float = 1.0, usm_percep: bool = False, lpips=None, lpips_weight: float = 1.0, usm_lpips: bool = False,
                 process_group=None, wire_bf16: bool = False):
        self._group, self._world, self._wire_bf16 = None, 1, bool(wire_bf16)
        self.collectives = 0        # gradient all-reduces issued so far (two per iteration under a process group)
        if process_group is not None:
            for net in (model_g, model_d):
                if isinstance(net, torch.nn.parallel.DistributedDataParallel):
                    raise TypeError("GanStep owns the gradient all-reduce: pass the bare modules and process_group=..., not a "
                                    "DistributedDataParallel wrapper")
            if not (dist.is_available() and dist.is_initialized()):
                raise ValueError("GanStep(process_group=...) needs an initialised torch.distributed")
            self._group, self._world = process_group, dist.get_world_size(process_group)
            for net in (model_g, model_d):       # (the discriminator's weight_u / weight_v are among the buffers)
                broadcast_module_state(net, process_group)
        self.model_g, self.model_d, self.opt_g, self.opt_d = model_g, model_d, opt_g, opt_d
        self.pixel_loss, self.pixel_weight, self.gan_weight, self.gan_loss_weight = pixel_loss, pixel_weight, gan_weight, gan_loss_weight
        self.usm_pixel, self.usm_gan = usm_pixel, usm_gan
        self.perceptual, self.perceptual_weight, self.usm_percep = perceptual, perceptual_weight, usm_percep and perceptual is not None
        self.lpips, self.lpips_weight, self.usm_lpips = lpips, lpips_weight, usm_lpips and lpips is not None

    def _step(self, opt, net):
        """The optimizer step that follows a ``backward()``.  Under a process group: the gradients of ``opt``'s parameters go into
        one flat buffer (fp32 on the GPU), ONE all-reduce (SUM; through a bf16 copy with ``wire_bf16``) runs over the group, ``p.grad`` become
        views of the buffer and the 1 / world factor rides in the optimizer's ``grad_scale`` -- clipping then sees the norm of the
        averaged gradient, and the weight average is the same on every replica (train_graph.py's eager step)."""
        if self._group is None:
            opt.step()
            return
        params = [p for g in opt.param_groups for p in g["params"]]
        for p in params:
            if p.grad is None:
                name = next((k for k, q in net.named_parameters() if q is p), "<unnamed>")
                raise RuntimeError(f"GanStep (data parallel): parameter {name} received no gradient; pass the optimizer only "
                                   "parameters that take part in the step (requires_grad=False ones excluded)")
        flat = torch.cat([p.grad.reshape(-1) for p in params])       # (fp32 on the GPU; the CPU tests run it in float64)
        wire = flat.to(torch.bfloat16) if self._wire_bf16 else flat
        dist.all_reduce(wire, group=self._group)
        self.collectives += 1
        if self._wire_bf16:
            flat.copy_(wire)
        scaled = "grad_scale" in inspect.signature(opt.step).parameters
        if not scaled:
            flat.div_(self._world)
        for p, v in zip(params, flat.split([p.numel() for p in params])):
            p.grad = v.view_as(p)
        if scaled:
            opt.step(grad_scale=1.0 / self._world)
        else:
            opt.step()

    def __call__(self, lq: torch.Tensor, gt: torch.Tensor, gt_usm: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        if (self.usm_pixel or self.usm_gan or self.usm_percep or self.usm_lpips) and gt_usm is None:
            raise ValueError("usm_pixel / usm_gan / usm_percep / usm_lpips need the sharpened target")
        G, D_ = self.model_g, self.model_d
        out = {}
        # ---- optimizer 0: the generator (base_gan.py:96-126); toggle_optimizer: the discriminator's parameters are off ----
        d_params = [p for p in D_.parameters() if p.requires_grad]
        for p in d_params:
            p.requires_grad_(False)
        try:
            restored = G(lq)
            loss_g_pix = self.pixel_loss(restored, gt_usm if self.usm_pixel else gt) * self.pixel_weight
            loss_g_percep = loss_g_style = None
            if self.perceptual is not None:
                loss_g_percep, loss_g_style = self.perceptual(restored, gt_usm if self.usm_percep else gt)
                if loss_g_percep is not None:
                    loss_g_percep = loss_g_percep * self.perceptual_weight
                if loss_g_style is not None:
                    loss_g_style = loss_g_style * self.perceptual_weight
            loss_g_lpips = None
            if self.lpips is not None:
                loss_g_lpips = self.lpips(restored, gt_usm if self.usm_lpips else gt) * self.lpips_weight
            loss_g_gan = gan_loss(D_(restored), True, is_disc=False, weight=self.gan_loss_weight) * self.gan_weight
            self.opt_g.zero_grad(set_to_none=True)
            total = loss_g_pix
            for term in (loss_g_percep, loss_g_style, loss_g_lpips, loss_g_gan):
                if term is not None:
                    total = total + term
            total.backward()
            self._step(self.opt_g, G)
            self.opt_g.zero_grad(set_to_none=True)      # (gradients do not outlive their step: nothing of one optimizer's pass is
        finally:                                        # visible to the other's)
            for p in d_params:
                p.requires_grad_(True)
        out["loss_g_pix"] = loss_g_pix.detach()
        if loss_g_percep is not None:
            out["loss_g_percep"] = loss_g_percep.detach()
        if loss_g_style is not None:
            out["loss_g_style"] = loss_g_style.detach()
        if loss_g_lpips is not None:
            out["loss_g_lpips"] = loss_g_lpips.detach()
        out["loss_g_gan"] = loss_g_gan.detach()
        # ---- optimizer 1: the discriminator (base_gan.py:129-145); training_step calls self(batch) again ----
        with torch.no_grad():
            restored = _forward_in_training(G, lq)
        real_d_pred = D_(gt_usm if self.usm_gan else gt)
        loss_d_real = gan_loss(real_d_pred, True, is_disc=True)
        fake_d_pred = D_(restored.detach())
        loss_d_fake = gan_loss(fake_d_pred, False, is_disc=True)
        self.opt_d.zero_grad(set_to_none=True)
        (loss_d_real + loss_d_fake).backward()
        self._step(self.opt_d, D_)
        self.opt_d.zero_grad(set_to_none=True)
        out.update(loss_d_real=loss_d_real.detach(), loss_d_fake=loss_d_fake.detach(), out_d_real=real_d_pred.detach().mean(),
                   out_d_fake=fake_d_pred.detach().mean())
        return out
