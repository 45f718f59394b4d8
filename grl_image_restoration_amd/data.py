"""Training batches from a device-resident image store: the reference's training data path without its host loop.

  PatchStore     the training images as 8-bit H x W x C arrays back to back in ONE uint8 tensor, with a table of byte offsets and a
                 table of (H, W): what the reference keeps per image in its HDF5 cache (data/datasets/base_image.py:333-354), here
                 on the device
  .sample        a work list (image, x, y, flags) -> (B, C, P scale, P scale) fp32 in [0, 1]: _pad_images, _sample_patches
                 (base_image.py:276-293), _augment (base_image.py:356-372), ascontiguousarray and to_tensor
                 (restoration_sr.py:111-115) for the whole batch
  PatchSampler   the draws of one training batch (``random.Random``: image, _random_index of base_image.py:252-256, the three
                 flips) and the task's (lq, gt) pair built from them

  sample_views   several stores cut by ONE work list into channel windows of shared batches (the dual-pixel batch: left view, right
                 view, GT)

CUDA stores go through ``grl_sample_patches`` of libgrl_hip.so (csrc/patches.hip): one launch per batch and store, the work list
read from device memory, so the launch can be captured and replayed while the list changes.  ``sample_views`` on CUDA stores is one
``grl_sample_patch_views`` launch for all of its views.  There is no torch fallback for either.
CPU stores take the plain torch restatement below; the two are bitwise equal (tests/test_gpu_patches.py), and both equal the
reference's numpy chain (tests/test_patches.py): a value is ``float(v) / 255`` by IEEE division.

Flags of a work-list entry: bit 0 reverses the rows (``x[::-1]``), bit 1 the columns (``x[:, ::-1]``), bit 2 swaps the two axes
(``np.swapaxes(x, 0, 1)``), applied in that order after the crop.  The crop is rows ``x * scale .. x * scale + P * scale - 1`` and
columns ``y * scale ..``; pixels outside the image are 0, which is the reference's bottom / right padding of images smaller than
the patch.
"""
import random
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .task_rules import TRAIN_TASKS as TASKS, resolve

FLIP_ROWS, FLIP_COLS, SWAP_AXES = 1, 2, 4


class PatchStore:
    def __init__(self, images: Sequence, device="cpu"):
        """``images``: uint8 arrays (numpy or torch), each H x W x C or H x W, one channel count (1 or 3) for all of them."""
        arrs = []
        for im in images:
            a = im.detach().cpu().numpy() if torch.is_tensor(im) else np.asarray(im)
            if a.dtype != np.uint8:
                raise TypeError(f"PatchStore holds 8-bit images, got {a.dtype}")
            if a.ndim == 2:
                a = a[:, :, None]
            if a.ndim != 3 or a.shape[2] not in (1, 3) or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError(f"PatchStore: need H x W x C images with C = 1 or 3, got {a.shape}")
            arrs.append(np.ascontiguousarray(a))
        if not arrs:
            raise ValueError("PatchStore: no images")
        if len({a.shape[2] for a in arrs}) != 1:
            raise ValueError("PatchStore: every image of a store has the same number of channels")
        self.channels = int(arrs[0].shape[2])
        self.dims = [(int(a.shape[0]), int(a.shape[1])) for a in arrs]
        sizes = [a.size for a in arrs]
        self.data = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs]))
        self._starts = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])]
        self.offsets = torch.tensor(self._starts, dtype=torch.int64)
        self.dims_t = torch.tensor(self.dims, dtype=torch.int32)
        self.to(device)

    @classmethod
    def from_folder(cls, folder: str, channels: int = 3, device="cpu") -> "PatchStore":
        """Every image file of ``folder`` in sorted order, read as ``evaluate._read_image`` reads it (the same extensions, PIL's
        ``convert("RGB")`` or ``convert("L")``), kept as 8 bit."""
        from PIL import Image

        from .evaluate import gt_images

        mode = "L" if channels == 1 else "RGB"
        return cls([np.asarray(Image.open(p).convert(mode), dtype=np.uint8) for p in gt_images(folder)], device)

    def to(self, device) -> "PatchStore":
        """Moves the store (in place) and returns it."""
        self.data, self.offsets, self.dims_t = self.data.to(device), self.offsets.to(device), self.dims_t.to(device)
        return self

    @property
    def device(self):
        return self.data.device

    def __len__(self):
        return len(self.dims)

    def image(self, n: int) -> torch.Tensor:
        """Image ``n`` as an H x W x C uint8 view of the store."""
        H, W = self.dims[n]
        o = self._starts[n]
        return self.data[o : o + H * W * self.channels].view(H, W, self.channels)

    def sample(self, work: torch.Tensor, patch: int, scale: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``work``: int32 (B, 4) on the store's device -- image, top row x, left column y, flags (module docstring).  Returns fp32
        (B, C, patch * scale, patch * scale); ``out`` receives it when given (a static buffer of a captured step)."""
        patch, scale = int(patch), int(scale)
        if work.dtype != torch.int32 or work.dim() != 2 or work.shape[1] != 4 or work.shape[0] < 1 or not work.is_contiguous():
            raise ValueError("work list: a contiguous int32 (B, 4) tensor")
        if work.device != self.data.device:
            raise ValueError(f"work list on {work.device}, store on {self.data.device}")
        if patch < 1 or scale < 1:
            raise ValueError(f"patch and scale must be positive, got {patch}, {scale}")
        B, S = work.shape[0], patch * scale
        if out is None:
            out = ops.empty(B, self.channels, S, S, dtype=torch.float32, device=self.data.device)
        elif out.shape != (B, self.channels, S, S) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != work.device:
            raise ValueError("out: a contiguous fp32 (B, C, patch * scale, patch * scale) tensor on the store's device")
        if self.data.is_cuda:
            return self._hip_sample(work, patch, scale, out)
        return self._torch_sample(work, patch, scale, out)

    def _hip_sample(self, work, patch, scale, out):
        from . import _lib

        args = _lib.GrlPatchArgs(store=self.data.data_ptr(), offsets=self.offsets.data_ptr(), dims=self.dims_t.data_ptr(),
                                 N=len(self), C=self.channels, work=work.data_ptr(), B=work.shape[0], P=patch, scale=scale,
                                 out=out.data_ptr())
        _lib.launch("grl_sample_patches", args)
        return out

    def _torch_sample(self, work, patch, scale, out):
        """The reference's chain per sample in plain torch (any device): zero-padded crop, flips, axis swap, to_tensor."""
        S = patch * scale
        for b, (n, x, y, flags) in enumerate(work.tolist()):
            if not 0 <= n < len(self):
                raise IndexError(f"work list: image {n} of a store of {len(self)}")
            img = self.image(n)
            H, W = self.dims[n]
            r0, c0 = x * scale, y * scale
            crop = torch.zeros(S, S, self.channels, dtype=torch.uint8, device=img.device)
            h, w = min(S, H - r0), min(S, W - c0)
            if r0 < 0 or c0 < 0:
                raise IndexError(f"work list: negative origin ({x}, {y})")
            if h > 0 and w > 0:
                crop[:h, :w] = img[r0 : r0 + h, c0 : c0 + w]
            if flags & FLIP_ROWS:
                crop = crop.flip(0)
            if flags & FLIP_COLS:
                crop = crop.flip(1)
            if flags & SWAP_AXES:
                crop = crop.transpose(0, 1)
            out[b] = crop.permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        return out


def sample_views(views, work: torch.Tensor, patch: int):
    """Cuts several stores by one work list.  ``views``: a sequence of at most four ``(store, scale, out, c0)`` -- the view's
    patches, ``store.sample(work, patch, scale)``, go to channels ``c0 .. c0 + store.channels - 1`` of ``out``, a contiguous fp32
    (B, Ctot, patch * scale, patch * scale) batch on the stores' device; views may share an ``out`` (overlapping channel windows
    are not checked).  CUDA stores: one ``grl_sample_patch_views`` launch (csrc/patches.hip).  CPU stores: the torch restatement per
    view, copied into its window.  The two are bitwise equal (tests/test_gpu_dual_pixel.py).  Returns the ``out`` tensors."""
    views, patch = list(views), int(patch)
    if not 1 <= len(views) <= 4:
        raise ValueError(f"sample_views takes 1 to 4 views, got {len(views)}")
    if work.dtype != torch.int32 or work.dim() != 2 or work.shape[1] != 4 or work.shape[0] < 1 or not work.is_contiguous():
        raise ValueError("work list: a contiguous int32 (B, 4) tensor")
    if patch < 1:
        raise ValueError(f"patch must be positive, got {patch}")
    B = work.shape[0]
    for store, scale, out, c0 in views:
        S = patch * int(scale)
        if work.device != store.device or out.device != store.device:
            raise ValueError(f"work list on {work.device}, out on {out.device}, store on {store.device}")
        if int(scale) < 1:
            raise ValueError(f"scale must be positive, got {scale}")
        if out.dim() != 4 or out.shape[0] != B or tuple(out.shape[2:]) != (S, S) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out: a contiguous fp32 (B, Ctot, patch * scale, patch * scale) tensor")
        if c0 < 0 or c0 + store.channels > out.shape[1]:
            raise ValueError(f"channels {c0} .. {c0 + store.channels - 1} do not lie in an out of {out.shape[1]} channels")
    if work.is_cuda:
        from . import ops

        ops.sample_patch_views([(st.data, st.offsets, st.dims_t, len(st), st.channels, int(scale), out, int(c0))
                                for st, scale, out, c0 in views], work, patch)
    else:
        for store, scale, out, c0 in views:
            out[:, c0 : c0 + store.channels] = store.sample(work, patch, int(scale))
    return [v[2] for v in views]


class PatchSampler:
    """(lq, gt) training batches of a task from PatchStores.  The tasks, what each accepts and its defaults:
    ``task_rules.RULES`` (``scale`` is the SR factor, 1 for the tasks that restore at scale 1).  How each LQ is made:

      sr          paired stores: LQ patch ``patch``, GT patch ``patch * scale`` at the same place; every GT image is ``scale`` times
                  its LQ image.  With ``usm`` the GT store is replaced at construction by its USM-sharpened 8-bit twin: every image
                  through ``tasks.usm_sharp`` whole, once, on the store's device, and back to 8 bit by ``image8.pack8`` (the
                  reference's ``use_usm_pixel`` target, restoration_bsr.py:56-59,103-104, engines/base_psnr.py:39-41).  The LQ
                  store, the draws, the work list and the generator are untouched: a seed gives the same crops with and without
                  it.  The one deliberate difference from the reference's bsr path: the target is rounded to 8 bits (at most
                  1 / 510 off), and it is sharpened on the whole image rather than on a 400 x 400 crop, so a patch carries no
                  reflected crop border
      sr with ``lq_r_store``
                  dual-pixel defocus deblurring (the reference's paired data set with ``dual_pixel: True``,
                  restoration_paired_dataset.py:144-162): scale 1, RGB, three stores of equal image count, sizes and device.
                  ``lq_store`` is the left sub-aperture view, ``lq_r_store`` the right one; ``next`` returns
                  (lq [B, 6, P, P], gt [B, 3, P, P]) with the left view in channels 0 .. 2, the engine's
                  ``torch.cat([img_lq_l, img_lq_r], dim=1)`` (engines/base.py:119-120).  The reference draws ONE position
                  (_random_index on the first LQ view) and ONE set of flips for the three images (_augment(img_lq + [img_gt])): the
                  draws, the work list and ``rng_state()`` are exactly those of the same sampler without the right store.  CUDA
                  stores: one ``sample_views`` launch writes the three views in place, no cat; CPU stores: three ``sample`` calls
                  and a cat.  ``usm``, ``degrade``, ``jitter`` and ``plain_gt`` are refused next to it
      sr with ``degrade``
                  GT store only, scale 2 or 4: the reference's real-world-SR data path (restoration_bsr.py:83-110).  Per sample a
                  ``degrade_crop`` x ``degrade_crop`` crop of a GT image is drawn (image, position and flags as for every task, at
                  the crop size), with ``usm`` sharpened by ``tasks.usm_sharp`` -- the sharpened CROP is the degradation's input
                  and the target (restoration_bsr.py:103-110), not a whole-image store as on the paired path -- and run through a
                  freshly drawn ``bsr_degrade.draw_plan`` by ``bsr_degrade.apply_plans``; then one patch position is drawn in the
                  crop / scale LQ and the aligned (lq, gt) patches are cut.  Images smaller than the crop are refused at
                  construction: the store would pad them with zeros where the reference reflects them.  With ``camera`` (an
                  ``isp.CameraBank``; the crop is then at least 32) the plans are drawn with the bank, so a quarter of them carry
                  stage 2, the camera-noise model.  The reference hands that stage the degradation's input as HR and makes what
                  comes back the sharpened target (restoration_bsr.py:104-110): with ``usm`` the target of an acting sample is
                  the sharpened crop after the stage's HR pass; the ``plain_gt`` output is untouched; without ``usm`` the
                  engines train on the untouched crop (engines/base_psnr.py:39-41, base_gan.py:99-131), so the HR pass is not
                  run.  With ``jitter`` every crop first goes through the reference's ``ColorJitter`` (restoration_bsr.py:66-68,
                  100; ``jitter.py``, csrc/jitter.hip on CUDA), in place, right after it is cut and before the sharpening: the
                  sharpened target, the ``plain_gt`` output and the degradation's input all derive from the jittered crop.  The
                  parameter sets come from a CPU ``torch.Generator`` of the sampler's own, seeded with ``seed`` -- the reference
                  takes them from torch's global generator, a stream apart from the Python ``random`` of the degradation --,
                  one ``jitter.draw_jitter`` per sample in sample order; the Python draw stream and the noise generator are
                  untouched, and without ``jitter`` nothing is drawn and ``rng_state()`` has no ``"jitter"`` key
      sr with ``usm`` and ``plain_gt``
                  ``next`` returns (lq, gt, gt_plain): the sharpened target as above and the unsharpened crop of the same place --
                  the GAN stage's pixel target and the discriminator's real input (use_usm_pixel: True, use_usm_gan: False of
                  config/experiment/bsr/grl.yaml).  Draws and generator are untouched
      sr_bicubic, jpeg at a fixed ``quality``
                  GT store only.  The LQ store is made once per image at construction (``tasks.TRAIN_STORE_LQ`` on the store's
                  device; sr_bicubic also replaces the GT store by the images cropped to the scale); then sampled as ``sr``
      dn, dm, db, jpeg with ``quality_range``
                  from the sampled GT batch (``tasks.TRAIN_PAIR``).  db (``taps``: the (K, K) table of ``tasks.blur_taps``) draws and
                  crops at the enlarged patch ``patch`` + K - 1; whole-image compression at a quality per sample is not built

    Draws, from ``random.Random(seed)``, per sample and in this order: ``randrange(N)`` for the image; ``randrange(H' - P + 1)``
    and ``randrange(W' - P + 1)`` with H' = max(H, P), W' = max(W, P) the LQ-side size after the reference's padding
    (_random_index on the padded image, base_image.py:252-256, 397-402); three ``random() < 0.5`` for the flags; with
    ``sigma_range`` one ``uniform(lo, hi)``; with ``quality_range`` one ``randint(lo, hi)`` in that place.  For db, P is P'.
    With ``degrade``, P is the crop, and in that place come the draws of ``bsr_degrade.draw_plan`` and then
    ``randrange(crop / scale - patch + 1)`` twice, the row and the column of the LQ patch.
    """

    def __init__(self, task: str, gt_store: PatchStore, lq_store: Optional[PatchStore] = None, patch: int = 64, batch: int = 8,
                 scale: int = 1, sigma: Optional[float] = None, sigma_range: Optional[Sequence[float]] = None, seed: int = 0,
                 taps: Optional[torch.Tensor] = None, quality: Optional[int] = None,
                 quality_range: Optional[Sequence[int]] = None, patchwise: bool = True, usm: bool = False, degrade: bool = False,
                 degrade_crop: int = 400, plain_gt: bool = False, camera=None, jitter: bool = False,
                 lq_r_store: Optional[PatchStore] = None):
        from . import tasks

        patch, batch, scale = int(patch), int(batch), int(scale)
        if patch < 1 or batch < 1:
            raise ValueError(f"patch and batch must be positive, got {patch}, {batch}")
        o = resolve(task, "sampler", scale=scale, channels=gt_store.channels, lq=lq_store is not None, sigma=sigma,
                    sigma_range=sigma_range, taps=taps is not None, quality=quality, quality_range=quality_range, patch=patch,
                    patchwise=patchwise, usm=usm, degrade=degrade, degrade_crop=degrade_crop if degrade else None,
                    camera=camera is not None, jitter=jitter, dual_pixel=lq_r_store is not None)
        if lq_r_store is not None and plain_gt:
            raise ValueError("task sr with a right view (lq_r_store, --lq-r) has no USM-sharpened target: plain_gt is not used")
        if taps is not None and (taps.dim() != 2 or taps.shape[0] != taps.shape[1] or taps.shape[0] % 2 == 0 or taps.shape[0] > 31):
            raise ValueError("taps: the (K, K) fp32 table of tasks.blur_taps, K odd and at most 31")
        store_lq = tasks.TRAIN_STORE_LQ.get(task) if o.quality_range is None else None
        if store_lq is not None:
            gt_store, lq_store = _derived_stores(gt_store, lambda gt: store_lq(gt, o), scale if o.rule.crop == "scale" else 1)
        if degrade:
            small = [n for n, (H, W) in enumerate(gt_store.dims) if H < o.degrade_crop or W < o.degrade_crop]
            if small:
                raise ValueError(f"degrade: image {small[0]} ({gt_store.dims[small[0]][0]} x {gt_store.dims[small[0]][1]}) is smaller than "
                                 f"the crop {o.degrade_crop}; the store pads with zeros where the reference reflects")
        elif usm:
            self.plain_store = gt_store if plain_gt else None
            gt_store = _usm_store(gt_store)
        if lq_store is not None:
            if len(lq_store) != len(gt_store) or lq_store.channels != gt_store.channels or lq_store.device != gt_store.device:
                raise ValueError("task sr: the two stores need the same number of images, channel count and device")
            for n, ((h, w), (H, W)) in enumerate(zip(lq_store.dims, gt_store.dims)):
                if (H, W) != (h * scale, w * scale):
                    raise ValueError(f"task sr: image {n} is {h} x {w} (LQ) and {H} x {W} (GT), not a x{scale} pair")
        if lq_r_store is not None and (len(lq_r_store) != len(lq_store) or lq_r_store.channels != lq_store.channels
                                       or lq_r_store.device != lq_store.device or lq_r_store.dims != lq_store.dims):
            raise ValueError("task sr with a right view: the left and the right store need the same number of images, image sizes, "
                             "channel count and device")
        self.task, self.gt_store, self.lq_store, self.lq_r_store = task, gt_store, lq_store, lq_r_store
        self.patch, self.batch, self.scale = patch, batch, scale
        self.sigma, self.sigma_range = o.sigma, (tuple(float(v) for v in sigma_range) if sigma_range is not None else None)
        self.quality, self.quality_range = o.quality, o.quality_range
        self.rng = random.Random(seed)
        self.device = gt_store.device
        self.gen = torch.Generator(device=self.device).manual_seed(int(seed)) if o.rule.noise or degrade else None
        self.degrade, self.degrade_crop, self.usm, self.camera = bool(degrade), o.degrade_crop, bool(usm), camera
        if plain_gt and not usm:
            raise ValueError("plain_gt hands out the unsharpened target next to the sharpened one: it belongs to usm")
        self.plain_gt = bool(plain_gt)
        self.taps = taps.to(device=self.device, dtype=torch.float32).contiguous() if taps is not None else None
        self.draw_patch = patch + (self.taps.shape[0] - 1 if taps is not None else 0)   # the side the draws and the crop use
        if degrade:
            self.draw_patch = o.degrade_crop
        self.work = torch.zeros(batch, 4, dtype=torch.int32, device=self.device)      # the device work list, rewritten in place
        # the device quality list of jpeg with a range, rewritten in place like the work list
        self.qualities = torch.zeros(batch, dtype=torch.int32, device=self.device) if quality_range is not None else None
        self._pair = tasks.TRAIN_PAIR.get(task)
        self.jitter = bool(jitter)
        if self.jitter:
            from .jitter import JitterLists

            self.jitter_gen = torch.Generator().manual_seed(int(seed))               # CPU: the draws are host values
            self.jitter_lists = JitterLists(batch, o.degrade_crop, self.device)       # device lists, rewritten in place like the work list

    # ---- draws ---------------------------------------------------------------------------------------------------------------
    def draw(self):
        """One batch of draws: ([(image, x, y, flags)] * batch, [sigma] * batch or None); for jpeg with a quality range the second
        list holds the qualities, with ``degrade`` per sample (plan, row, column): the plan of ``bsr_degrade.draw_plan`` and the
        place of the LQ patch; with ``jitter`` (plan, row, column, params), ``params`` of ``jitter.draw_jitter``."""
        sizes = (self.lq_store or self.gt_store).dims
        P, work, sigmas = self.draw_patch, [], []
        for _ in range(self.batch):
            n = self.rng.randrange(len(sizes))
            H, W = max(sizes[n][0], P), max(sizes[n][1], P)
            x = self.rng.randrange(0, H - P + 1)
            y = self.rng.randrange(0, W - P + 1)
            flags = sum(bit for bit in (FLIP_ROWS, FLIP_COLS, SWAP_AXES) if self.rng.random() < 0.5)
            work.append((n, x, y, flags))
            if self.sigma_range is not None:
                sigmas.append(self.rng.uniform(*self.sigma_range))
            if self.quality_range is not None:
                sigmas.append(self.rng.randint(*self.quality_range))
            if self.degrade:
                from .bsr_degrade import draw_plan

                plan = draw_plan(self.rng, self.scale, self.degrade_crop, camera=self.camera)
                room = self.degrade_crop // self.scale - self.patch + 1
                sigmas.append((plan, self.rng.randrange(room), self.rng.randrange(room)))
                if self.jitter:
                    from .jitter import draw_jitter

                    sigmas[-1] += (draw_jitter(self.jitter_gen),)
        return work, (sigmas if self.sigma_range is not None or self.quality_range is not None or self.degrade else None)

    def rng_state(self):
        """What a checkpoint keeps to continue the stream of batches: the draws' state and the noise generator's; with ``jitter``
        also the state of the jitter's generator, under a key of its own."""
        state = {"draws": self.rng.getstate(), "noise": self.gen.get_state().cpu() if self.gen is not None else None}
        if self.jitter:
            state["jitter"] = self.jitter_gen.get_state()
        return state

    def set_rng_state(self, state):
        self.rng.setstate(_as_rng_state(state["draws"]))
        if self.gen is not None and state.get("noise") is not None:
            self.gen.set_state(state["noise"].cpu())
        if self.jitter and state.get("jitter") is not None:
            self.jitter_gen.set_state(state["jitter"].cpu())

    # ---- batches -------------------------------------------------------------------------------------------------------------
    def next(self, work=None, sigmas: Optional[Sequence[float]] = None, noise: Optional[torch.Tensor] = None):
        """(lq, gt) -- with ``plain_gt`` (lq, gt, gt_plain) -- on the store's device.  ``work``: an explicit work list (a sequence of (image, x, y, flags) or an int32 (B, 4)
        tensor) instead of fresh draws; ``sigmas`` with it for dn with a sigma range and for jpeg with a quality range (the
        qualities) and for ``degrade`` (the (plan, row, column) per sample; with ``jitter`` (plan, row, column, params)).
        ``noise`` (db): a unit-variance (B, 3, patch, patch) fp32 tensor used instead of the generator's draw (it is scaled by
        ``sigma / 255``)."""
        if work is None:
            work, sigmas = self.draw()
        if torch.is_tensor(work):
            wt = work.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            wt = self.in_place(self.work, torch.tensor([list(w) for w in work], dtype=torch.int32).reshape(-1, 4))
        if self.degrade:
            return self._degraded(wt, sigmas)
        if self.lq_r_store is not None:              # dual-pixel: left and right view side by side, one crop and one set of flips
            B, P = wt.shape[0], self.patch
            if not wt.is_cuda:
                lq = torch.cat([self.lq_store.sample(wt, P, 1), self.lq_r_store.sample(wt, P, 1)], dim=1)
                return lq, self.gt_store.sample(wt, P, 1)
            lq = ops.empty(B, 6, P, P, dtype=torch.float32, device=self.device)
            gt = ops.empty(B, 3, P, P, dtype=torch.float32, device=self.device)
            sample_views([(self.lq_store, 1, lq, 0), (self.lq_r_store, 1, lq, 3), (self.gt_store, 1, gt, 0)], wt, P)
            return lq, gt
        if self.lq_store is not None:                # paired stores, given or made at construction
            lq = self.lq_store.sample(wt, self.patch, 1)
            gt = self.gt_store.sample(wt, self.patch, self.scale)
            if self.plain_gt:
                return lq, gt, self.plain_store.sample(wt, self.patch, self.scale)
            return lq, gt
        return self._pair(self, self.gt_store.sample(wt, self.draw_patch, 1), sigmas, noise)

    def _degraded(self, wt, extras):
        """The batch of ``degrade``: crops, their optional sharpening, the pipeline, the aligned patches."""
        from . import tasks
        from .bsr_degrade import apply_plans

        if extras is None or len(extras) != wt.shape[0]:
            raise ValueError("degrade: one (plan, row, column) per sample next to an explicit work list")
        if any(len(e) != (4 if self.jitter else 3) for e in extras):
            raise ValueError("degrade: a sample's extras are (plan, row, column), with jitter (plan, row, column, params)")
        crops = plain = self.gt_store.sample(wt, self.degrade_crop, 1)
        if self.jitter:
            crops = plain = self.jitter_lists.run_(crops, [e[3] for e in extras])
        extras = [e[:3] for e in extras]
        if self.usm:
            crops = tasks.usm_sharp(crops)
        plans = [e[0] for e in extras]
        target = crops
        if self.usm and any(op["op"] == "camera" for plan in plans for op in plan):
            full, target = apply_plans(crops, plans, self.gen, hr=crops.clone())
        else:
            full = apply_plans(crops, plans, self.gen)
        P, s = self.patch, self.scale
        lq = torch.stack([full[b, :, r : r + P, c : c + P] for b, (_, r, c) in enumerate(extras)])
        gt = torch.stack([target[b, :, r * s : (r + P) * s, c * s : (c + P) * s] for b, (_, r, c) in enumerate(extras)])
        if self.plain_gt:
            return lq, gt, torch.stack([plain[b, :, r * s : (r + P) * s, c * s : (c + P) * s] for b, (_, r, c) in enumerate(extras)])
        return lq, gt

    @staticmethod
    def in_place(own: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """``t`` (CPU) written into the sampler's own device list ``own`` when the shapes match -- a captured launch reads that
        address -- else moved to its device."""
        if t.shape == own.shape:
            own.copy_(t)
            return own
        return t.to(own.device)


def _as_rng_state(s):
    """``random.Random.setstate`` wants tuples; a state that went through a checkpoint may hold lists."""
    return (s[0], tuple(s[1]), s[2])


def _derived_stores(gt_store: PatchStore, degrade, crop: int = 1):
    """(GT store, LQ store) of a task whose LQ is made once per image: every image of the GT store, cropped to a multiple of
    ``crop``, through ``degrade`` as a whole on the store's device, and back to 8 bit (the front ends return k / 255 exactly).
    With a crop the GT store is replaced by the cropped images."""
    from . import tasks

    gts: List[torch.Tensor] = []
    lqs: List[torch.Tensor] = []
    for n in range(len(gt_store)):
        img = gt_store.image(n)
        gt = tasks.modcrop(img.permute(2, 0, 1).unsqueeze(0), crop)
        if gt.shape[-2] < crop or gt.shape[-1] < crop:
            raise ValueError(f"image {n} ({img.shape[0]} x {img.shape[1]}) is smaller than the scale")
        lq = degrade(gt.to(torch.float32).div(255).contiguous())
        lqs.append((lq[0] * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().cpu())
        gts.append(gt[0].permute(1, 2, 0).contiguous().cpu())
    return (PatchStore(gts, gt_store.device) if crop > 1 else gt_store), PatchStore(lqs, gt_store.device)


def _usm_store(gt_store: PatchStore) -> PatchStore:
    """The store of the USM-sharpened images: every image whole through ``tasks.usm_sharp`` on the store's device, packed back to
    8 bit by ``image8.pack8``."""
    from . import tasks
    from .image8 import pack8

    out: List[torch.Tensor] = []
    for n in range(len(gt_store)):
        # k / 255 by IEEE division, on the host: torch divides a CUDA tensor by a scalar through the reciprocal
        x = gt_store.image(n).cpu().permute(2, 0, 1).unsqueeze(0).to(torch.float32).div(255).contiguous()
        out.append(pack8(tasks.usm_sharp(x.to(gt_store.device)))[0].cpu())
    return PatchStore(out, gt_store.device)
