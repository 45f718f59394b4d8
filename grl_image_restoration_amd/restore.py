"""Restores a folder of degraded images that have no ground truth: every image of --lq goes through the model, whole or tiled, and
is written as ``<out>/<stem><suffix>.png``.  Nothing is synthesised and nothing is scored (``evaluate`` does that); the 8-bit pack
and the PNG writer are ``image8.pack8`` / ``image8.ImageWriter``, the rounding is the reference's (engines/base.py:259-264,545-550).

    python -m grl_image_restoration_amd.restore --model base --geometry sr_ckpt_df2 --scale 4 --ckpt sr_grl_base_c3x4.ckpt \\
        --lq photos --out restored [--tile 256 --overlap 32 [--blend linear]] [--self-ensemble]
    python -m grl_image_restoration_amd.restore --model small --geometry dn_df4 --ckpt dn_grl_small_c3s25.ckpt --lq noisy --out clean
    python -m grl_image_restoration_amd.restore --model base --geometry defocus --ckpt db_defocus_dual_pixel_grl_base.ckpt \\
        --lq shots/left --lq-r shots/right --out sharp --tile 480 --overlap 48      (dual-pixel: the two views side by side, 6 in / 3 out)
"""
import argparse
import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional

import torch

from .evaluate import _read_image, _side_by_side, check_blend, gt_images, load_checkpoint
from .image8 import ImageWriter


@torch.no_grad()
def restore_folder(model, lq_dir: str, out_dir: str, scale: int = 1, tile: int = 0, overlap: int = 32, device: str = "cuda:0",
                   channels: int = 3, suffix: str = "_HQ", workers: int = 4, compress_level: int = 6, verbose: bool = False,
                   lq_r_dir: Optional[str] = None, self_ensemble: bool = False, blend: str = "uniform") -> List[str]:
    """Writes ``<out_dir>/<stem><suffix>.png`` for every image of ``lq_dir`` in sorted order and returns the paths; every file is
    complete when the call returns.  ``tile > 0`` restores images larger than the tile through ``tiling.forward_tiled``.  One reader
    thread decodes the next image while the device works on the current one; ``workers`` threads compress the PNGs.  ``lq_r_dir``
    (scale 1, RGB): dual-pixel inputs -- ``lq_dir`` holds the left views, ``lq_r_dir`` the right ones, matched by sorted order; the
    model (``GRL(in_channels=6, out_channels=3)``) gets the two side by side (engines/base.py:119-120) and the written file takes
    the LEFT view's stem.  ``self_ensemble``: the model runs as ``ensemble.SelfEnsemble(model)``, the x8 geometric self-ensemble (with
    ``tile``: every tile on its own).  ``blend`` (with ``tile``; ValueError without): "linear" or "cosine" feathers the overlaps of
    tiled inference (``tiling.blend_window``) instead of the reference's uniform average, which leaves a visible step where
    neighbouring tiles disagree."""
    from . import tiling

    if blend not in tiling.BLENDS:
        raise ValueError(f"blend is one of {', '.join(tiling.BLENDS)}, got {blend!r}")
    if blend != "uniform" and not tile:
        raise ValueError("blend belongs to tiled inference: give a tile size")

    if self_ensemble:
        from .ensemble import SelfEnsemble

        model = SelfEnsemble(model)

    files = gt_images(lq_dir)
    mode = "L" if channels == 1 else "RGB"
    read = _read_image
    if lq_r_dir is not None:
        if scale != 1 or channels != 3:
            raise ValueError(f"dual-pixel inputs (lq_r_dir) are RGB images restored at scale 1, got scale {scale}, {channels} channel(s)")
        rights = gt_images(lq_r_dir)
        if len(rights) != len(files):
            raise ValueError(f"{lq_dir}: {len(files)} images, {lq_r_dir}: {len(rights)} images")
        right_of = dict(zip(files, rights))
        read = lambda f, mode: _side_by_side(_read_image(f, mode), _read_image(right_of[f], mode))
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    with ThreadPoolExecutor(max_workers=1, thread_name_prefix="grl-image-reader") as reader, \
            ImageWriter(workers, compress_level) as writer:
        ahead = reader.submit(read, files[0], mode)
        for i, f in enumerate(files):
            lq = ahead.result()
            if i + 1 < len(files):
                ahead = reader.submit(read, files[i + 1], mode)
            lq = lq.to(device)
            if tile and tile < min(lq.shape[-2:]):
                sr = tiling.forward_tiled(model, lq, tile, overlap, scale, out_channels=getattr(model, "out_channels", None), blend=blend)
            else:
                sr = model(lq)
            path = os.path.join(out_dir, os.path.splitext(os.path.basename(f))[0] + suffix + ".png")
            writer.write(path, sr.float())
            paths.append(path)
            if verbose:
                print(f"{os.path.basename(f):32s} -> {path}")
    return paths


def _parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lq", required=True, help="folder of degraded images")
    ap.add_argument("--lq-r", default=None,
                    help="folder of the RIGHT sub-aperture views of dual-pixel inputs (--lq holds the left ones; --scale 1, --channels 3): "
                         "the model is built with 6 input and 3 output channels")
    ap.add_argument("--out", required=True, help="folder the restored images are written to (created)")
    ap.add_argument("--ckpt", default=None, help="reference checkpoint (.ckpt / .pth); random init without it")
    ap.add_argument("--ema", action="store_true",
                    help="load the averaged weights of --ckpt (state_dict_ema of train --ema-decay, or BasicSR's params_ema)")
    ap.add_argument("--model", default="base", choices=["tiny", "small", "base"])
    ap.add_argument("--geometry", required=True, help="a key of presets.GEOMETRIES")
    ap.add_argument("--scale", type=int, default=1, help="the model's upscaling factor; SR checkpoints need theirs (2, 3, 4)")
    ap.add_argument("--channels", type=int, default=3, choices=[1, 3], help="1: grayscale model and images")
    ap.add_argument("--upsampler", default=None, choices=["pixelshuffle", "pixelshuffledirect", "nearest+conv"],
                    help="the reconstruction tail; default: the model size's classical-SR tail (bsr_grl_base.ckpt: nearest+conv)")
    ap.add_argument("--depths", default=None, help="blocks per stage as a+b+c instead of the model size's (short experiments)")
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--blend", default=None, choices=["uniform", "linear", "cosine"],
                    help="with --tile: how overlapping tiles are mixed.  uniform (default): the reference's plain average; linear, "
                         "cosine: a ramp over the overlap that feathers the seams")
    ap.add_argument("--self-ensemble", action="store_true",
                    help="x8 geometric self-ensemble: restore the image under the eight flips and rotations and average the results "
                         "mapped back (with --tile: every tile on its own)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--suffix", default="_HQ", help="written files are <stem><suffix>.png")
    ap.add_argument("--workers", type=int, default=4, help="PNG writer threads (at most 8)")
    ap.add_argument("--compress-level", type=int, default=6, choices=range(10), metavar="0..9")
    return ap


def main(argv: Optional[List[str]] = None):
    from . import GRL, make_config

    ap = _parser()
    a = ap.parse_args(argv)
    if a.scale < 1:
        ap.error("--scale is at least 1")
    check_blend(ap, a)
    if a.lq_r is not None and (a.scale != 1 or a.channels != 3):
        ap.error("--lq-r (dual-pixel inputs) goes with --scale 1 and --channels 3")
    try:
        depths = [int(d) for d in a.depths.split("+")] if a.depths else None
    except ValueError:
        ap.error("--depths are integers joined by +")
    over = {"upsampler": a.upsampler} if a.upsampler and a.scale > 1 else {}
    if depths:
        heads = make_config(a.model, a.geometry)["num_heads_window"][0]
        over.update(depths=depths, num_heads_window=[heads] * len(depths), num_heads_stripe=[heads] * len(depths))
    channels = dict(in_channels=6, out_channels=3) if a.lq_r is not None else dict(in_channels=a.channels)
    model = GRL(**make_config(a.model, a.geometry, upscale=a.scale, **channels, **over)).eval()
    if a.ema and not a.ckpt:
        ap.error("--ema belongs to --ckpt")
    if a.ckpt:
        try:
            load_checkpoint(model, a.ckpt, ema=a.ema)
        except KeyError as e:
            ap.error(f"--ema: {e.args[0]}")
    model = model.to(a.device)
    return restore_folder(model, a.lq, a.out, a.scale, a.tile, a.overlap, a.device, a.channels, a.suffix, a.workers,
                          a.compress_level, verbose=True, lq_r_dir=a.lq_r, self_ensemble=a.self_ensemble, blend=a.blend)


if __name__ == "__main__":
    main()
