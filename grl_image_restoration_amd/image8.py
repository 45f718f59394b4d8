"""Restored images as files: the 8-bit pack on the device, the PNG writer behind it, and the reference's folder layout.

  pack8        fp32 (N, C, H, W) -> uint8 (N, H rep, W rep, C): tensor_round (utils/utils_image.py:30-33), for ``rep > 1`` the nearest
               upscale ``F.interpolate(input, scale_factor=scale)`` of the saved SR input (engines/base.py:529-530), and
               ``to_pil_image`` of a float tensor (``mul(255).byte()``, HWC; engines/base.py:545-554) in one ``grl_image_pack8`` launch
               (csrc/image8.hip).  What leaves the device is a quarter of the fp32 image, already in the encoder's layout
  ImageWriter  packs on the current stream, copies the bytes to pinned memory on a stream of its own, and compresses the PNG in a few
               threads while the GPU goes on with the next image
  save_paths   ``<save_dir>/X4/<dataset>/<stem>_{LQ,HQ,GT}.png`` and its siblings (engines/base.py:500-524, without the Lightning log
               folder); which subfolder a task gets is ``task_rules.RULES[task].save_tag``
"""
import ctypes as C
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Optional

import torch

from .task_rules import RULES

MAX_REP = 8
MAX_WORKERS = 8


def _torch_pack8(x: torch.Tensor, rep: int) -> torch.Tensor:
    """The formula of ``grl_image_pack8`` in torch ops; NaN is mapped to 0 first so that the cast is defined."""
    v = torch.where(x > 0, x, torch.zeros((), dtype=x.dtype, device=x.device)).clamp(max=1.0)
    k = (v * 255.0).round().to(torch.uint8)
    if rep > 1:
        k = k.repeat_interleave(rep, 2).repeat_interleave(rep, 3)
    return k.permute(0, 2, 3, 1).contiguous()


def pack8(x: torch.Tensor, rep: int = 1) -> torch.Tensor:
    """``uint8(rint(clamp(x, 0, 1) * 255))`` of an (N, C, H, W) fp32 tensor, C = 1 or 3, as (N, H rep, W rep, C) bytes; every source
    pixel fills a ``rep`` x ``rep`` block (1 .. 8).  Rounds half to even, NaN gives 0.  A CUDA tensor takes one ``grl_image_pack8``
    launch on the current stream and is read through its strides (a crop is not copied); a CPU tensor takes ``_torch_pack8``."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise TypeError(f"pack8 takes fp32 tensors, got {getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() != 4 or x.shape[1] not in (1, 3) or min(x.shape) < 1:
        raise ValueError(f"pack8: need a non-empty (N, C, H, W) tensor with C = 1 or 3, got {tuple(x.shape)}")
    if isinstance(rep, bool) or not isinstance(rep, int) or not 1 <= rep <= MAX_REP:
        raise ValueError(f"pack8: rep is an integer 1 .. {MAX_REP}, got {rep!r}")
    N, Cn, H, W = x.shape
    if N * H * rep * W * rep * Cn >= 1 << 31:
        raise ValueError(f"pack8: {tuple(x.shape)} at rep {rep} is 2^31 bytes or more")
    if not x.is_cuda:
        return _torch_pack8(x, rep)
    from . import _lib, ops

    out = ops.empty((N, H * rep, W * rep, Cn), dtype=torch.uint8, device=x.device)
    args = _lib.GrlPack8Args(x=x.data_ptr(), stride=(C.c_int64 * 4)(*x.stride()), N=N, C=Cn, H=H, W=W, rep=rep, out=out.data_ptr())
    _lib.launch("grl_image_pack8", args)
    return out


class ImageWriter:
    """Writes (1, C, H, W) fp32 images as 8-bit PNG files without holding the device up.

        with ImageWriter(workers=4) as w:
            w.write("out/a_HQ.png", sr)
            w.write("out/a_LQ.png", lq, rep=4)

    ``write`` packs on the current stream, copies the bytes into a pinned buffer on the writer's own stream (which first waits for
    the pack) and hands the buffer to one of ``workers`` threads (at most 8); the thread waits for the copy, writes ``path + ".tmp"``
    and renames it into place.  At most ``workers + 2`` images are in flight: beyond that ``write`` blocks.  ``close`` (or leaving the
    ``with`` block) waits for the threads and raises the first exception one of them met.  The directories must exist."""

    def __init__(self, workers: int = 4, compress_level: int = 6):
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.compress_level = int(compress_level)
        self.in_flight = self.workers + 2
        self._pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="grl-image-writer")
        self._slots = threading.BoundedSemaphore(self.in_flight)
        self._lock = threading.Lock()
        self._free = []                         # pinned staging buffers that no worker holds
        self.staging_allocated = 0              # pinned buffers made so far; images of one size need at most workers + 2
        self._streams = {}                      # device -> the copy stream
        self._seen = set()
        self._error = None
        self._closed = False

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:                                   # the block's own exception goes on; a worker's does not replace it
            self._pool.shutdown(wait=True)
            self._closed = True
        return False

    def _take(self, nbytes: int) -> torch.Tensor:
        """A pinned buffer of at least ``nbytes``: one of the free list, or a new one in place of a free one that is too small."""
        with self._lock:
            for i, b in enumerate(self._free):
                if b.numel() >= nbytes:
                    return self._free.pop(i)
            if self._free:
                self._free.pop()
            self.staging_allocated += 1
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)

    def write(self, path: str, x: torch.Tensor, rep: int = 1) -> None:
        if self._closed:
            raise RuntimeError("ImageWriter.write after close")
        if x.dim() != 4 or x.shape[0] != 1:
            raise ValueError(f"ImageWriter.write takes one image (1, C, H, W), got {tuple(x.shape)}")
        key = os.path.abspath(path)
        if key in self._seen:
            raise ValueError(f"{path}: already written by this writer (two inputs with one stem?)")
        self._slots.acquire()                   # blocks while workers + 2 images are in flight
        try:
            packed = pack8(x, rep)
            self._seen.add(key)
            if packed.is_cuda:
                stream = self._streams.get(packed.device)
                if stream is None:
                    stream = self._streams[packed.device] = torch.cuda.Stream(packed.device)
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(packed.device))
                buf = self._take(packed.numel())
                host = buf[: packed.numel()].view(packed.shape[1:])
                with torch.cuda.stream(stream):
                    stream.wait_event(ready)
                    host.copy_(packed[0], non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(stream)
            else:
                buf, host, done = None, packed[0], None
            # ``packed`` travels with the job: its memory is not handed out again before the copy on the other stream has finished
            self._pool.submit(self._job, done, buf, host, packed, path)
        except BaseException:
            self._slots.release()
            raise

    def _job(self, done, buf, host, packed, path):
        tmp = path + ".tmp"
        try:
            from PIL import Image

            if done is not None:
                done.synchronize()
            a = host.numpy()
            img = Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a)         # uint8 (H, W): mode "L"; (H, W, 3): "RGB"
            with open(tmp, "wb") as f:
                img.save(f, format="PNG", compress_level=self.compress_level)
            os.replace(tmp, path)
        except BaseException as e:
            with self._lock:
                if self._error is None:
                    self._error = e
            try:
                os.remove(tmp)
            except OSError:
                pass
        finally:
            del packed
            if buf is not None:
                with self._lock:
                    self._free.append(buf)
            self._slots.release()

    def close(self) -> None:
        """Waits for every image and raises the first exception a worker met."""
        if not self._closed:
            self._closed = True
            self._pool.shutdown(wait=True)
            self._free.clear()
        e, self._error = self._error, None
        if e is not None:
            raise e


def save_paths(save_dir: str, task: str, name: str, scale: int = 1, sigma: Optional[float] = None, quality: Optional[int] = None,
               dataset: str = "", flat: bool = False) -> Dict[str, str]:
    """{"LQ", "HQ", "GT"} -> file path of image ``name`` under the reference's layout (engines/base.py:500-524):
    ``<save_dir>/X<scale>/<dataset>/<stem>_HQ.png`` for the SR tasks, ``Sigma<sigma>`` for dn, ``QF<quality>`` for jpeg and
    ``<save_dir>/<dataset>/`` for the rest, as ``RULES[task].save_tag`` says.  ``stem``: the base name without its extension.
    ``flat``: straight under the data set's name whatever the task's tag is -- the reference's ``paired`` data module
    (engines/base.py:521-524), which the dual-pixel pairs of task sr come from."""
    tag = None if flat else RULES[task].save_tag
    sub = {"scale": f"X{scale}", "sigma": f"Sigma{float(sigma):g}" if tag == "sigma" else "", "quality": f"QF{quality}", None: ""}[tag]
    folder = os.path.join(*(p for p in (save_dir, sub, dataset) if p))
    stem = os.path.splitext(os.path.basename(name))[0]
    return {k: os.path.join(folder, f"{stem}_{k}.png") for k in ("LQ", "HQ", "GT")}
