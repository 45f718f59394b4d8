"""Writes tests/golden/tasks/image8.npz: fp32 images and the bytes the reference saves for them (save_images: True).

The rounding is the UNMODIFIED reference's ``utils.utils_image.tensor_round``, imported from its tree (GRL_REFERENCE_ROOT, as for
oracle/refshim.py).  ``BaseModel._save_images`` itself needs Lightning and torchvision, which the fixture must not depend on; its
lines engines/base.py:529-550 are followed call for call in ``saved_bytes``:

    input_ = tensor_round(input_, 1.0)                              engines/base.py:260 (validation_step, before _save_images)
    tn_input = F.interpolate(tn_input, scale_factor=scale)          engines/base.py:529-530 (the SR tasks; rep > 1 here)
    to_pil_image(tn_input[0].detach())                              engines/base.py:545-550

and torchvision's ``to_pil_image`` is restated for its float branch, the only one a float tensor takes: ``pic.mul(255).byte()``, then
``np.transpose(pic.cpu().numpy(), (1, 2, 0))``.

The value set ``adversarial()``: every level k / 255; every tie (k + 0.5) / 255 computed in fp32 -- all 255 of them give exactly
k + 0.5 after the fp32 multiply by 255, so rounding half to even is what decides them, and a "+ 0.5 and truncate" gives k + 1 for
every even k -- with both fp32 neighbours of each; -0.0, negatives, values above 1, +-inf and a denormal.  NaN is left out: the
reference's result for it is undefined.  Cases (``meta["cases"]``: name, rep; arrays ``<name>__x`` fp32 (N, C, H, W) and ``<name>__y``
uint8 (N, H rep, W rep, C)): the value set as a gray and as an RGB image, at rep 1 and 2; a seeded ``rand * 1.2 - 0.1`` batch; and
small images at rep 2, 3, 4 and 8 filled from the value set.  ``meta["ties"]`` counts the exact ties and those with an even k.

The archive is written with fixed time stamps: the same reference tree gives the same bytes.

    python tools/make_golden_image8.py [--reference DIR] [--out tests/golden/tasks]
"""
import argparse
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tasks")


def adversarial() -> torch.Tensor:
    k = torch.arange(256, dtype=torch.float32)
    levels = k / 255.0
    ties = (k[:255] + 0.5) / 255.0
    inf = torch.tensor(float("inf"))
    special = torch.tensor([-0.0, -1e-3, -0.25, -1.0, -1e30, 1.0000001, 1.5, 3.0, 1e30, float("inf"), float("-inf"), 1e-40],
                           dtype=torch.float32)
    return torch.cat([levels, ties, torch.nextafter(ties, -inf), torch.nextafter(ties, inf), special])


def fill(values: torch.Tensor, shape, start: int = 0) -> torch.Tensor:
    """``shape`` filled with ``values`` cyclically, from index ``start``."""
    n = int(np.prod(shape))
    idx = (torch.arange(n) + start) % values.numel()
    return values[idx].reshape(shape).contiguous()


def saved_bytes(tensor_round, x: torch.Tensor, rep: int) -> torch.Tensor:
    """engines/base.py:260,529-550 on a batch: (N, C, H, W) fp32 -> (N, H rep, W rep, C) uint8."""
    t = tensor_round(x.clone(), 1.0)                      # clamps in place
    if rep > 1:
        t = F.interpolate(t, scale_factor=rep)
    out = []
    for pic in t:
        pic = pic.detach().mul(255).byte()                # to_pil_image, float tensor
        out.append(np.transpose(pic.cpu().numpy(), (1, 2, 0)))
    return torch.from_numpy(np.ascontiguousarray(np.stack(out)))


def build(tensor_round):
    v = adversarial()
    n = v.numel()
    side = int(np.ceil(np.sqrt(n / 3)))
    g = torch.Generator().manual_seed(8)
    cases = [("adv_c1", fill(v, (1, 1, 31, (n + 30) // 31)), 1), ("adv_c3", fill(v, (1, 3, side, side)), 1),
             ("adv_c3_rep2", fill(v, (1, 3, side, side), 7), 2), ("adv_c1_rep2", fill(v, (1, 1, 31, (n + 30) // 31), 3), 2),
             ("rand_c3", torch.rand(2, 3, 16, 20, generator=g) * 1.2 - 0.1, 1)]
    for rep in (2, 3, 4):
        cases.append((f"c3_4x5_rep{rep}", fill(v, (1, 3, 4, 5), 256 + 10 * rep), rep))
        cases.append((f"c1_3x3_rep{rep}", fill(v, (1, 1, 3, 3), 300 + 10 * rep), rep))
    cases.append(("c3_2x3_rep8", fill(v, (1, 3, 2, 3), 256), 8))
    arrays, meta_cases = {}, []
    for name, x, rep in cases:
        arrays[name + "__x"] = x.numpy()
        arrays[name + "__y"] = saved_bytes(tensor_round, x, rep).numpy()
        meta_cases.append({"name": name, "rep": rep, "shape": list(x.shape)})
    k = torch.arange(255, dtype=torch.float32)
    exact = ((k + 0.5) / 255.0) * 255.0 == k + 0.5
    meta = {"cases": meta_cases, "values": n, "ties": int(exact.sum()), "even_ties": int(exact[0::2].sum()),
            "source": "utils/utils_image.py:30-33 tensor_round; engines/base.py:260,529-550; torchvision to_pil_image (float branch)"}
    return arrays, meta


def write_npz(path: str, arrays: dict) -> None:
    """``np.savez_compressed`` with a fixed time stamp on every member, so that the file's bytes depend on the arrays alone."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=refshim.REFERENCE_ROOT)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args(argv)
    if a.reference not in sys.path:
        sys.path.insert(0, a.reference)
    from utils.utils_image import tensor_round  # the reference's

    arrays, meta = build(tensor_round)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "image8.npz")
    write_npz(path, dict(meta=np.array(json.dumps(meta)), **arrays))
    print(f"wrote {path}: {len(meta['cases'])} cases, {meta['ties']} exact ties ({meta['even_ties']} at even k), "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
