"""Writes tests/golden/tasks/dihedral.npz: the eight test-time transforms of the UNMODIFIED reference on a small image.

``Augment_RGB_torch`` (utils/dataset_utils.py:6-39) is imported from the reference's tree (GRL_REFERENCE_ROOT, as for
oracle/refshim.py) and its ``transform0`` .. ``transform7`` are called on ``arange(90).reshape(2, 3, 3, 5)``: non-square, so that a
transposing transform cannot pass for a shape-keeping one, and every value distinct, so that every index map is pinned.  Arrays:
``x`` int64 (2, 3, 3, 5) and ``t0`` .. ``t7``, (2, 3, 3, 5) for k = 0, 2, 4, 6 and (2, 3, 5, 3) for k = 1, 3, 5, 7.

The archive is written with fixed time stamps: the same reference tree gives the same bytes.

    python tools/make_golden_ensemble.py [--reference DIR] [--out tests/golden/tasks]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import refshim  # noqa: E402
from tools.make_golden_image8 import write_npz  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tasks")
SHAPE = (2, 3, 3, 5)


def build(augment):
    x = torch.arange(int(np.prod(SHAPE))).reshape(SHAPE)
    arrays = {"x": x.numpy()}
    for k in range(8):
        arrays[f"t{k}"] = np.ascontiguousarray(getattr(augment, f"transform{k}")(x).numpy())
    meta = {"shape": list(SHAPE), "source": "utils/dataset_utils.py:6-39 Augment_RGB_torch.transform0 .. transform7"}
    return arrays, meta


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=refshim.REFERENCE_ROOT)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args(argv)
    if a.reference not in sys.path:
        sys.path.insert(0, a.reference)
    from utils.dataset_utils import Augment_RGB_torch  # the reference's

    arrays, meta = build(Augment_RGB_torch())
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "dihedral.npz")
    write_npz(path, dict(meta=np.array(json.dumps(meta)), **arrays))
    print(f"wrote {path}: 8 transforms of {SHAPE}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
