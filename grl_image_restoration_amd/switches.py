"""Every ``GRL_*`` environment switch of the project: one table, four accessors.

This module is the only place in the package that touches ``os.environ`` for a ``GRL_*`` name.  A new switch is one row here, one
accessor call where it is read (``grl_env_int`` in csrc/common.h on the C side) and one row in DESIGN.md's "Knobs" table;
tests/test_switches.py fails when the three disagree.  No switch selects a kernel: a path is chosen from what the code can observe
(shape, precision, device), and an A/B toggle lives on a development branch and is removed before merge.  Nor does a ``-D`` flag:
csrc has one build, its only preprocessor conditionals test the compiler's own ``__HIPCC__``, and instrumented or ablated builds
live on a development branch.

kind   on     default-on:  off only for the exact string "0"
       off    default-off: on only for the exact string "1"
       int, float, str     converted with int() / float() / taken as it is
default  ``SITE``: the read site passes it (``num(name, default=...)`` / ``text(name, default=...)``)
when   import | plan (while a plan is built or a module is constructed) | call -- documentation only, nothing enforces it.  For a
       ``csrc`` switch ``import`` means once per process, at the first launch that looks (a function-local static).
where  py | csrc (read by the launchers of libgrl_hip.so only; the accessors refuse these names)

The accessors do one ``os.environ.get`` each and cache nothing: the tests flip the per-call switches with ``monkeypatch.setenv``.
The measurements behind a switch stay in the comment at its read site and in DESIGN.md; the lines here are short on purpose.
"""
import os
from collections import namedtuple

Switch = namedtuple("Switch", "name kind default when doc where", defaults=("py",))
SITE = "site-dependent"

TABLE = {row[0]: Switch(*row) for row in (
    # ---- precision ----
    ("GRL_PRECISION", "str", SITE, "plan", "fast | high | auto: overrides the constructor's `precision` argument"),
    ("GRL_SPLIT_SITES", "str", SITE, "plan", "comma list of conv sites kept on split operands in `fast` (stage_conv, after, last, cab0; "
                                             "`name:x` = activations only); default: the model's own list"),
    ("GRL_HIQ_SCALE", "float", 50.0, "plan", "logit scale above which a block's q / k / anchor projection runs on split operands (0: always)"),
    ("GRL_NARROW_HIGH_SCALE", "float", 25.0, "plan", "logit scale above which `auto` moves the narrow / same-resolution models to split operands"),
    ("GRL_HIGH_CAB", "str", "", "plan", "split | fp16: operands of the CAB convolutions in precision `high` (default: fp16 where `auto` chose `high` "
                                        "for a Base-width model)"),
    ("GRL_CALIBRATE", "on", True, "plan", "0: `auto` without the measured per-block choice (the blanket rules)"),
    ("GRL_CAL_RMS", "float", 1.3e-4, "plan", "calibration bar on the probe image: rms error"),
    ("GRL_CAL_MAX", "float", 8.5e-4, "plan", "calibration bar on the probe image: largest error"),
    # ---- scheduling ----
    ("GRL_SPLIT_STREAMS", "int", 2, "call", "tile groups / HIP streams a batch is processed in"),
    ("GRL_GRAPH", "off", False, "plan", "1: replay the inference forward as a captured HIP graph (read at the first forward)"),
    ("GRL_CONV_SPLIT", "int", SITE, "call", "output channels per launch of a 3x3 convolution (0: one launch); default 96 for short-K layers, else 0"),
    ("GRL_PERSIST_GRID", "int", 256, "import", "cap on the grid of the persistent kernels (one workgroup per CU)", "csrc"),
    ("GRL_NO_CPU_COMPOSITE", "off", False, "call", "1: CPU tensors raise instead of taking the composite torch path"),
    ("GRL_NIQE_PARAMS", "str", "", "call", "path of the pristine NIQE model (niqe_pris_params.npz) when none is passed"),
    # ---- training ----
    ("GRL_DETERMINISTIC", "off", False, "call", "1: bit-identical training gradients (fixed-point accumulation; slower)"),
    ("GRL_TRAIN_BATCHED_PLANES", "on", True, "call", "0: per-slot plane and per-block table chains"),
    ("GRL_PLANES_KERNEL", "on", True, "call", "0: the torch chain instead of the head-plane kernel"),
    ("GRL_PLANES_WRITE32", "off", False, "call", "1: the head-plane kernel also writes the fp32 planes"),
    ("GRL_SE_KERNEL", "on", True, "call", "0: the torch expression of the squeeze-excite gate and gated residual"),
    ("GRL_REAL_WIDTHS", "on", True, "import", "0: padded operand copies everywhere"),
    ("GRL_STAT_REPLICAS", "int", 32, "import", "copies of the small cross-workgroup sums (LayerNorm dgamma / dbeta, plane scale gradients)"),
    ("GRL_GEMM_TN_WGS", "int", 0, "call", "workgroups the weight-gradient GEMM aims for (0: chosen by tile count)"),
    ("GRL_ATTN_BWD_SPLITS", "int", 0, "call", "1: no split attention-backward launches, n: n parts on every launch, -n: cap of the automatic choice",
     "csrc"),
    # ---- debug ----
    ("GRL_POISON", "off", False, "import", "1: every workspace tensor is NaN-filled before use"),
    ("GRL_DIRTY_LDS", "off", False, "import", "1: fill the LDS of every CU with NaN bytes before every launch"),
    ("GRL_CHECK_RANGE", "off", False, "call", "1: print the largest residual-stream magnitude per block (one stream)"),
)}


def _py(name, *kinds):
    s = TABLE[name]                       # KeyError: not a declared switch
    if s.where != "py":
        raise ValueError(f"{name} is read on the C side only (csrc/): there is nothing for Python to parse")
    if kinds and s.kind not in kinds:
        raise TypeError(f"{name} is a switch of kind {s.kind!r}")
    return s


def _default(s, default):
    if default is None:
        default = s.default
    if default is SITE:
        raise TypeError(f"{s.name}: the default depends on the read site, pass default=")
    return default


def on(name: str) -> bool:
    """An ``on`` / ``off`` switch."""
    if _py(name, "on", "off").kind == "on":
        return os.environ.get(name, "1") != "0"
    return os.environ.get(name, "0") == "1"


def num(name: str, default=None):
    """An ``int`` / ``float`` switch."""
    s = _py(name, "int", "float")
    v = os.environ.get(name)
    if v is None:
        return _default(s, default)
    return int(v) if s.kind == "int" else float(v)


def text(name: str, default=None) -> str:
    """A ``str`` switch."""
    return os.environ.get(name, _default(_py(name, "str"), default))


def is_set(name: str) -> bool:
    """Whether the variable exists at all, whatever it holds."""
    _py(name)
    return os.environ.get(name) is not None
