"""Writes tests/golden/tasks/verdicts.json: what the task-aware entry points accept and reject, outcomes only.

Run in a checkout of the commit whose behaviour is to be kept; tests/test_task_rules.py replays every case on the current code
through ``run_case`` below and compares.  Only entry points that every commit since the jpeg task has are used:

  evaluate.main, train.main   ``grl_image_restoration_amd.GRL`` is patched to raise a sentinel, so no model is built: "accepted" (the
                              sentinel was reached) or "exit2"; accepted train cases also record (a.scale, a.sigma) after
                              ``_parser()`` and ``_check()``
  evaluate.task_inputs        a folder with one 16 x 24 PNG, device "cpu": "ok", "ValueError" or "TypeError"
  evaluate.evaluate_folder    the synthesised tasks over the same folder under an identity model: the base set, scale 1 / 2, and an LQ folder given
  data.PatchSampler           a CPU store of two 40 x 48 images, patch 16, batch 2, constructed and asked for one batch

Per entry point and task: the task's minimal valid option set, then that set with ONE change each -- scale unset / 1 / 2, the LQ
folder or store given or withheld, one channel, sigma given or withheld, a sigma range, quality 0 / 10 / 101, a quality range (10, 40)
and (40, 10), quality and range together, ``real3`` without a kernel file, a kernel file alone (for the library calls: the taps given
or withheld), patch 2 / 15, and for train ``--val-every 1`` alone, with ``--val-gt`` and with ``--val-lq`` as well.  Options foreign to
a task are included on purpose.

    python tools/make_golden_task_verdicts.py [--out tests/golden/tasks/verdicts.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "tasks", "verdicts.json")
NIQE = os.path.join("tests", "golden", "niqe", "niqe_pris_params.npz")

EVAL_TASKS = ("sr", "dn", "dm", "sr_bicubic", "bsr", "db", "jpeg")
TRAIN_TASKS = ("sr", "sr_bicubic", "dn", "dm", "db", "jpeg")
SYNTH_TASKS = ("dn", "dm", "sr_bicubic", "db", "jpeg")
ENTRIES = {"evaluate.main": EVAL_TASKS, "train.main": TRAIN_TASKS, "task_inputs": SYNTH_TASKS, "evaluate_folder": SYNTH_TASKS,
           "PatchSampler": TRAIN_TASKS}

# the minimal valid option set of a task per entry point; "{gt}", "{lq}", "{kernel}", "{niqe}" stand for the environment's paths
# (CLI), True for "the environment's store / taps" (PatchSampler, task_inputs)
BASE = {
    "evaluate.main": {"sr": {"lq": "{lq}", "gt": "{gt}"}, "dn": {"gt": "{gt}", "sigma": 25}, "dm": {"gt": "{gt}"},
                      "sr_bicubic": {"gt": "{gt}"}, "bsr": {"lq": "{lq}", "niqe_params": "{niqe}"}, "db": {"gt": "{gt}"},
                      "jpeg": {"gt": "{gt}", "quality": 10}},
    "train.main": {"sr": {"lq": "{lq}"}, "sr_bicubic": {}, "dn": {"sigma": 25}, "dm": {}, "db": {}, "jpeg": {"quality": 10}},
    "task_inputs": {"dn": {"sigma": 25}, "dm": {}, "sr_bicubic": {"scale": 2}, "db": {}, "jpeg": {"quality": 10}},
    "evaluate_folder": {"dn": {"sigma": 25}, "dm": {}, "sr_bicubic": {"scale": 2}, "db": {}, "jpeg": {"quality": 10}},
    "PatchSampler": {"sr": {"lq": True}, "sr_bicubic": {"scale": 2}, "dn": {"sigma": 25}, "dm": {}, "db": {"taps": True},
                     "jpeg": {"quality": 10}},
}


def _toggle(base, key, value):
    return {key: None} if key in base else {key: value}


def changes(entry, base):
    """[(label, {option: value, or None to withhold it})] for one entry point; see the module docstring."""
    cli = entry.endswith(".main")
    out = [("scale_unset", {"scale": None}), ("scale_1", {"scale": 1}), ("scale_2", {"scale": 2})]
    if entry != "task_inputs":                                   # task_inputs has no LQ argument
        out += [("lq_toggled", _toggle(base, "lq", "{lq}" if cli else True))]
    if entry == "evaluate_folder":
        return out[1:]
    out += [("channels_1", {"channels": 1}), ("sigma_toggled", _toggle(base, "sigma", 5))]
    out += [(f"quality_{q}", {"quality": q}) for q in (0, 10, 101)]
    if entry in ("train.main", "PatchSampler"):
        out += [("sigma_range", {"sigma_range": [5, 50]}), ("quality_range_10_40", {"quality": None, "quality_range": [10, 40]}),
                ("quality_range_40_10", {"quality": None, "quality_range": [40, 10]}),
                ("quality_and_range", {"quality": 10, "quality_range": [10, 40]}), ("patch_2", {"patch": 2}), ("patch_15", {"patch": 15})]
    if cli:
        out += [("real3_without_file", {"blur_kernel": "real3"}), ("kernel_file_alone", {"blur_kernel_file": "{kernel}"})]
    else:
        out += [("taps_toggled", _toggle(base, "taps", True))]
    if entry == "train.main":
        out += [("val_every", {"val_every": 1}), ("val_every_gt", {"val_every": 1, "val_gt": "{gt}"}),
                ("val_every_gt_lq", {"val_every": 1, "val_gt": "{gt}", "val_lq": "{lq}"})]
    return out


def cases():
    out = []
    for entry, tasks in ENTRIES.items():
        for task in tasks:
            base = BASE[entry][task]
            for label, change in [("base", {})] + changes(entry, base):
                opts = {k: v for k, v in {**base, **change}.items() if v is not None}
                out.append({"entry": entry, "task": task, "label": label, "options": opts})
    return out


# ---- running a case --------------------------------------------------------------------------------------------------------------
class Env:
    """The folders, stores and taps the cases name, made once in a temporary directory."""

    def __init__(self, root):
        from PIL import Image

        from grl_image_restoration_amd import tasks
        from grl_image_restoration_amd.data import PatchStore

        g = np.random.RandomState(0)
        self.paths = {"niqe": os.path.join(ROOT, NIQE), "kernel": os.path.join(root, "kernel.npy")}
        for name in ("gt", "lq"):
            self.paths[name] = os.path.join(root, name)
            os.makedirs(self.paths[name])
            Image.fromarray(g.randint(0, 256, (16, 24, 3)).astype(np.uint8)).save(os.path.join(self.paths[name], "im0.png"))
        np.save(self.paths["kernel"], np.full((5, 5), 1 / 25))
        imgs = [g.randint(0, 256, (40, 48, 3)).astype(np.uint8) for _ in range(2)]
        self.stores = {3: PatchStore(imgs), 1: PatchStore([im[:, :, 0] for im in imgs])}
        self.taps = tasks.blur_taps(tasks.gaussian_blur_kernel())


class _Reached(Exception):
    pass


def _argv(opts, env):
    argv = []
    for k, v in opts.items():
        vs = v if isinstance(v, list) else [v]
        argv += ["--" + k.replace("_", "-")] + [str(x).format(**env.paths) for x in vs]
    return argv


def _cli(mod, argv):
    import grl_image_restoration_amd as pkg

    def stop(*a, **k):
        raise _Reached()

    keep, pkg.GRL = pkg.GRL, stop
    try:
        with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
            mod.main(argv)
    except _Reached:
        return "accepted"
    except SystemExit as e:
        return f"exit{e.code}"
    except Exception as e:
        return type(e).__name__
    finally:
        pkg.GRL = keep
    return "returned"


def run_case(case, env):
    """The outcome of one case as the JSON file records it: a string; accepted train cases append the resolved scale and sigma."""
    from grl_image_restoration_amd import data, evaluate, train

    entry, task, o = case["entry"], case["task"], dict(case["options"])
    common = ["--task", task, "--model", "tiny", "--geometry", "yaml", "--device", "cpu"]
    if entry == "evaluate.main":
        return _cli(evaluate, common + _argv(o, env))
    if entry == "train.main":
        argv = common + ["--gt", env.paths["gt"], "--steps", "1", "--depths", "1", "--batch", "2", "--eager"]
        argv += _argv({"patch": 16, **o}, env)
        res = _cli(train, argv)
        if res == "accepted":
            ap = train._parser()
            a = ap.parse_args(argv)
            train._check(ap, a)
            res += f" scale={a.scale} sigma={a.sigma}"
        return res
    taps = env.taps if o.pop("taps", None) else None
    channels = o.pop("channels", 3)
    try:
        if entry == "task_inputs":
            list(evaluate.task_inputs(env.paths["gt"], task, channels, device="cpu", taps=taps, **o))
        elif entry == "evaluate_folder":
            lq = env.paths["lq"] if o.pop("lq", None) else None
            evaluate.evaluate_folder(lambda x: x, lq, env.paths["gt"], o.pop("scale", 1), device="cpu", verbose=False, task=task, taps=taps, **o)
        else:
            store = env.stores[channels]
            lq = env.stores[channels] if o.pop("lq", None) else None
            data.PatchSampler(task, store, lq, patch=o.pop("patch", 16), batch=2, taps=taps, **o).next()
    except Exception as e:
        return type(e).__name__
    return "ok"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as root:
        env = Env(root)
        done = {}
        for c in cases():
            done.setdefault(c["entry"], {}).setdefault(c["task"], {})[c["label"]] = run_case(c, env)
    with open(a.out, "w") as f:
        json.dump(done, f, indent=1)
        f.write("\n")
    print(f"{a.out}: {len(cases())} cases")


if __name__ == "__main__":
    main()
