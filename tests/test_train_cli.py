"""CPU tests of ``python -m grl_image_restoration_amd.train``: argument errors, and the checkpoint round trip with a one-block Tiny
model on CPU tensors (the composite torch path and FusedAdamW's CPU arithmetic): save, strict load, resume."""
import os

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, make_config, multistep_warmup_lr, train
from grl_image_restoration_amd.evaluate import load_checkpoint


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image

    d = tmp_path_factory.mktemp("train_gt")
    g = np.random.RandomState(0)
    for i in range(3):
        Image.fromarray(g.randint(0, 256, (40, 48, 3)).astype(np.uint8)).save(d / f"im{i}.png")
    return str(d)


def test_argument_errors(folder, capsys):
    base = ["--gt", folder, "--steps", "1", "--device", "cpu"]
    bad = [
        ["--task", "sr"],                                              # no --lq
        ["--task", "dn"],                                              # no --sigma
        ["--task", "dn", "--sigma", "25", "--sigma-range", "5", "50"],  # both
        ["--task", "dn", "--sigma", "25", "--scale", "2"],
        ["--task", "dm", "--scale", "2"],
        ["--task", "dm", "--lq", folder],
        ["--task", "sr_bicubic", "--scale", "1"],
        ["--task", "sr_bicubic", "--scale", "2", "--sigma", "5"],
        ["--task", "sr_bicubic", "--scale", "2", "--val-every", "1"],   # no --val-gt
        ["--task", "sr_bicubic", "--scale", "2", "--save-every", "1"],  # no --out
        ["--task", "sr_bicubic", "--scale", "2", "--milestones", "a+b"],
    ]
    for extra in bad:
        with pytest.raises(SystemExit) as e:
            train.main(base + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()


ARGS = ["--task", "sr_bicubic", "--scale", "2", "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--patch", "16", "--batch", "2",
        "--eager", "--device", "cpu", "--lr", "1e-3", "--milestones", "1+2", "--gamma", "0.5", "--warmup-iter", "1",
        "--warmup-init-lr", "1e-4", "--seed", "3"]


def test_checkpoint_round_trip_and_resume(folder, tmp_path, capsys):
    torch.manual_seed(0)
    whole = train.main(ARGS + ["--gt", folder, "--steps", "3", "--out", str(tmp_path / "whole")])
    assert whole["steps"] == [0, 1, 2] and all(np.isfinite(whole["losses"]))
    sched = dict(base_lr=1e-3, milestones=[1, 2], gamma=0.5, warmup_iter=1, warmup_init_lr=1e-4)
    assert whole["lrs"] == [multistep_warmup_lr(n, **sched) for n in range(3)] and whole["lrs"][2] == 1e-4 * 0.5 * 0.5

    torch.manual_seed(0)
    first = train.main(ARGS + ["--gt", folder, "--steps", "2", "--out", str(tmp_path / "split")])
    assert first["losses"] == whole["losses"][:2] and first["work"] == whole["work"][:2]
    ckpt = first["checkpoint"]
    assert ckpt == str(tmp_path / "split" / "step_2.ckpt") and os.path.isfile(ckpt)

    obj = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert set(obj) == {"state_dict", "step", "optimizer", "sampler_rng", "args"} and obj["step"] == 2
    assert all(k.startswith("model.") for k in obj["state_dict"])
    fresh = GRL(**make_config("tiny", "yaml", upscale=2, img_size=16, depths=[1], num_heads_window=[2], num_heads_stripe=[2]))
    res = load_checkpoint(fresh, ckpt, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert {int(s["step"]) for s in obj["optimizer"]["state"].values()} == {2}

    rest = train.main(ARGS + ["--gt", folder, "--steps", "3", "--resume", ckpt, "--out", str(tmp_path / "split")])
    assert rest["steps"] == [2] and rest["lrs"] == [whole["lrs"][2]]
    assert rest["work"] == [whole["work"][2]]                            # the next batch is that of the uninterrupted run
    assert rest["losses"][0] == pytest.approx(whole["losses"][2], rel=1e-5)
    a = torch.load(whole["checkpoint"], map_location="cpu", weights_only=False)["state_dict"]
    b = torch.load(rest["checkpoint"], map_location="cpu", weights_only=False)["state_dict"]
    assert a.keys() == b.keys() and all(torch.allclose(a[k], b[k], rtol=1e-5, atol=1e-7) for k in a)
    capsys.readouterr()
