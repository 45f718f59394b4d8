"""CPU tests of ``train --clip-grad-norm / --ema-decay`` and of ``load_checkpoint(..., ema=True)``, on the one-block Tiny model of
tests/test_train_cli.py (the composite torch path and FusedAdamW's CPU arithmetic)."""
import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, make_config, train
from grl_image_restoration_amd.evaluate import load_checkpoint


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image

    d = tmp_path_factory.mktemp("train_gt")
    g = np.random.RandomState(0)
    for i in range(3):
        Image.fromarray(g.randint(0, 256, (40, 48, 3)).astype(np.uint8)).save(d / f"im{i}.png")
    return str(d)


ARGS = ["--task", "sr_bicubic", "--scale", "2", "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--patch", "16", "--batch", "2",
        "--eager", "--device", "cpu", "--lr", "1e-3", "--seed", "3"]
# (a norm small enough to bite on every step of this model: the step line's grad_norm is the norm BEFORE clipping)
BOTH = ["--clip-grad-norm", "0.01", "--ema-decay", "0.9"]


def _tiny():
    return GRL(**make_config("tiny", "yaml", upscale=2, img_size=16, depths=[1], num_heads_window=[2], num_heads_stripe=[2]))


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def test_refusals(folder, capsys):
    base = ARGS + ["--gt", folder, "--steps", "1"]
    for extra in (["--ema-decay", "1.0"], ["--ema-decay", "-0.1"], ["--clip-grad-norm", "0"], ["--clip-grad-norm", "-1"]):
        with pytest.raises(SystemExit) as e:
            train.main(base + extra)
        assert e.value.code == 2, extra
    capsys.readouterr()


@pytest.fixture(scope="module")
def whole(folder, tmp_path_factory):
    """Four uninterrupted steps with both options (shared: run once)."""
    torch.manual_seed(0)
    out = tmp_path_factory.mktemp("whole")
    return train.main(ARGS + BOTH + ["--gt", folder, "--steps", "4", "--out", str(out)])


def test_checkpoint_holds_the_average_and_evaluate_loads_it(whole, capsys):
    assert len(whole["grad_norms"]) == 4 and all(np.isfinite(whole["grad_norms"])) and min(whole["grad_norms"]) > 0.01
    obj = _load(whole["checkpoint"])
    assert "state_dict_ema" in obj and obj["state_dict_ema"].keys() == obj["state_dict"].keys()
    assert all(g["max_grad_norm"] == 0.01 and g["ema_decay"] == 0.9 for g in obj["optimizer"]["param_groups"])
    raw, avg = _tiny(), _tiny()
    res = load_checkpoint(raw, obj, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    res = load_checkpoint(avg, obj, strict=True, ema=True)
    assert not res.missing_keys and not res.unexpected_keys
    moved = 0
    for (k, p), q in zip(raw.named_parameters(), avg.parameters()):
        assert torch.equal(q.detach(), obj["state_dict_ema"]["model." + k]), k
        assert torch.equal(p.detach(), obj["state_dict"]["model." + k]), k
        moved += int(not torch.equal(p, q))
    assert moved > 0                                    # the average lags the weights: it is not a copy of them
    # BasicSR's layout: {"params": ..., "params_ema": ...}
    basic = {"params": {k[len("model."):]: v for k, v in obj["state_dict"].items()},
             "params_ema": {k[len("model."):]: v for k, v in obj["state_dict_ema"].items()}}
    other = _tiny()
    load_checkpoint(other, basic, ema=True)
    assert all(torch.equal(a, b) for a, b in zip(other.parameters(), avg.parameters()))
    capsys.readouterr()


def test_a_checkpoint_without_the_average_is_refused_by_name(folder, tmp_path, capsys):
    torch.manual_seed(0)
    plain = train.main(ARGS + ["--gt", folder, "--steps", "1", "--out", str(tmp_path)])
    obj = _load(plain["checkpoint"])
    assert "state_dict_ema" not in obj
    with pytest.raises(KeyError, match="state_dict_ema"):
        load_checkpoint(_tiny(), obj, ema=True)
    capsys.readouterr()


def test_resume_restores_the_averages(whole, folder, tmp_path, capsys):
    torch.manual_seed(0)
    first = train.main(ARGS + BOTH + ["--gt", folder, "--steps", "2", "--out", str(tmp_path)])
    assert first["grad_norms"] == whole["grad_norms"][:2]
    rest = train.main(ARGS + BOTH + ["--gt", folder, "--steps", "4", "--resume", first["checkpoint"], "--out", str(tmp_path)])
    assert rest["steps"] == [2, 3]
    a, b = _load(whole["checkpoint"]), _load(rest["checkpoint"])
    assert a["state_dict_ema"].keys() == b["state_dict_ema"].keys()
    for k in a["state_dict_ema"]:
        assert torch.equal(a["state_dict_ema"][k], b["state_dict_ema"][k]), k
    capsys.readouterr()


def test_gan_stage_clips_both_optimizers_and_averages_the_generator_only(tmp_path, capsys):
    from PIL import Image

    gt, lq = tmp_path / "gt", tmp_path / "lq"
    gt.mkdir(); lq.mkdir()
    g = np.random.RandomState(0)
    for i in range(3):
        Image.fromarray(g.randint(0, 256, (40, 48, 3)).astype(np.uint8)).save(gt / f"im{i}.png")
        Image.fromarray(g.randint(0, 256, (20, 24, 3)).astype(np.uint8)).save(lq / f"im{i}.png")
    torch.manual_seed(0)
    out = train.main(["--task", "sr", "--scale", "2", "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--patch", "8", "--batch", "2",
                      "--gan", "--disc-feat", "8", "--device", "cpu", "--lr", "1e-3", "--seed", "3", "--gt", str(gt), "--lq", str(lq),
                      "--steps", "2", "--out", str(tmp_path / "run")] + BOTH)
    obj = _load(out["checkpoint"])
    gen = {k for k in obj["state_dict"] if k.startswith("model.model_g.")}
    assert gen and obj["state_dict_ema"].keys() == gen                    # generator keys only
    assert all(g["max_grad_norm"] == 0.01 for g in obj["optimizer"]["param_groups"] + obj["optimizer_d"]["param_groups"])
    assert all(g["ema_decay"] == 0.9 for g in obj["optimizer"]["param_groups"])
    assert all(g["ema_decay"] is None for g in obj["optimizer_d"]["param_groups"])
    assert all("ema" not in s for s in obj["optimizer_d"]["state"].values())
    model = GRL(**make_config("tiny", "yaml", upscale=2, img_size=8, depths=[1], num_heads_window=[2], num_heads_stripe=[2]))
    res = load_checkpoint(model, obj, strict=True, ema=True)              # model.model_g.* of the averaged dictionary
    assert not res.missing_keys and not res.unexpected_keys
    capsys.readouterr()


def test_step_line_names_the_norm(folder, capsys):
    torch.manual_seed(0)
    train.main(ARGS + ["--clip-grad-norm", "0.01", "--gt", folder, "--steps", "1"])
    assert "grad_norm" in capsys.readouterr().out
