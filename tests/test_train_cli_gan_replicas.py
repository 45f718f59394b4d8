"""``train --gan --data-parallel`` on the CPU: two spawned ranks call ``train.main`` with RANK / WORLD_SIZE / MASTER_* set, as torchrun
would set them (gloo; the arguments of tests/test_gan.py's GAN_ARGS).  A whole run of three steps that saves after two, and the third step
again from that checkpoint: the checkpoint carries every rank's sampler state, and the resumed replicas go on drawing their OWN patches.
"""
import os
import socket

import pytest
import torch

from tests.test_gan import GAN_ARGS, folders  # noqa: F401  (the fixture)

DP = GAN_ARGS + ["--data-parallel"]


def _rank(rank, world, port, ret, gt, lq, tmp):
    import torch.distributed as dist

    from grl_image_restoration_amd import train

    torch.set_num_threads(2)                         # (two ranks side by side; tiny tensors: more threads only contend)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    common = DP + ["--gt", gt, "--lq", lq]
    torch.manual_seed(0)
    whole = train.main(common + ["--steps", "3", "--save-every", "2", "--out", os.path.join(tmp, "whole")])
    dist.barrier()                                   # rank 0 has written step_2.ckpt on its way
    ckpt = os.path.join(tmp, "whole", "step_2.ckpt")
    rest = train.main(common + ["--steps", "3", "--resume", ckpt, "--out", os.path.join(tmp, "split")])
    dist.barrier()
    ret[rank] = {k: dict(steps=r["steps"], work=r["work"], checkpoint=r["checkpoint"], gan=r["gan"])
                 for k, r in (("whole", whole), ("rest", rest))}
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def runs(folders, tmp_path_factory):  # noqa: F811
    import torch.multiprocessing as mp

    gt, lq = folders
    tmp = str(tmp_path_factory.mktemp("gan_dp"))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ret = mp.Manager().dict()
    mp.spawn(_rank, args=(2, port, ret, gt, lq, tmp), nprocs=2, join=True)
    return ret[0], ret[1]


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def test_three_steps_and_a_checkpoint_with_every_ranks_sampler_state(runs):
    r0, r1 = runs
    assert r0["whole"]["steps"] == r1["whole"]["steps"] == [0, 1, 2]
    assert r0["whole"]["work"] != r1["whole"]["work"]                      # seed + rank: each replica draws its own patches
    assert r1["whole"]["checkpoint"] is None                                # rank 0 writes
    obj = _load(r0["whole"]["checkpoint"])
    assert set(obj) == {"state_dict", "step", "optimizer", "optimizer_d", "sampler_rng", "args", "sampler_rng_ranks"}
    ranks = obj["sampler_rng_ranks"]
    assert len(ranks) == 2 and repr(ranks[0]) != repr(ranks[1]) and repr(ranks[0]) == repr(obj["sampler_rng"])
    assert obj["args"]["data_parallel"] is True and obj["step"] == 3


def _equal(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_equal(x, y) for x, y in zip(a, b))
    return a == b


def test_resume_continues_the_whole_run_bit_for_bit(runs):
    r0, r1 = runs
    a, b = _load(r0["whole"]["checkpoint"]), _load(r0["rest"]["checkpoint"])
    assert a["state_dict"].keys() == b["state_dict"].keys()
    for k in a["state_dict"]:
        assert torch.equal(a["state_dict"][k], b["state_dict"][k]), k       # both networks, weight_u / weight_v among them
    assert _equal(a["optimizer"]["state"], b["optimizer"]["state"]) and _equal(a["optimizer_d"]["state"], b["optimizer_d"]["state"])
    for r in (r0, r1):
        assert r["rest"]["gan"] == r["whole"]["gan"][2:]


def test_after_the_resume_the_ranks_draw_different_patches(runs):
    r0, r1 = runs
    assert r0["rest"]["steps"] == r1["rest"]["steps"] == [2]
    assert r0["rest"]["work"] != r1["rest"]["work"]
    for r in (r0, r1):
        assert r["rest"]["work"] == [r["whole"]["work"][2]]                 # ... the ones the uninterrupted run drew


def test_flag_errors(folders, capsys, monkeypatch):  # noqa: F811
    from grl_image_restoration_amd import train

    gt, lq = folders
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:                                    # not a GAN run
        train.main(["--task", "sr", "--scale", "2", "--gt", gt, "--lq", lq, "--steps", "1", "--device", "cpu", "--data-parallel"])
    assert e.value.code == 2 and "--data-parallel belongs to --gan" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                                    # no process group, no WORLD_SIZE
        train.main(DP + ["--gt", gt, "--lq", lq, "--steps", "1"])
    assert e.value.code == 2 and "--data-parallel needs WORLD_SIZE > 1" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:                                    # without the flag: as ever
        train.main(GAN_ARGS + ["--gt", gt, "--lq", lq, "--steps", "1"])
    assert e.value.code == 2
    assert "--eager is single-process; the captured step owns the gradient all-reduce" in capsys.readouterr().err
