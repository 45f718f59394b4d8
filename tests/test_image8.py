"""Saving restored images on the CPU (image8.py, restore.py, evaluate's --save-dir).  ``pack8`` is pinned bit for bit against
tests/golden/tasks/image8.npz, which tools/make_golden_image8.py wrote with the reference's own ``tensor_round`` followed by the calls
of ``_save_images`` (engines/base.py:529-550).  Every comparison is integer equality."""
import os

import numpy as np
import pytest
import torch

import grl_image_restoration_amd as G
from grl_image_restoration_amd import GRL, _lib, evaluate as EV, image8 as I, make_config, restore
from tests.test_tasks import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FIXTURE = {}


def image8_cases():
    return [c["name"] for c in golden("image8")[0]["cases"]]


def image8_case(name):
    """(x fp32 (N, C, H, W), rep, the reference's bytes (N, H rep, W rep, C)), loaded once and shared with the GPU tests."""
    if not _FIXTURE:
        meta, z = golden("image8")
        for c in meta["cases"]:
            _FIXTURE[c["name"]] = (z[c["name"] + "__x"], int(c["rep"]), z[c["name"] + "__y"])
    return _FIXTURE[name]


def adversarial_values():
    """The fixture's value set in its first case: levels, ties and their neighbours, the specials."""
    return image8_case("adv_c1")[0].flatten()


def read_png(path):
    from PIL import Image

    a = np.asarray(Image.open(path))
    return torch.from_numpy(a[:, :, None].copy() if a.ndim == 2 else a.copy())


def tiny_model(scale=1, seed=0):
    heads = make_config("tiny", "yaml")["num_heads_window"][0]
    torch.manual_seed(seed)
    return GRL(**make_config("tiny", "yaml", upscale=scale, depths=[1], num_heads_window=[heads], num_heads_stripe=[heads])).eval()


@pytest.mark.parametrize("name", image8_cases())
def test_pack8_on_the_cpu_equals_the_fixture(name):
    x, rep, want = image8_case(name)
    got = I.pack8(x, rep)
    assert got.dtype == torch.uint8 and got.is_contiguous() and got.shape == want.shape and torch.equal(got, want), name


def test_fixture_keeps_its_teeth():
    meta, _ = golden("image8")
    v = adversarial_values()
    k = torch.arange(255, dtype=torch.float32)
    ties = (k + 0.5) / 255.0
    present = torch.isin(ties, v)
    exact = (ties * 255.0 == k + 0.5) & present
    assert int(exact.sum()) >= 255 and int(exact[0::2].sum()) >= 120
    assert meta["ties"] >= 255 and meta["even_ties"] >= 120
    assert bool(torch.isin(torch.arange(256, dtype=torch.float32) / 255.0, v).all())
    inf = torch.tensor(float("inf"))
    assert bool(torch.isin(torch.nextafter(ties, inf), v).all()) and bool(torch.isin(torch.nextafter(ties, -inf), v).all())
    assert bool((v == float("inf")).any()) and bool((v == float("-inf")).any()) and bool((v < 0).any()) and bool((v > 1).any())
    assert bool(((v == 0) & torch.signbit(v)).any())                                      # -0.0
    assert bool(((v > 0) & (v < torch.finfo(torch.float32).tiny)).any())                  # a denormal
    assert not bool(torch.isnan(v).any())
    # half to even is what the fixture asks: adding 0.5 and truncating differs from it on every even k
    x, _, want = image8_case("adv_c1")
    trunc = (x.clamp(0, 1) * 255.0 + 0.5).floor().to(torch.uint8).permute(0, 2, 3, 1)
    assert int((trunc != want).sum()) >= 120
    assert {c["rep"] for c in meta["cases"]} >= {1, 2, 3, 4, 8}


def test_nan_gives_zero_and_arguments_are_checked():
    x = torch.full((1, 3, 2, 5), float("nan"))
    x[0, 1, 1, 2] = 1.0
    got = I.pack8(x, 2)
    assert got.shape == (1, 4, 10, 3) and int(got.sum()) == 4 * 255 and int(got[0, 2:, 4:6, 1].sum()) == 4 * 255
    good = torch.zeros(1, 3, 4, 4)
    with pytest.raises(TypeError):
        I.pack8(good.double())
    with pytest.raises(TypeError):
        I.pack8(good.to(torch.uint8))
    for bad in (good[0], good[:, :2], torch.zeros(1, 4, 2, 2), torch.zeros(1, 3, 0, 4)):
        with pytest.raises(ValueError):
            I.pack8(bad)
    for rep in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError):
            I.pack8(good, rep)
    assert G.pack8 is I.pack8 and G.ImageWriter is I.ImageWriter and G.restore_folder is restore.restore_folder


def test_pack8_args_layout_matches_header_and_abi():
    """The layout of GrlPack8Args is compared with the header in tests/test_abi.py, like every struct's;
    what is particular to this entry point stays here."""
    assert _lib.ABI_VERSION >= 30
    assert "grl_image_pack8" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "grl_hip.h")).read()
    assert "utils/utils_image.py:30-33" in header and "engines/base.py:529-530" in header and "NaN gives 0" in header


def test_save_paths_for_every_task():
    p = lambda task, **kw: I.save_paths("out", task, "sub/im_01.PNG", dataset="Set5", **kw)["HQ"]
    assert p("sr", scale=4) == os.path.join("out", "X4", "Set5", "im_01_HQ.png")
    assert p("sr_bicubic", scale=2) == os.path.join("out", "X2", "Set5", "im_01_HQ.png")
    assert p("bsr", scale=4) == os.path.join("out", "X4", "Set5", "im_01_HQ.png")
    assert p("dn", sigma=25.0) == os.path.join("out", "Sigma25", "Set5", "im_01_HQ.png")
    assert p("dn", sigma=12.5) == os.path.join("out", "Sigma12.5", "Set5", "im_01_HQ.png")
    assert p("jpeg", quality=10) == os.path.join("out", "QF10", "Set5", "im_01_HQ.png")
    assert p("dm") == os.path.join("out", "Set5", "im_01_HQ.png")
    assert p("db", sigma=2.0) == os.path.join("out", "Set5", "im_01_HQ.png")
    all_ = I.save_paths("out", "jpeg", "a.bmp", quality=40, dataset="live1")
    assert set(all_) == {"LQ", "HQ", "GT"} and all_["LQ"].endswith("a_LQ.png") and all_["GT"].endswith("a_GT.png")
    assert {t: EV.RULES[t].save_tag for t in EV.TASKS} == {"sr": "scale", "sr_bicubic": "scale", "bsr": "scale", "dn": "sigma",
                                                         "jpeg": "quality", "dm": None, "db": None}


def test_image_writer_on_cpu_tensors(tmp_path):
    g = torch.Generator().manual_seed(2)
    v = adversarial_values()
    rgb = v[torch.randint(0, v.numel(), (1, 3, 21, 34), generator=g)]
    gray = torch.rand(1, 1, 9, 13, generator=g) * 1.2 - 0.1
    with I.ImageWriter(workers=2) as w:
        assert w.workers == 2 and w.in_flight == 4
        w.write(str(tmp_path / "rgb.png"), rgb)
        w.write(str(tmp_path / "gray.png"), gray)
        w.write(str(tmp_path / "gray3.png"), gray, rep=3)
        for i in range(8):                                                             # more than workers + 2: write blocks, then goes on
            w.write(str(tmp_path / f"n{i}.png"), rgb[..., i:, :])
        with pytest.raises(ValueError, match="already written"):
            w.write(str(tmp_path / "rgb.png"), gray)
        with pytest.raises(ValueError):
            w.write(str(tmp_path / "two.png"), torch.zeros(2, 3, 4, 4))
    assert torch.equal(read_png(tmp_path / "rgb.png"), I.pack8(rgb)[0])
    assert torch.equal(read_png(tmp_path / "gray.png"), I.pack8(gray)[0])
    assert torch.equal(read_png(tmp_path / "gray3.png"), I.pack8(gray, 3)[0]) and read_png(tmp_path / "gray3.png").shape == (27, 39, 1)
    for i in range(8):
        assert torch.equal(read_png(tmp_path / f"n{i}.png"), I.pack8(rgb[..., i:, :])[0])
    from PIL import Image

    assert Image.open(tmp_path / "rgb.png").mode == "RGB" and Image.open(tmp_path / "gray.png").mode == "L"
    assert sorted(os.listdir(tmp_path)) == sorted(["rgb.png", "gray.png", "gray3.png"] + [f"n{i}.png" for i in range(8)])   # no .tmp
    with pytest.raises(RuntimeError):
        w.write(str(tmp_path / "late.png"), gray)
    assert I.ImageWriter(workers=100).workers == 8


def test_image_writer_raises_a_worker_exception_from_close(tmp_path):
    blocker = tmp_path / "dir"
    blocker.write_text("a file where the directory should be")
    w = I.ImageWriter(workers=1)
    w.write(str(tmp_path / "ok.png"), torch.rand(1, 3, 4, 4))
    w.write(str(blocker / "a.png"), torch.rand(1, 3, 4, 4))
    with pytest.raises(OSError):
        w.close()
    w.close()                                                                          # raised once
    assert sorted(os.listdir(tmp_path)) == ["dir", "ok.png"]
    with pytest.raises(OSError):
        with I.ImageWriter(workers=1) as w2:
            w2.write(str(blocker / "b.png"), torch.rand(1, 1, 4, 4))


def _folder(tmp_path, name, sizes, seed=0):
    from PIL import Image

    rng = np.random.RandomState(seed)
    d = tmp_path / name
    d.mkdir()
    imgs = {}
    for i, (h, w) in enumerate(sizes):
        imgs[f"im{i}"] = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        Image.fromarray(imgs[f"im{i}"]).save(d / f"im{i}.png")
    return d, imgs


def test_restore_main_on_the_cpu(tmp_path, capsys):
    d, imgs = _folder(tmp_path, "lq", [(16, 24), (20, 12)])
    out = tmp_path / "restored"
    torch.manual_seed(0)
    paths = restore.main(["--lq", str(d), "--out", str(out), "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--device", "cpu",
                          "--workers", "2"])
    capsys.readouterr()
    assert paths == [str(out / "im0_HQ.png"), str(out / "im1_HQ.png")] and sorted(os.listdir(out)) == ["im0_HQ.png", "im1_HQ.png"]
    model = tiny_model(seed=0)
    for (name, im), p in zip(imgs.items(), paths):
        lq = torch.from_numpy(im).permute(2, 0, 1)[None].float().div(255)
        with torch.no_grad():
            want = I.pack8(model(lq))[0]
        assert want.shape == im.shape and torch.equal(read_png(p), want), name
    # the library form, another suffix
    more = restore.restore_folder(model, str(d), str(tmp_path / "again"), suffix="_x", device="cpu", workers=1)
    assert [os.path.basename(p) for p in more] == ["im0_x.png", "im1_x.png"]
    assert torch.equal(read_png(more[1]), read_png(paths[1]))
    for bad in ([], ["--lq", str(d)], ["--lq", str(d), "--out", str(out)]):                # --lq, --out, --geometry are required
        with pytest.raises(SystemExit) as e:
            restore.main(bad)
        assert e.value.code == 2
    capsys.readouterr()


def test_evaluate_folder_saves_sr_images_on_the_cpu(tmp_path, capsys):
    lq_dir, lqs = _folder(tmp_path, "lq", [(12, 16), (10, 14)], seed=1)
    gt_dir, gts = _folder(tmp_path, "Set5", [(24, 32), (20, 28)], seed=2)
    model = tiny_model(scale=2, seed=3)
    save = tmp_path / "results"
    plain = EV.evaluate_folder(model, str(lq_dir), str(gt_dir), 2, device="cpu", verbose=False)
    said = capsys.readouterr().out
    saved = EV.evaluate_folder(model, str(lq_dir), str(gt_dir), 2, device="cpu", verbose=False, save_dir=str(save), save_gt=True)
    assert saved == plain and said == capsys.readouterr().out == ""
    folder = save / "X2" / "Set5"
    assert sorted(os.listdir(folder)) == sorted(f"im{i}_{k}.png" for i in range(2) for k in ("LQ", "HQ", "GT"))
    for i in range(2):
        lq = torch.from_numpy(lqs[f"im{i}"])
        assert torch.equal(read_png(folder / f"im{i}_LQ.png"), lq.repeat_interleave(2, 0).repeat_interleave(2, 1))
        assert torch.equal(read_png(folder / f"im{i}_GT.png"), torch.from_numpy(gts[f"im{i}"]))
        with torch.no_grad():
            want = I.pack8(model(lq.permute(2, 0, 1)[None].float().div(255)))[0]
        assert torch.equal(read_png(folder / f"im{i}_HQ.png"), want)
    # without --save-gt there is no _GT; the printed lines are those of a run without --save-dir
    EV.evaluate_folder(model, str(lq_dir), str(gt_dir), 2, device="cpu")
    lines = capsys.readouterr().out
    EV.evaluate_folder(model, str(lq_dir), str(gt_dir), 2, device="cpu", save_dir=str(tmp_path / "r2"))
    assert capsys.readouterr().out == lines
    assert sorted(os.listdir(tmp_path / "r2" / "X2" / "Set5")) == sorted(f"im{i}_{k}.png" for i in range(2) for k in ("LQ", "HQ"))
    a = EV._parser().parse_args(["--gt", "x", "--lq", "y", "--save-dir", "z", "--save-gt"])
    assert a.save_dir == "z" and a.save_gt is True
    assert EV._parser().parse_args(["--gt", "x"]).save_dir is None
