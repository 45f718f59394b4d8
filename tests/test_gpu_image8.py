"""The 8-bit pack on the MI355X (csrc/image8.hip through image8.pack8), the writer on CUDA tensors, and the two commands that save
images -- needs the GPU.  Everything is integer equality: against tests/golden/tasks/image8.npz (the reference's own rounding) and
against the CPU restatement ``image8._torch_pack8``."""
import ctypes as C
import os

import pytest
import torch

from grl_image_restoration_amd import GRL, _lib, evaluate as EV, image8 as I, make_config, restore, tasks as T, tiling
from oracle import grl_oracle as O
from tests.test_gpu_jpeg import _folder
from tests.test_image8 import adversarial_values, image8_case, image8_cases, read_png

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def adversarial(shape, start=0):
    """``shape`` filled cyclically with the fixture's value set (every level, every tie and its neighbours, the specials)."""
    v = adversarial_values()
    n = 1
    for s in shape:
        n *= s
    return v[(torch.arange(n) * 7 + start) % v.numel()].reshape(shape).contiguous()       # 7 and 1033 are coprime: every value is met


def check(x, rep=1):
    got = I.pack8(x.to(DEV), rep)
    torch.cuda.synchronize()
    want = I._torch_pack8(x, rep)
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and got.shape == want.shape
    assert torch.equal(got.cpu(), want), (tuple(x.shape), rep, int((got.cpu() != want).sum()))
    return got


@pytest.mark.parametrize("name", image8_cases())
def test_hip_pack8_equals_the_fixture_and_the_cpu_restatement(name):
    x, rep, want = image8_case(name)
    got = check(x, rep)
    assert torch.equal(got.cpu(), want), name


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 1, 9, 13), (1, 3, 67, 129)], ids=lambda s: "x".join(map(str, s)))
def test_unaligned_images_tails_and_several_workgroups(shape):
    """105 bytes per image with a tail of 2; gray with a tail of 1; 25929 bytes: 26 workgroups, the last one partly filled."""
    for start in (0, 400):
        check(adversarial(shape, start))


def test_a_strided_view_is_packed_in_place():
    base = adversarial((1, 3, 12, 19), 5).to(DEV)
    view = base[..., 1:10, 2:17]
    assert not view.is_contiguous()
    got = I.pack8(view)
    assert torch.equal(got, I.pack8(view.contiguous())) and torch.equal(got.cpu(), I._torch_pack8(view.cpu(), 1))
    got = I.pack8(view, 3)
    assert torch.equal(got.cpu(), I._torch_pack8(view.cpu(), 3))
    cl = adversarial((2, 3, 6, 10), 9).to(DEV).contiguous(memory_format=torch.channels_last)
    assert torch.equal(I.pack8(cl).cpu(), I._torch_pack8(cl.cpu(), 1))


@pytest.mark.parametrize("rep", [2, 3, 4, 8])
def test_replication(rep):
    """rep = 3 on five columns: 45-byte rows."""
    shapes = [(1, 3, 2, 3)] if rep == 8 else [(1, 3, 4, 5), (1, 1, 3, 3)]
    for shape in shapes:
        for start in (0, 256, 700):
            check(adversarial(shape, start), rep)


def test_nan_gives_zero():
    x = torch.full((1, 3, 5, 7), float("nan"))
    x[0, 2, 4, 6] = 0.5
    got = check(x, 2).cpu()
    assert int(got.sum()) == 4 * 128 and int((got != 0).sum()) == 4


def test_bad_arguments_raise_without_a_fault():
    x = adversarial((2, 3, 5, 7)).to(DEV)
    with pytest.raises(TypeError):
        I.pack8(x.half())
    with pytest.raises(ValueError):
        I.pack8(x[:, :2])
    with pytest.raises(ValueError):
        I.pack8(x, 9)
    L = _lib.lib()
    out = torch.zeros(2 * 5 * 7 * 3 + 8, dtype=torch.uint8, device=DEV)
    good = dict(x=x.data_ptr(), stride=(C.c_int64 * 4)(*x.stride()), N=2, C=3, H=5, W=7, rep=1, out=out.data_ptr())
    call = lambda **kw: L.grl_image_pack8(_lib.stream_ptr(), C.byref(_lib.GrlPack8Args(**dict(good, **kw))))
    for kw in (dict(x=None), dict(out=None), dict(C=2), dict(C=4), dict(N=0), dict(N=-1), dict(H=0), dict(H=-3), dict(W=0), dict(W=-1),
               dict(rep=0), dict(rep=9), dict(out=out.data_ptr() + 1), dict(x=x.data_ptr() + 2),
               dict(N=1 << 15, H=1 << 10, W=1 << 10),                                   # 3 * 2^35 bytes
               dict(N=1, C=1, H=1 << 15, W=1 << 16),                                    # exactly 2^31 bytes
               dict(H=(1 << 31) - 1, W=(1 << 31) - 1, N=(1 << 31) - 1, rep=8)):         # nothing overflows on the way to the refusal
        assert call(**kw) == -1, kw
    assert L.grl_image_pack8(_lib.stream_ptr(), None) == -1
    torch.cuda.synchronize()
    assert int(out.sum()) == 0                                                           # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out[: 2 * 5 * 7 * 3].view(2, 5, 7, 3).cpu(), I._torch_pack8(x.cpu(), 1)) and int(out[210:].sum()) == 0


def test_launch_names_the_entry_point_it_called():
    """_lib.launch checks the return code under the name it looked up: the library refuses the null pointers before any launch."""
    with pytest.raises(RuntimeError, match="grl_image_pack8 failed: bad argument"):
        _lib.launch("grl_image_pack8", _lib.GrlPack8Args())


def test_image_writer_on_cuda_tensors_reuses_its_buffers(tmp_path):
    """Eight images through two workers and four staging buffers; an image is overwritten on the device right after its write."""
    g = torch.Generator().manual_seed(4)
    imgs = [torch.rand(1, 3, 96, 128, generator=g) * 1.2 - 0.1 for _ in range(8)]
    dev = torch.empty_like(imgs[0], device=DEV)
    with I.ImageWriter(workers=2, compress_level=1) as w:
        for i, im in enumerate(imgs):
            dev.copy_(im)
            w.write(str(tmp_path / f"im{i}.png"), dev)
            w.write(str(tmp_path / f"im{i}_x2.png"), dev[..., 3:51, 5:69], rep=2)         # a view, the same 36864 bytes
        made = w.staging_allocated
    assert 1 <= made <= 4, made
    for i, im in enumerate(imgs):
        assert torch.equal(read_png(tmp_path / f"im{i}.png"), I._torch_pack8(im, 1)[0]), i
        assert torch.equal(read_png(tmp_path / f"im{i}_x2.png"), I._torch_pack8(im[..., 3:51, 5:69], 2)[0]), i
    assert len(os.listdir(tmp_path)) == 16


def test_evaluate_folder_jpeg_saves_images(tmp_path, capsys):
    d, imgs = _folder(tmp_path)
    model = GRL(**make_config("tiny", "dm", depths=[1], num_heads_window=[2], num_heads_stripe=[2])).eval()
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, 1)
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    save = tmp_path / "results"
    with torch.no_grad():
        plain = EV.evaluate_folder(model, None, str(d), 1, device=DEV, task="jpeg", quality=10, verbose=False)
        saved = EV.evaluate_folder(model, None, str(d), 1, device=DEV, task="jpeg", quality=10, verbose=False, save_dir=str(save),
                                   save_gt=True)
        grp = EV.evaluate_folder(model, None, str(d), 1, device=DEV, task="jpeg", quality=10, metric_group="restorer_jpeg", verbose=False)
        grp_saved = EV.evaluate_folder(model, None, str(d), 1, device=DEV, task="jpeg", quality=10, metric_group="restorer_jpeg",
                                       verbose=False, save_dir=str(tmp_path / "again"))
    assert saved == plain and grp_saved == grp and capsys.readouterr().out == ""
    folder = save / "QF10" / "live1"
    assert sorted(os.listdir(folder)) == sorted(f"im{i}_{k}.png" for i in range(2) for k in ("LQ", "HQ", "GT"))
    for i, im in enumerate(imgs):
        gt = torch.from_numpy(im).permute(2, 0, 1)[None].float().div(255).to(DEV)
        lq = T.jpeg_roundtrip(gt, 10)
        with torch.no_grad():
            want = I.pack8(model(lq).float())[0].cpu()
        assert torch.equal(read_png(folder / f"im{i}_HQ.png"), want), i
        assert torch.equal(read_png(folder / f"im{i}_LQ.png"), I.pack8(lq)[0].cpu()), i
        assert torch.equal(read_png(folder / f"im{i}_GT.png"), torch.from_numpy(im)), i


def test_restore_main_tiled(tmp_path, capsys):
    from PIL import Image

    g = torch.Generator().manual_seed(6)
    im = torch.randint(0, 256, (37, 53, 3), generator=g, dtype=torch.uint8)
    d = tmp_path / "lq"
    d.mkdir()
    Image.fromarray(im.numpy()).save(d / "photo.png")
    torch.manual_seed(0)
    paths = restore.main(["--lq", str(d), "--out", str(tmp_path / "out"), "--model", "tiny", "--geometry", "yaml", "--depths", "1",
                          "--tile", "16", "--overlap", "4", "--workers", "1"])
    capsys.readouterr()
    assert paths == [str(tmp_path / "out" / "photo_HQ.png")]
    heads = make_config("tiny", "yaml")["num_heads_window"][0]
    torch.manual_seed(0)
    model = GRL(**make_config("tiny", "yaml", upscale=1, depths=[1], num_heads_window=[heads], num_heads_stripe=[heads])).eval().to(DEV)
    lq = im.permute(2, 0, 1)[None].float().div(255).to(DEV)
    with torch.no_grad():
        want = I.pack8(tiling.forward_tiled(model, lq, 16, 4, 1).float())[0].cpu()
    assert want.shape == (37, 53, 3) and torch.equal(read_png(paths[0]), want)
