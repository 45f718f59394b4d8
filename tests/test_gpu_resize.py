"""grl_imresize (csrc/imresize.hip) through tasks.py on the MI355X: against the reference fixture through contiguous, cropped and
channels-last inputs, against the CPU path on large and ragged sizes (and on the direct path of very small scales), on bad arguments;
GRL-Tiny x2 on the LQ made on the device from the fixture GT; and the evaluate CLI's sr_bicubic task end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import GRL, _lib, evaluate as EV, metrics as M, tasks as T
from oracle import grl_oracle as O
from tests.test_gpu_tasks import _check_cli
from tests.test_resize import resize_cases
from tests.test_tasks import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the kernel holds the row pass in fp64 and rounds once; the bar allows the two fp32 roundings of an fp32 strip (2 x 2^-24 below 2)
BAR = 2.4e-7


@pytest.mark.parametrize("name", resize_cases())
def test_hip_imresize_matches_reference(name):
    meta, z = golden("imresize")
    c, x = meta["cases"][name], z[f"{name}__in"]
    exact, ref32 = z[f"{name}__ref64"].float(), z[f"{name}__ref32"]
    N, Cn, H, W = x.shape
    big = torch.rand(N, Cn + 2, H + 3, W + 5).to(DEV)
    big[:, 1 : 1 + Cn, 2 : 2 + H, 3 : 3 + W] = x.to(DEV)
    outs = {
        "contiguous": T.imresize(x.to(DEV), c["scale"], c["antialiasing"]),
        "view": T.imresize(big[:, 1 : 1 + Cn, 2 : 2 + H, 3 : 3 + W], c["scale"], c["antialiasing"]),   # a crop of a larger tensor
        "channels_last": T.imresize(x.to(DEV).to(memory_format=torch.channels_last), c["scale"], c["antialiasing"]),
    }
    for k, got in outs.items():
        assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and got.shape == exact.shape, k
        got = got.cpu()
        d64, d32 = (got - exact).abs().max().item(), (got - ref32).abs().max().item()
        print(f"{name} {k}: |hip - ref64| = {d64:.3e}, |hip - ref32| = {d32:.3e}")
        assert d64 <= BAR and d32 <= c["ref32_vs_ref64"] + BAR, (k, d64, d32)


@pytest.mark.parametrize("shape,scale", [((2, 3, 1080, 1920), 1 / 4), ((1, 3, 263, 1001), 1 / 3), ((1, 3, 263, 1001), 1 / 2),
                                         ((1, 2, 131, 77), 4), ((1, 1, 200, 240), 1 / 40)])
def test_hip_matches_cpu_path(shape, scale):
    """Full HD at 1/4; partial tiles in both directions of a grid with several tiles each way; upsampling; and 1/40, whose 160
    taps fit no LDS tile, so the kernel's direct path runs."""
    x = torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(12)).float() / 255
    want = T.imresize(x, scale)
    got = T.imresize(x.to(DEV), scale)
    d = (got.cpu() - want).abs().max().item()
    print(f"{shape} x {scale:.4f}: |hip - cpu| = {d:.3e}")
    assert got.shape == want.shape and d <= BAR
    q = T.imresize(x.to(DEV), scale, quantize=True)
    assert torch.equal(q.cpu(), EV.tensor_round(got.cpu()))        # on the CPU, where the reference rounds its LQ


def test_quantize_clamps_like_tensor_round():
    x = (torch.rand(1, 3, 40, 52, generator=torch.Generator().manual_seed(2)) * 3 - 1).to(DEV)
    plain = T.imresize(x, 2)
    assert float(plain.min()) < 0 and float(plain.max()) > 1
    assert torch.equal(T.imresize(x, 2, quantize=True).cpu(), EV.tensor_round(plain.cpu()))


def test_foreign_tables_take_the_direct_path():
    """Tables whose indices spread over the whole image (a random permutation per tap) exceed every LDS window."""
    g = torch.Generator().manual_seed(4)
    x = torch.rand(1, 2, 300, 500, generator=g)
    ih = torch.stack([torch.randperm(300, generator=g)[:40] for _ in range(3)], 1).int()        # (40, 3)
    iw = torch.stack([torch.randperm(500, generator=g)[:70] for _ in range(2)], 1).int()        # (70, 2)
    wh, ww = torch.rand(40, 3, generator=g, dtype=torch.float64), torch.rand(70, 2, generator=g, dtype=torch.float64)
    want = T._torch_resize(x, (wh, ih), (ww, iw)).float()
    got = T.hip_resize(x.to(DEV), (wh.to(DEV), ih.to(DEV)), (ww.to(DEV), iw.to(DEV)))
    assert (got.cpu() - want).abs().max() <= 4 * BAR            # values up to 6: four times the rounding step of values below 2


def test_bad_arguments():
    x = torch.rand(1, 3, 16, 16, device=DEV)
    with pytest.raises(TypeError):
        T.imresize(x.half(), 1 / 2)
    with pytest.raises(ValueError):
        T.imresize(x[..., :5], 1 / 4)
    L = _lib.lib()
    rows = T._device_tables((16, 8, 0.5, True), x.device)
    out = torch.empty(1, 3, 8, 8, device=DEV)

    def call(**kw):
        a = dict(src=x.data_ptr(), stride=(C.c_int64 * 4)(*x.stride()), N=1, C=3, H=16, W=16, out_h=8, out_w=8,
                 taps_h=rows[0].shape[1], taps_w=rows[0].shape[1], wh=rows[0].data_ptr(), ih=rows[1].data_ptr(),
                 ww=rows[0].data_ptr(), iw=rows[1].data_ptr(), out=out.data_ptr())
        a.update(kw)
        return L.grl_imresize(_lib.stream_ptr(), C.byref(_lib.GrlResizeArgs(**a)))

    assert call() == 0
    torch.cuda.synchronize()
    assert (out.cpu() - T.imresize(x.cpu(), 1 / 2)).abs().max() <= BAR
    for bad in (dict(src=None), dict(out=None), dict(wh=None), dict(ih=None), dict(ww=None), dict(iw=None), dict(N=0), dict(C=0),
                dict(H=0), dict(W=-1), dict(out_h=0), dict(out_w=0), dict(taps_h=0), dict(taps_w=0)):
        assert call(**bad) == -1, bad


def _pipeline_model():
    meta, z = golden("sr_pipeline")
    model = GRL(**meta["cfg"]).eval()
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, meta["weight_seed"])
    model.load_state_dict(sd, strict=True)
    return model, sd, z


def test_sr_pipeline_matches_reference():
    """GT -> sr_lq on the GPU -> GRL-Tiny x2 through the HIP path, against the reference network on the reference's LQ, at the bar
    of the tiny x2 fixtures (1e-3 max-abs).  The fixture's texture seed is one for which the reference's LQ has no 8-bit level off
    the float64 truth (tools/make_golden_resize.py prints the count), so the LQs agree level for level."""
    model, _, z = _pipeline_model()
    lq, gtc = T.sr_lq((z["gt"].float() / 255).to(DEV), 2)
    levels = ((lq.cpu().double() * 255).round() - (z["lq_x2"].double() * 255).round()).abs()
    print(f"LQ levels that differ from the reference's: {int((levels > 0).sum())}")
    assert levels.max() <= 1
    with torch.no_grad():
        out = model.to(DEV)(lq).float().cpu()
    d = (out - z["output"]).abs()
    print(f"max|hip - reference| = {d.max():.3e}  rms = {d.pow(2).mean().sqrt():.3e}")
    assert out.shape == z["output"].shape == (1, 3) + tuple(gtc.shape[-2:]) and d.max() < 1e-3, d.max()


def test_evaluate_cli_sr_bicubic(tmp_path, capsys):
    from PIL import Image

    model, sd, z = _pipeline_model()
    ck = tmp_path / "sr.ckpt"
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}}, ck)
    d = tmp_path / "set5"
    d.mkdir()
    Image.fromarray(z["gt"][0].permute(1, 2, 0).numpy()).save(d / "pipe.png")                   # 131 x 139: cropped to 130 x 138
    Image.fromarray(np.random.RandomState(3).randint(0, 256, (64, 80, 3)).astype(np.uint8)).save(d / "even.png")
    model = model.to(DEV)
    want = {}
    for name in ("even.png", "pipe.png"):
        lq, gt = T.sr_lq(EV._read_image(str(d / name)).to(DEV), 2)
        with torch.no_grad():
            sr = model(lq)
        want[name] = {k: float(v) for k, v in M.image_metrics(sr, gt, "restorer", 2).items()}
    got = EV.main(["--task", "sr_bicubic", "--scale", "2", "--model", "tiny", "--geometry", "sr_ckpt_df4", "--ckpt", str(ck),
                   "--gt", str(d), "--metric", "restorer"])
    _check_cli(got, capsys.readouterr().out, want)
