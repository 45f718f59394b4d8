"""The JPEG artifact-removal front end on the CPU (tasks.py, data.py, the two CLIs).  ``tasks.jpeg_roundtrip`` restates libjpeg's
integer arithmetic, so every comparison with the library is ``torch.equal``: against Pillow's bundled libjpeg-turbo run live
(skipped only when this Pillow is built on another libjpeg), and against tests/golden/tasks/jpeg_roundtrip.npz, which
tools/make_jpeg_golden.py wrote from the same library (never skipped).  OpenCV, which the reference calls
(data/datasets/restoration_jpeg.py:62-79), runs libjpeg-turbo with the same defaults: 4:2:0, JDCT_ISLOW, baseline tables, fancy
upsampling."""
import io
import os
import random

import numpy as np
import pytest
import torch

from grl_image_restoration_amd import PatchSampler, PatchStore, _lib, data as D, evaluate as EV, tasks as T, train
from tests.test_tasks import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (8, 8), (9, 17), (16, 16), (24, 31), (37, 53), (50, 16), (64, 64)]
QUALITIES = [1, 10, 40, 50, 75, 100]
KINDS = ["noise", "ramp", "checker1", "checker8", "binary"]


def turbo():
    from PIL import features

    return bool(features.check("libjpeg_turbo"))


def pillow_roundtrip(img, quality):
    """(H, W, C) uint8 -> what Pillow decodes after saving it as JPEG at ``quality``, (H, W, C) uint8."""
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(img[:, :, 0] if img.shape[2] == 1 else img).save(buf, format="JPEG", quality=int(quality))
    buf.seek(0)
    out = np.asarray(Image.open(buf))
    return out[:, :, None] if out.ndim == 2 else out


def pattern(kind, H, W, C, rng):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":
        a = rng.randint(0, 256, (H, W, C))
    elif kind == "binary":
        a = rng.randint(0, 2, (H, W, C)) * 255
    elif kind == "ramp":
        a = np.stack([(3 * yy + 2 * xx + 40 * c) % 256 for c in range(C)], 2)
    else:
        s = int(kind[-1])
        a = np.repeat((((yy // s + xx // s) % 2) * 255)[:, :, None], C, 2)
    return a.astype(np.uint8)


def to_batch(imgs):
    """[(H, W, C) uint8] -> (N, C, H, W) fp32 k / 255."""
    return torch.from_numpy(np.stack(imgs)).permute(0, 3, 1, 2).float().div(255).contiguous()


def levels(x):
    """fp32 k / 255 -> uint8 k, asserting that every value is such a level exactly."""
    k = (x * 255).round()
    assert torch.equal(k / 255, x)
    return k.to(torch.uint8)


_FIXTURE = {}


def jpeg_cases():
    return [c["name"] for c in golden("jpeg_roundtrip")[0]["cases"]]


def jpeg_case(name):
    """(meta, x fp32 (3, C, H, W), qualities, Pillow's output uint8), loaded once and shared with the GPU tests."""
    if not _FIXTURE:
        meta, z = golden("jpeg_roundtrip")
        for c in meta["cases"]:
            _FIXTURE[c["name"]] = (c, z[c["name"] + "__x"].float().div(255), list(c["quality"]), z[c["name"] + "__y"])
    return _FIXTURE[name]


@pytest.mark.skipif(not turbo(), reason="this Pillow is not built on libjpeg-turbo")
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("channels", [3, 1])
def test_torch_jpeg_equals_live_pillow(size, channels):
    """Every size x pattern x quality: one batched call per quality over the five patterns."""
    H, W = size
    rng = np.random.RandomState(H * 100 + W + channels)
    imgs = [pattern(k, H, W, channels, rng) for k in KINDS]
    x = to_batch(imgs)
    for q in QUALITIES:
        got = levels(T.jpeg_roundtrip(x, q))
        want = torch.from_numpy(np.stack([pillow_roundtrip(im, q) for im in imgs])).permute(0, 3, 1, 2)
        assert got.shape == want.shape and torch.equal(got, want), (size, channels, q, int((got != want).sum()))


@pytest.mark.parametrize("name", jpeg_cases())
def test_torch_jpeg_equals_the_fixture(name):
    c, x, quality, want = jpeg_case(name)
    got = T.jpeg_roundtrip(x, quality)                                         # three qualities in one call
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(levels(got), want), name
    assert torch.equal(T.jpeg_roundtrip(x, torch.tensor(quality, dtype=torch.int32)), got)
    assert torch.equal(T.jpeg_roundtrip(x[1:2], quality[1]), got[1:2])         # a sample does not depend on its batch


def test_fixture_covers_the_edge_rules():
    meta, _ = golden("jpeg_roundtrip")
    sizes = {tuple(c["size"]) for c in meta["cases"]}
    assert {(1, 1), (8, 8), (9, 17), (24, 31), (50, 16), (37, 53), (64, 64), (20, 4)} <= sizes
    assert {c["channels"] for c in meta["cases"]} == {1, 3}
    b = next(c for c in meta["cases"] if c["name"] == "64x64_c3_b")
    assert b["kinds"][:2] == ["checker1", "checker1"] and b["quality"][:2] == [100, 1]
    # the compression is not the identity and depends on the quality
    _, x, q, y = jpeg_case("64x64_c3_a")
    assert not torch.equal(levels(x), y)
    assert not torch.equal(T.jpeg_roundtrip(x[:1], 10), T.jpeg_roundtrip(x[:1], 11))


def test_quality_is_clamped_and_arguments_are_checked():
    _, x, _, _ = jpeg_case("9x17_c3_a")
    assert torch.equal(T.jpeg_roundtrip(x, 0), T.jpeg_roundtrip(x, 1))
    assert torch.equal(T.jpeg_roundtrip(x, [-5, 100, 1000]), T.jpeg_roundtrip(x, [1, 100, 100]))
    assert torch.equal(T.jpeg_tables(0), T.jpeg_tables(1)) and torch.equal(T.jpeg_tables(101), T.jpeg_tables(100))
    assert int(T.jpeg_tables(100).max()) == 1 and int(T.jpeg_tables(1).min()) == 255
    with pytest.raises(ValueError):
        T.jpeg_roundtrip(x, [10, 20])                                          # two qualities for three samples
    with pytest.raises(ValueError):
        T.jpeg_roundtrip(x[0], 10)
    with pytest.raises(ValueError):
        T.jpeg_roundtrip(x[:, :2], 10)                                         # two channels
    with pytest.raises(TypeError):
        T.jpeg_roundtrip(x.double(), 10)
    with pytest.raises(TypeError):
        T.jpeg_roundtrip(x, torch.tensor([1.0, 2.0, 3.0]))


@pytest.mark.skipif(not turbo(), reason="this Pillow is not built on libjpeg-turbo")
def test_tables_are_the_decoded_files():
    from PIL import Image

    img = pattern("noise", 16, 16, 3, np.random.RandomState(0))
    for q in (1, 5, 10, 37, 49, 50, 51, 75, 95, 100):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="JPEG", quality=q)
        buf.seek(0)
        qt = Image.open(buf).quantization
        natural = T.jpeg_tables(q)
        assert natural.shape == (2, 64) and natural.dtype == torch.int64
        for k in (0, 1):
            assert list(qt[k]) == natural[k].tolist(), (q, k)


def test_jpeg_args_layout_matches_header_and_abi():
    """The layout of GrlJpegArgs is compared with the header in tests/test_abi.py, like every struct's;
    what is particular to this entry point stays here."""
    assert _lib.ABI_VERSION >= 29
    assert "grl_jpeg_roundtrip" in _lib.EXPORTS and "grl_jpeg_workspace_bytes" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "grl_hip.h")).read()
    assert "restoration_jpeg.py:62-79" in header


def test_task_inputs_jpeg_on_the_cpu(tmp_path):
    """evaluate's jpeg items from a folder with odd sizes: the GT is not cropped, the LQ is the library's."""
    from PIL import Image

    rng = np.random.RandomState(3)
    imgs = {"a.png": pattern("noise", 37, 53, 3, rng), "b.png": pattern("ramp", 9, 17, 3, rng)}
    for n, im in imgs.items():
        Image.fromarray(im).save(tmp_path / n)
    items = list(EV.task_inputs(str(tmp_path), "jpeg", quality=10, device="cpu"))
    assert [n for n, _, _ in items] == ["a.png", "b.png"]
    for name, lq, gt in items:
        assert torch.equal(gt, to_batch([imgs[name]])) and lq.shape == gt.shape            # uncropped
        want = pillow_roundtrip(imgs[name], 10) if turbo() else None
        if want is not None:
            assert torch.equal(levels(lq), torch.from_numpy(want.copy()).permute(2, 0, 1)[None]), name
        assert torch.equal(lq, T.jpeg_roundtrip(gt, 10))
    gray = list(EV.task_inputs(str(tmp_path), "jpeg", channels=1, quality=30, device="cpu"))
    assert gray[0][1].shape == (1, 1, 37, 53)
    for bad in (None, 0, 101):
        with pytest.raises(ValueError):
            list(EV.task_inputs(str(tmp_path), "jpeg", quality=bad, device="cpu"))


STORE_SIZES = [(40, 52), (12, 30)]                 # with P = 16 the second one is zero padded at the bottom


def store_images(channels=3):
    g = np.random.RandomState(33)
    return [pattern("noise" if i else "ramp", h, w, channels, g) for i, (h, w) in enumerate(STORE_SIZES)]


WORK = [(1, 0, 0, 0), (1, 0, 14, 3), (0, 24, 36, 0), (0, 5, 7, 4), (0, 3, 1, 6)]


def test_jpeg_sampler_with_a_fixed_quality_on_a_cpu_store():
    imgs = store_images()
    P, B = 16, len(WORK)
    s = PatchSampler("jpeg", PatchStore(imgs), patch=P, batch=B, quality=10, seed=5)
    assert s.lq_store is not None and s.lq_store.dims == s.gt_store.dims and s.qualities is None
    whole = [levels(T.jpeg_roundtrip(to_batch([im]), 10))[0].permute(1, 2, 0) for im in imgs]     # compressed as a whole, once
    for n in range(2):
        assert torch.equal(s.lq_store.image(n), whole[n])
    lq, gt = s.next(WORK)
    assert lq.shape == gt.shape == (B, 3, P, P)
    for b, (n, x, y, flags) in enumerate(WORK):
        for got, img in ((lq[b], whole[n]), (gt[b], torch.from_numpy(imgs[n]))):
            crop = torch.zeros(P, P, 3, dtype=torch.uint8)
            h, w = min(P, img.shape[0] - x), min(P, img.shape[1] - y)
            crop[:h, :w] = img[x : x + h, y : y + w]                              # zero padded AFTER the compression
            if flags & 1:
                crop = crop.flip(0)
            if flags & 2:
                crop = crop.flip(1)
            if flags & 4:
                crop = crop.transpose(0, 1)
            assert torch.equal(levels(got), crop.permute(2, 0, 1)), (b, n)
    assert float(lq[0, :, 12:].abs().max()) == 0 and float(gt[0, :, 12:].abs().max()) == 0      # image 1 has 12 rows
    assert not torch.equal(lq, gt)
    # a patch at an odd phase of the 8 x 8 grid is not what compressing the patch gives
    assert not torch.equal(lq[3:4], T.jpeg_roundtrip(gt[3:4], 10))
    # the draws are the plain ones: nothing is drawn for the quality
    got, second = s.draw()
    rng = random.Random(5)
    want = []
    for _ in range(B):
        n = rng.randrange(2)
        x, y = rng.randrange(0, max(STORE_SIZES[n][0], P) - P + 1), rng.randrange(0, max(STORE_SIZES[n][1], P) - P + 1)
        want.append((n, x, y, sum(bit for bit in (1, 2, 4) if rng.random() < 0.5)))
    assert got == want and second is None
    gray = PatchSampler("jpeg", PatchStore(store_images(1)), patch=P, batch=2, quality=40)
    assert gray.next()[0].shape == (2, 1, P, P)


def test_jpeg_sampler_with_a_quality_range_on_a_cpu_store():
    imgs = store_images()
    P, B, seed, lo, hi = 16, len(WORK), 11, 10, 40
    s = PatchSampler("jpeg", PatchStore(imgs), patch=P, batch=B, quality_range=(lo, hi), seed=seed)
    assert s.lq_store is None and s.qualities.dtype == torch.int32 and s.qualities.shape == (B,)
    # the draw order: image, row, column, three flips, then the quality -- the place sigma_range's draw has
    state = s.rng_state()
    work, quals = s.draw()
    rng = random.Random(seed)
    want_w, want_q = [], []
    for _ in range(B):
        n = rng.randrange(2)
        x, y = rng.randrange(0, max(STORE_SIZES[n][0], P) - P + 1), rng.randrange(0, max(STORE_SIZES[n][1], P) - P + 1)
        want_w.append((n, x, y, sum(bit for bit in (1, 2, 4) if rng.random() < 0.5)))
        want_q.append(rng.randint(lo, hi))
    assert work == want_w and quals == want_q
    many = [q for _ in range(40) for q in s.draw()[1]]
    assert min(many) >= lo and max(many) <= hi and len(set(many)) > 10 and all(isinstance(q, int) for q in many)
    # crop and augment first, then compress the patch
    quals = [10, 25, 40, 33, 17]
    lq, gt = s.next(WORK, quals)
    assert torch.equal(gt, PatchStore(imgs).sample(torch.tensor(WORK, dtype=torch.int32), P, 1))
    assert torch.equal(lq, T.jpeg_roundtrip(gt, quals)) and s.qualities.tolist() == quals
    for b in range(B):
        assert torch.equal(lq[b : b + 1], T.jpeg_roundtrip(gt[b : b + 1], quals[b]))
    with pytest.raises(ValueError):
        s.next(WORK)                                                           # an explicit list needs its qualities
    # the state round trip continues the stream of batches
    s.set_rng_state(state)
    assert s.draw() == (want_w, want_q)
    a = s.next()
    mid = s.rng_state()
    b = s.next()
    s.set_rng_state(mid)
    c = s.next()
    assert torch.equal(b[0], c[0]) and torch.equal(b[1], c[1]) and not torch.equal(a[1], b[1])


def test_jpeg_sampler_argument_errors():
    st = PatchStore(store_images())
    with pytest.raises(ValueError):
        PatchSampler("jpeg", st, patch=16, batch=2)                            # neither
    with pytest.raises(ValueError):
        PatchSampler("jpeg", st, patch=16, batch=2, quality=10, quality_range=(10, 40))
    with pytest.raises(ValueError, match="recompress"):
        PatchSampler("jpeg", st, patch=16, batch=2, quality_range=(10, 40), patchwise=False)
    for bad in ((0, 40), (40, 10), (10, 101), (10,)):
        with pytest.raises(ValueError):
            PatchSampler("jpeg", st, patch=16, batch=2, quality_range=bad)
    for bad in (0, 101):
        with pytest.raises(ValueError):
            PatchSampler("jpeg", st, patch=16, batch=2, quality=bad)
    with pytest.raises(ValueError):
        PatchSampler("jpeg", st, patch=16, batch=2, quality=10, scale=2)
    with pytest.raises(ValueError):
        PatchSampler("jpeg", st, st, patch=16, batch=2, quality=10)
    with pytest.raises(ValueError):
        PatchSampler("jpeg", st, patch=16, batch=2, quality=10, sigma=3)
    with pytest.raises(ValueError):
        PatchSampler("dn", st, patch=16, batch=2, sigma=3, quality=10)


def test_task_lists_and_cli_errors(tmp_path, capsys):
    assert "jpeg" in EV.TASKS and "jpeg" in D.TASKS
    gt = tmp_path / "gt"
    gt.mkdir()
    ev = ["--task", "jpeg", "--gt", str(gt), "--device", "cpu"]
    for extra in ([], ["--quality", "0"], ["--quality", "101"], ["--quality", "10", "--scale", "2"], ["--quality", "10", "--lq", str(gt)],
                  ["--quality", "ten"]):
        with pytest.raises(SystemExit) as e:
            EV.main(ev + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit):
        EV.main(["--task", "dm", "--gt", str(gt), "--quality", "10"])            # the option belongs to jpeg
    for extra in ([], ["--channels", "1"]):                                    # accepted by the parser; the empty folder stops it
        with pytest.raises(ValueError, match="no images"):
            EV.main(ev + ["--quality", "10", "--model", "tiny", "--geometry", "yaml"] + extra)
    tr = ["--task", "jpeg", "--gt", str(gt), "--steps", "1", "--device", "cpu"]
    for extra in ([], ["--quality", "0"], ["--quality-range", "40", "10"], ["--quality-range", "0", "10"], ["--quality", "10", "--scale", "2"],
                  ["--quality", "10", "--lq", str(gt)], ["--quality", "10", "--sigma", "3"], ["--quality", "10", "--val-lq", str(gt)],
                  ["--quality-range", "10", "40", "--val-gt", str(gt), "--val-every", "1"]):
        with pytest.raises(SystemExit) as e:
            train.main(tr + extra)
        assert e.value.code == 2, extra
    with pytest.raises(SystemExit):
        train.main(["--task", "dm", "--gt", str(gt), "--steps", "1", "--device", "cpu", "--quality", "10"])
    ap = train._parser()
    a = ap.parse_args(tr + ["--quality-range", "10", "40", "--quality", "10", "--val-gt", str(gt), "--val-every", "1"])
    train._check(ap, a)
    assert a.scale == 1 and a.quality == 10 and a.quality_range == [10, 40]
    capsys.readouterr()


def test_train_cli_jpeg_on_the_cpu(tmp_path, capsys):
    """One eager step and one validation of --task jpeg on CPU tensors, in both modes."""
    from PIL import Image

    g = np.random.RandomState(4)
    d = tmp_path / "gt"
    d.mkdir()
    for i in range(2):
        Image.fromarray(g.randint(0, 256, (24, 31, 3)).astype(np.uint8)).save(d / f"im{i}.png")
    common = ["--task", "jpeg", "--model", "tiny", "--geometry", "yaml", "--depths", "1", "--patch", "16", "--batch", "2", "--eager",
              "--device", "cpu", "--gt", str(d), "--steps", "1", "--val-gt", str(d), "--val-every", "1"]
    for mode, extra in (("fixed", ["--quality", "10"]), ("range", ["--quality-range", "10", "40", "--quality", "10"])):
        torch.manual_seed(0)
        r = train.main(common + extra + ["--out", str(tmp_path / mode)])
        assert r["steps"] == [0] and np.isfinite(r["losses"][0]) and os.path.isfile(r["checkpoint"])
        assert len(r["val"]) == 1 and r["val"][0][0] == 1 and np.isfinite(r["val"][0][1])
        obj = torch.load(r["checkpoint"], map_location="cpu", weights_only=False)
        assert obj["args"]["task"] == "jpeg" and obj["args"]["quality"] == 10
    capsys.readouterr()
