"""Writes tests/golden/niqe/{niqe_pris_params,niqe,bsr_pipeline}.npz: what the reference's NIQE reports, and its blind-SR network.

The values come from the UNMODIFIED reference module utils/metrics/niqe.py, imported from the reference tree (GRL_REFERENCE_ROOT, as
for oracle/refshim.py) with the two stand-ins of tools/make_golden_metrics.py in ``sys.modules``: ``cv2`` (imported, never called on
the Y path) and ``torchmetrics.Metric``.  It needs SciPy, as the reference does, and runs only where the reference tree exists.

  niqe_pris_params.npz   a byte copy of the reference's utils/metrics/niqe_pris_params.npz (the pristine model: user data, like a
                         checkpoint; the package ships no copy outside tests/golden/).  The recipe checks metrics.niqe_window()
                         against its ``gaussian_window``.
  niqe.npz               per case ``<name>``:
      <name>__input      the (B, C, H, W) image: uint8 levels (image = level / 255 in fp32) or int16 levels (same rule; levels
                         below 0 and above 255 give values outside [0, 1], which tensor_round clamps)
      <name>__ref32      (B,) what NaturalImageQualityEvaluator.update stores for tensor_round(image): fp32 internals
      <name>__distparam32  (B, blocks, 36) the feature matrix of that run
      <name>__ref64      (B,) float64 adjudication: the same niqe() on the same plane cast to float64, its half-scale image taken
                         from the reference's float64 tables summed in float64 (tools/make_golden_resize.py: ref64_resize)
      <name>__distparam64  (B, blocks, 36) the feature matrix of the adjudication
                         ``meta`` holds per case max |ref32 - ref64| and the count of features whose alpha differs between the two
                         runs, and ``y_mismatches``: metrics.niqe_plane against the reference's to_y_channel over all 2^24 colours
  bsr_pipeline.npz       seeded weights (grl_oracle.seeded_state_dict, seed 0) in a GRL-Tiny-width model at the bsr geometry with the
                         ``nearest+conv`` x4 tail, built through the product's make_config; the reference module loads the same
                         state dict.  ``lq`` (1, 3, 48, 64), ``output`` (fp32 reference), ``output64_ulps`` (the reference run in float64, rounded to fp32,
                         as its int32 distance from ``output`` in units of the last place),
                         ``niqe_output`` / ``niqe_output64``: the float64-adjudicated NIQE of the two outputs (192 x 256: 2 x 2 blocks);
                         ``meta["niqe_level_flip_spread"]``: how far that NIQE moves when the 8-bit levels within the model bar (1e-3 for precision
                         "auto", 1e-5 for "high") of a rounding boundary round the other way

    python tools/make_golden_niqe.py [--reference DIR] [--out tests/golden/niqe]
"""
import argparse
import json
import os
import shutil
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import grl_oracle as O  # noqa: E402
from oracle import refshim  # noqa: E402
from tools.make_golden_resize import ref64_resize  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "niqe")
BSR_OVERRIDES = dict(depths=[2, 2], num_heads_window=[2, 2], num_heads_stripe=[2, 2])


def _install_stubs():
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    if "torchmetrics" not in sys.modules:
        tm = types.ModuleType("torchmetrics")

        class Metric:
            def __init__(self, compute_on_step=None, **kwargs):
                pass

            def add_state(self, name, default, dist_reduce_fx=None):
                setattr(self, name, list(default))

        tm.Metric = Metric
        sys.modules["torchmetrics"] = tm


def texture(rs, C, H, W, smooth, lo=0.04, hi=0.96):
    """Seeded image-like texture (C, H, W) float64: low-pass noise at two scales, a few waves and hard edges; ``smooth`` is the
    Gaussian sigma of the fine layer (NIQE on white noise is not what users score).  Scaled into [lo, hi]: inside [0, 1], so that
    no 7 x 7 window saturates at 255 -- see ``flat_nonzero_windows``."""
    from scipy.ndimage import gaussian_filter

    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = gaussian_filter(rs.standard_normal((H, W)), 6 * smooth + 4)
    base = base / base.std()
    img = np.zeros((C, H, W))
    for c in range(C):
        fine = gaussian_filter(rs.standard_normal((H, W)), smooth)
        f = rs.uniform(0.02, 0.3, 3)
        img[c] = 0.5 + 0.17 * base + 0.1 * fine / fine.std() + 0.08 * np.sin(f[0] * x + f[1] * y) + 0.12 * ((x // 37 + y // 29) % 2 - 0.5)
        img[c] += 0.006 * rs.standard_normal((H, W))
    img = (img - img.min()) / (img.max() - img.min())
    return lo + (hi - lo) * img


def make_cases():
    """{name: integer levels (B, C, H, W)} -- deterministic, independent of the reference."""
    rs = np.random.RandomState(96)
    u8 = lambda a: np.clip(np.round(a * 255), 0, 255).astype(np.uint8)
    cases = {}
    cases["rgb_192x288"] = u8(texture(rs, 3, 192, 288, 1.0))[None]
    out = np.round(texture(rs, 1, 200, 301, 0.7) * 255).astype(np.int16)
    spikes = rs.uniform(size=out.shape)
    out[spikes < 0.01], out[spikes > 0.99] = -50, 320               # isolated samples outside [0, 1]: tensor_round clamps them
    cases["gray_200x301_outside"] = out[None]
    cases["rgb_b2_192x192"] = np.stack([u8(texture(rs, 3, 192, 192, 0.6)), u8(texture(rs, 3, 192, 192, 2.0))])
    cases["gray_384x480"] = u8(texture(rs, 1, 384, 480, 1.5))[None]
    big = texture(rs, 1, 480, 672, 0.9)
    big[:, 90:300, 280:500] = 0.0                                  # a black region that holds whole blocks: nan features
    cases["gray_480x672_flat"] = u8(big)[None]
    return cases


def flat_nonzero_windows(plane):
    """7 x 7 windows of the scored plane that are flat at a level other than 0.  There the reference's fp32 ``mu`` rounds to the
    level and MSCN is exactly 0, while the float64 run of the same lines leaves sum(w) * level - level = 3e-14 of one sign: the
    float64 adjudication means nothing for such windows (at level 0 both are exactly 0), so the fixtures have none."""
    from scipy.ndimage import maximum_filter, minimum_filter

    hi, lo = maximum_filter(plane, 7, mode="nearest"), minimum_filter(plane, 7, mode="nearest")
    return int(((hi == lo) & (hi != 0)).sum())


def to_image(levels):
    return torch.from_numpy(levels.astype(np.float32)) / 255.0


class Recorder:
    """Wraps the module's compute_feature to keep what niqe() concatenates into ``distparam``."""

    def __init__(self, N):
        self.N, self.orig, self.rows = N, N.compute_feature, []

    def __enter__(self):
        def wrapped(block):
            f = self.orig(block)
            self.rows.append(f)
            return f

        self.N.compute_feature = wrapped
        return self

    def __exit__(self, *exc):
        self.N.compute_feature = self.orig

    def distparam(self):
        a = np.array(self.rows, dtype=np.float64)
        n = a.shape[0] // 2
        return np.concatenate([a[:n], a[n:]], axis=1)


def ref_plane(N, p):
    """calculate_niqe (niqe.py:529-542) up to the plane it hands to niqe(), for one CHW image ``p * 255``."""
    img = (p * 255).astype(np.float32)
    img = N.reorder_image(img, input_order="CHW")
    img = np.squeeze(N.to_y_channel(img))
    return img.round()


def ref64(N, plane, params):
    """niqe() on the float64 plane, its imresize replaced by the float64 tables summed in float64."""
    orig = N.imresize
    N.imresize = lambda img, scale, antialiasing=True: ref64_resize(N, np.asarray(img, dtype=np.float64)[None], scale, antialiasing)[0]
    try:
        with Recorder(N) as rec, np.errstate(all="ignore"):
            v = N.niqe(plane.astype(np.float64), params["mu_pris_param"], params["cov_pris_param"], params["gaussian_window"])
        return v, rec.distparam()
    finally:
        N.imresize = orig


def build_niqe(N, U, params):
    arrays, meta = {}, {}
    for name, levels in make_cases().items():
        preds = U.tensor_round(to_image(levels).clone(), 1.0)
        v32, d32, v64, d64 = [], [], [], []
        for b in range(preds.shape[0]):
            m = N.NaturalImageQualityEvaluator()
            with Recorder(N) as rec, np.errstate(all="ignore"):
                m.update(preds[b : b + 1], None, idx=[b])
            v32.append(float(m.value[0][0]))
            d32.append(rec.distparam())
            plane = ref_plane(N, preds[b].numpy())
            assert flat_nonzero_windows(plane) == 0, name
            v, d = ref64(N, plane, params)
            v64.append(v)
            d64.append(d)
        d32, d64 = np.stack(d32), np.stack(d64)
        assert (np.isnan(d32) == np.isnan(d64)).all(), name
        alpha_cols = [0] + list(range(2, 18, 4)) + [18] + list(range(20, 36, 4))
        flips = int((d32[..., alpha_cols] != d64[..., alpha_cols]).sum())
        arrays[f"{name}__input"] = levels
        arrays[f"{name}__ref32"], arrays[f"{name}__ref64"] = np.array(v32, dtype=np.float32), np.array(v64)
        arrays[f"{name}__distparam32"], arrays[f"{name}__distparam64"] = d32, d64
        gap = float(np.abs(np.array(v32, dtype=np.float64) - np.array(v64)).max())
        meta[name] = dict(ref32_vs_ref64=gap, alpha_differs=flips, nan_rows=int(np.isnan(d64).any(-1).sum()), blocks=int(d64.shape[1]),
                          score=[float(x) for x in v64])
        print(f"{name}: NIQE {v64}  max|ref32 - ref64| = {gap:.3e}  alphas differing {flips}  nan rows {meta[name]['nan_rows']}")
    return arrays, meta


def y_mismatches(N):
    """metrics.niqe_plane against the reference's plane over all 2^24 colours."""
    from grl_image_restoration_amd.metrics import niqe_plane

    lv = np.arange(256, dtype=np.uint8)
    bad = 0
    for r0 in range(0, 256, 16):
        r, g, b = np.meshgrid(lv[r0 : r0 + 16], lv, lv, indexing="ij")
        p = to_image(np.stack([r.reshape(16 * 16, 4096), g.reshape(16 * 16, 4096), b.reshape(16 * 16, 4096)]))
        want = ref_plane(N, p.numpy())
        got = niqe_plane(p.unsqueeze(0))[0, 0].numpy()
        bad += int((want != got).sum())
    return bad


def build_bsr_pipeline(N, params):
    from grl_image_restoration_amd.presets import make_config
    from tools.make_golden_tasks import _texture

    cfg = make_config("tiny", "bsr", upscale=4, img_size=64, upsampler="nearest+conv", **BSR_OVERRIDES)
    GRL = refshim.import_reference_grl()
    torch.manual_seed(0)
    ref = GRL(**cfg).eval()
    sd = O.seeded_state_dict({k: tuple(v.shape) for k, v in ref.state_dict().items()}, seed=0)
    full = ref.state_dict()
    full.update(sd)
    ref.load_state_dict(full, strict=True)
    lq = _texture(np.random.RandomState(21), 48, 64).transpose(2, 0, 1)[None].copy()
    x = torch.from_numpy(lq).float() / 255
    with torch.no_grad():
        y32 = ref(x)
        y64 = ref.double()(x.double())
    scores = []
    for y in (y32, y64):
        p = torch.clamp(y.float(), 0, 1).mul(255).round().div(255)[0].numpy()
        scores.append(ref64(N, ref_plane(N, p), params)[0])
    # how far the reference's NIQE of its own output moves when every 8-bit level that an output within 1e-3 (the model bar of the
    # GPU tests) could round the other way does so: all such levels down, all up, and three random choices
    lv = y64[0].clamp(0, 1).numpy() * 255
    rs, spreads, nears = np.random.RandomState(4), {}, {}
    for tag, tol in (("auto", 1e-3), ("high", 1e-5)):             # the model bars of precision "auto" and "high"
        near = np.abs(lv - np.floor(lv) - 0.5) <= tol * 255
        spread = 0.0
        for pick in ("down", "up", 0, 1, 2):
            up = np.ones(lv.shape, bool) if pick == "up" else np.zeros(lv.shape, bool) if pick == "down" else rs.uniform(size=lv.shape) < 0.5
            q = np.where(near, np.where(up, np.ceil(lv), np.floor(lv)), np.round(lv)).astype(np.float32) / np.float32(255)
            spread = max(spread, abs(ref64(N, ref_plane(N, q), params)[0] - scores[1]))
        spreads[tag], nears[tag] = spread, int(near.sum())
        print(f"bsr_pipeline: {nears[tag]} of {near.size} levels within {tol:g} of a rounding boundary; NIQE moves by up to {spread:.4f}")
    levels_differ = int(((y32.clamp(0, 1) * 255).round() != (y64.float().clamp(0, 1) * 255).round()).sum())
    meta = dict(cfg=cfg, weight_seed=0, out32_vs_out64=float((y32.double() - y64).abs().max()), levels_differ=levels_differ,
                niqe_output=scores[0], niqe_output64=scores[1], near_boundary_levels=nears, niqe_level_flip_spread=spreads)
    print(f"bsr_pipeline: output {tuple(y32.shape)} max|fp32 - fp64| = {meta['out32_vs_out64']:.3e}, {levels_differ} levels differ, "
          f"NIQE {scores[0]:.6f} (fp32 output) / {scores[1]:.6f} (float64 output)")
    # the float64 run is kept at fp32 precision, as its distance from the fp32 run in units of the last place (the two arrays side by
    # side do not fit the size limit of a fixture): fp32(output64) = (output.view(int32) + output64_ulps).view(float32)
    ulps = y64.float().numpy().view(np.int32) - y32.numpy().view(np.int32)
    arrays = dict(lq=lq, output=y32.numpy(), output64_ulps=ulps, niqe_output=np.array(scores[0]), niqe_output64=np.array(scores[1]))
    return arrays, meta


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=refshim.REFERENCE_ROOT)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args(argv)
    src = os.path.join(a.reference, "utils", "metrics", "niqe_pris_params.npz")
    if not os.path.isfile(src):
        raise SystemExit(f"reference tree not found at {a.reference} (no utils/metrics/niqe_pris_params.npz): this recipe needs it")
    if a.reference != refshim.REFERENCE_ROOT:
        refshim.REFERENCE_ROOT = a.reference
    _install_stubs()
    refshim.install_shims()
    if a.reference not in sys.path:
        sys.path.insert(0, a.reference)
    from utils import utils_image as U
    from utils.metrics import niqe as N

    from grl_image_restoration_amd.metrics import niqe_window

    os.makedirs(a.out, exist_ok=True)
    shutil.copyfile(src, os.path.join(a.out, "niqe_pris_params.npz"))
    params = dict(np.load(src))
    win_err = float(np.abs(niqe_window().numpy() - params["gaussian_window"]).max())
    print(f"fspecial('gaussian', 7, 7/6) against the file's gaussian_window: max difference {win_err:.3e}")
    assert win_err < 1e-16, win_err

    arrays, cases = build_niqe(N, U, params)
    bad = y_mismatches(N)
    print(f"Y plane over all 2^24 colours: {bad} mismatches")
    assert bad == 0, bad
    meta = dict(cases=cases, y_mismatches=bad, window_max_diff=win_err,
                largest_ref32_vs_ref64=max(c["ref32_vs_ref64"] for c in cases.values()),
                source="utils/metrics/niqe.py: NaturalImageQualityEvaluator.update (ref32), niqe() on the float64 plane (ref64)")
    for name, (arr, m) in (("niqe", (arrays, meta)), ("bsr_pipeline", build_bsr_pipeline(N, params))):
        path = os.path.join(a.out, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(m), **arr)
        print(f"wrote {path}: {len(arr)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
