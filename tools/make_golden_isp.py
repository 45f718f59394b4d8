"""Writes tests/golden/tasks/isp.npz, the yardstick of the camera-noise stage (grl_image_restoration_amd/isp.py, csrc/isp.hip), from
the reference's own modules: ``utils/utils_bsr/utils_isp.py`` is imported from the reference checkout given as argument (``cv2``,
``pandas`` and ``torchvision``, which its imports pull in and the ISP does not use, are stubbed in ``sys.modules`` when missing).
Nothing of the package under test is imported, and nothing of the reference is copied: the file holds data its programs read
(camera profiles) and results they computed.

  curve_x, curve_y    (11, K) the knots of the tone curves the reference draws from, rows 0, 1, 2, 66, 126, 115, 127, 128, 132, 133, 74
                      of ``tonecurves.mat``, each reshaped (2, -1) in Fortran order
  forward1, forward2  (11, 3, 3) ``ForwardMatrix1 / 2`` of the 11 cameras of ``ISPModel.CameraType``
  table_idx, table_yi, table_yi_inv
                      per curve a sample of ``ToneMapping.yi`` / ``yi_inv``: every 4999th entry and the 64 entries around the
                      largest step of ``yi_inv`` (idx (11, n); the values fp32)
  case<i>__*          three cases on curves 2, 74 and 127 (positions 2, 10, 6 of the bank), batch of one: ``x`` uint8 (h, w, 3) the LQ,
                      ``hr`` uint8 the HR, ``camera`` / ``curve`` (bank positions), ``fw``, ``d_r``, ``d_b``, ``e``, ``shot``, ``read``,
                      ``z`` (h, w) unit normals, and from the reference's modules ``raw`` (h, w): the RGGB plane before the noise
                      (``ISPNet.reverse`` without ``AddNoise``), ``out`` (3, h, w): ``ISPNet.forward(noisy, True)`` of
                      ``noisy = clamp(raw + sqrt(raw * shot + read) * z)``, and ``hr_out`` (3, H, W): ``forward(reverse(hr, False), False)``.
                      That noise line is asserted once, under ``torch.manual_seed``, to equal the reference's
                      ``utils_noise.add_noise`` on the same stream to fp32 rounding.

    python tools/make_golden_isp.py /path/to/reference
"""
import importlib
import os
import sys
import types

import numpy as np
import scipy.io
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "tasks", "isp.npz")

CAMERAS = ("canon_eos_1d_mark_ii", "canon_eos_5d_mark_iii", "canon", "canon_eos_6d_v1", "huawei_p20", "huawei_p30", "huawei_v8",
           "nikon_d500", "nikon_d810", "nikon_d5600", "olympus_em1")
CURVES = (0, 1, 2, 66, 126, 115, 127, 128, 132, 133, 74)
# (h, w), (H, W), camera position, curve position, fw, d_r, d_b, e, shot, read
CASES = [
    ((7, 9), (12, 10), 7, 2, 0.3, 1.9, 1.5, 0.06, 0.004, 0.0004),
    ((33, 20), (40, 28), 8, 10, 0.8, 1.3, 2.3, -0.08, 0.0006, 2e-5),
    ((64, 64), (64, 64), 4, 6, 0.55, 2.1, 1.25, 0.02, 0.0015, 1e-4),
]


def reference_isp(ref: str):
    for name in ("cv2", "pandas", "torchvision", "torchvision.utils"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["torchvision.utils"], "make_grid"):
        sys.modules["torchvision.utils"].make_grid = None
        sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
    sys.path.insert(0, ref)
    from utils.utils_bsr import utils_isp, utils_noise

    return utils_isp, utils_noise


def image(g, h, w):
    """An 8-bit test image: a smooth colour ramp plus texture, with a dark and a saturated corner."""
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 255.0 * (x + y) / max(h + w - 2, 1)], -1)
    im = np.clip(0.7 * base + 0.3 * g.randint(0, 256, (h, w, 3)), 0, 255)
    im[:2, :2], im[-2:, -2:] = 0, 255
    return im.astype(np.uint8)


def main():
    ref = sys.argv[1]
    utils_isp, utils_noise = reference_isp(ref)
    prof = os.path.join(ref, "utils", "cameraprofile")
    curves = scipy.io.loadmat(os.path.join(prof, "tonecurves.mat"))["ToneCurves"]
    xy = [np.reshape(curves[i, :], (2, -1), "F") for i in CURVES]
    mats = [scipy.io.loadmat(os.path.join(prof, name + ".mat")) for name in CAMERAS]
    arrays = {
        "curve_x": np.stack([c[0] for c in xy]).astype(np.float64), "curve_y": np.stack([c[1] for c in xy]).astype(np.float64),
        "forward1": np.stack([np.asarray(m["ForwardMatrix1"], dtype=np.float64).reshape(3, 3) for m in mats]),
        "forward2": np.stack([np.asarray(m["ForwardMatrix2"], dtype=np.float64).reshape(3, 3) for m in mats]),
    }

    idx, yi, yi_inv, tone = [], [], [], {}
    for k, c in enumerate(xy):
        tm = utils_isp.ToneMapping(ToneCurveX=c[0], ToneCurveY=c[1])
        assert not bool(torch.isnan(tm.yi).any() | torch.isnan(tm.yi_inv).any()), k
        at = int((tm.yi_inv[1:] - tm.yi_inv[:-1]).abs().argmax())
        lo = min(max(at - 31, 0), tm.yi.numel() - 64)
        i = np.unique(np.concatenate([np.arange(0, tm.yi.numel(), 4999), np.arange(lo, lo + 64)]))
        idx.append(i), yi.append(tm.yi.numpy()[i]), yi_inv.append(tm.yi_inv.numpy()[i])
        print(f"curve {CURVES[k]}: largest step of yi_inv {float((tm.yi_inv[1:] - tm.yi_inv[:-1]).abs().max()):.3e} at {at}")
    n = min(len(i) for i in idx)               # the 64 may overlap the grid: keep a common length
    arrays["table_idx"] = np.stack([i[:n] for i in idx]).astype(np.int32)
    arrays["table_yi"], arrays["table_yi_inv"] = np.stack([v[:n] for v in yi]), np.stack([v[:n] for v in yi_inv])

    # the noise line of the cases against the reference's add_noise on the same stream
    torch.manual_seed(11)
    plane = torch.rand(1, 1, 16, 16)
    torch.manual_seed(12)
    theirs = utils_noise.add_noise(plane.clone(), 0.004, 0.0004)
    torch.manual_seed(12)
    z = torch.distributions.normal.Normal(torch.Tensor([0.0]), torch.ones(1, 1, 16, 16)).sample()
    ours = plane + torch.sqrt(plane * 0.004 + 0.0004) * z
    assert float((ours - theirs).abs().max()) <= 2 ** -22, float((ours - theirs).abs().max())

    g = np.random.RandomState(2025)
    for n, ((h, w), (H, W), cam, cur, fw, d_r, d_b, e, shot, read) in enumerate(CASES):
        x8, hr8 = image(g, h, w), image(g, H, W)
        zn = g.standard_normal((h, w)).astype(np.float32)
        f1 = torch.from_numpy(arrays["forward1"][cam]).float().reshape(3, 3)
        f2 = torch.from_numpy(arrays["forward2"][cam]).float().reshape(3, 3)
        FW = torch.tensor([fw], dtype=torch.float32)
        D = torch.tensor([d_r, 1.0, d_b]).diag().float()
        net = utils_isp.ISPNet(weight_raw2xyz=torch.matmul(FW * f1 + (1 - FW) * f2, D), ToneCurveX=xy[cur][0], ToneCurveY=xy[cur][1],
                               BaselineExposure=0, BaselineExposureOffset=torch.tensor([e], dtype=torch.float32))
        t4 = lambda a: torch.from_numpy(a.astype(np.float32) / 255.0).permute(2, 0, 1)[None].contiguous()
        with torch.no_grad():
            v = t4(x8)
            for m in (net.gammacorrect, net.tonemapping, net.xyz2linearrgb, net.raw2xyz, net.exposurecompensation, net.demosaic):
                v = m.reverse(v)
            raw = v.clone()
            noisy = (raw + torch.sqrt(raw * np.float32(shot) + np.float32(read)) * torch.from_numpy(zn)[None, None]).clamp(0, 1)
            out = net.forward(noisy.clone(), True)
            hr_out = net.forward(net.reverse(t4(hr8), False), False)
        for key, val in dict(x=x8, hr=hr8, z=zn, raw=raw[0, 0].numpy(), out=out[0].numpy(), hr_out=hr_out[0].numpy(),
                             camera=np.int64(cam), curve=np.int64(cur), fw=np.float64(fw), d_r=np.float64(d_r), d_b=np.float64(d_b),
                             e=np.float64(e), shot=np.float64(shot), read=np.float64(read)).items():
            arrays[f"case{n}__{key}"] = val
        assert raw.dtype == out.dtype == hr_out.dtype == torch.float32 and raw.shape == (1, 1, h, w)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
