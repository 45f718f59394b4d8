"""The camera-noise stage of the blind-SR degradation: stage 2 of the reference's ``degradation_sr2`` (utils/utils_bsr/utils_sisr.py:
365-370), ``ISPModel.forward`` (utils/utils_bsr/utils_isp.py:480-547).  The LQ goes sRGB -> camera raw (inverse gamma, inverse tone
curve, sRGB -> XYZ(D50) -> camera, exposure), RGGB mosaic, signal-dependent shot and read noise, Malvar demosaic, and back (exposure,
camera -> XYZ -> sRGB, tone curve, gamma); the HR goes through the same colour round trip without mosaic and noise.  The arithmetic
of every step is stated in include/grl_hip.h (grl_isp_unprocess / grl_isp_process / grl_isp_roundtrip).

  CameraBank      the data of the reference's ``utils/cameraprofile`` folder: ``ForwardMatrix1 / 2`` of the 11 cameras and the 11 tone
                  curves of ``tonecurves.mat`` the reference draws from, and the 22 tables of 1,000,001 fp32 entries built from the
                  curves as ``ToneMapping`` builds them (scipy's cubic ``interp1d``; scipy is imported when a table is built).
                  The profiles are the user's: ``CameraBank.load(dir)`` reads their copy of the folder, nothing is downloaded.
  camera_noise    lists of LQ and HR images through the stage.  CUDA tensors (fp32): one launch of each entry per call
                  (csrc/isp.hip; there is no fallback).  CPU tensors: the torch restatement below in the tensors' dtype, every
                  operation rounded to it -- in float64 the yardstick of the kernels, in fp32 the reference's own arithmetic.
"""
import os
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from . import item_lists, ops

CAMERAS = ("canon_eos_1d_mark_ii", "canon_eos_5d_mark_iii", "canon", "canon_eos_6d_v1", "huawei_p20", "huawei_p30", "huawei_v8",
           "nikon_d500", "nikon_d810", "nikon_d5600", "olympus_em1")                      # ISPModel.CameraType, utils_isp.py:465-477
CURVES = (0, 1, 2, 66, 126, 115, 127, 128, 132, 133, 74)                                  # rows of tonecurves.mat, utils_isp.py:502-504
TABLE_N, DELTA, REC = 1000001, 1e-6, 40
MIN_SIDE = 3                                                                              # the demosaic reflects by 2


def _srgb_from_xyz_d50() -> torch.Tensor:
    """W1 of the header: XYZ(D50) -> linear sRGB(D65), the sRGB matrix times the Bradford adaptation D50 -> D65, in fp32 as
    ``utils_color.xyz2linearrgb_weight(0)`` computes it (utils_color.py:25-40, 77-118)."""
    d50 = torch.tensor([0.96422, 1, 0.82521], dtype=torch.float32).reshape(3, 1)
    d65 = torch.tensor([0.95047, 1, 1.08883], dtype=torch.float32).reshape(3, 1)
    bfd = torch.tensor([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]], dtype=torch.float32)
    adapt = torch.matmul(torch.matmul(torch.inverse(bfd), (torch.matmul(bfd, d65) / torch.matmul(bfd, d50)).diagflat()), bfd)
    srgb = torch.tensor([[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]],
                        dtype=torch.float32)
    return torch.matmul(srgb, adapt)


class CameraParams(NamedTuple):
    """One acting sample: ``rec`` the fp32 record of the header (W1i, W2i, W2, W1, 2^e, 2^-e, shot, read), ``curve`` the position of
    its tone curve in the bank, ``bank`` the bank that holds the tables."""
    rec: torch.Tensor
    curve: int
    bank: "CameraBank"


class CameraBank:
    """``forward1`` / ``forward2``: (11, 3, 3) the cameras' ``ForwardMatrix1 / 2`` in the order of ``CAMERAS``; ``curve_x`` /
    ``curve_y``: (11, K) the knots of the tone curves in the order of ``CURVES``.  ``tables``: {curve: (2, 1000001) fp32 ``yi``,
    ``yi_inv``} for curves whose tables the caller has (an analytic curve); the others are built from the knots."""

    def __init__(self, forward1, forward2, curve_x, curve_y, tables: Optional[dict] = None):
        self.forward1 = torch.as_tensor(np.asarray(forward1)).float().reshape(-1, 3, 3)
        self.forward2 = torch.as_tensor(np.asarray(forward2)).float().reshape(-1, 3, 3)
        self.curve_x, self.curve_y = np.asarray(curve_x, dtype=np.float64), np.asarray(curve_y, dtype=np.float64)
        n, k = len(CAMERAS), len(CURVES)
        if self.forward1.shape != (n, 3, 3) or self.forward2.shape != (n, 3, 3):
            raise ValueError(f"CameraBank: {n} ForwardMatrix1 and {n} ForwardMatrix2 of 3 x 3")
        if self.curve_x.ndim != 2 or self.curve_x.shape != self.curve_y.shape or self.curve_x.shape[0] != k or self.curve_x.shape[1] < 4:
            raise ValueError(f"CameraBank: the knots are two ({k}, K) arrays, K at least 4")
        self.w1 = _srgb_from_xyz_d50()
        self.w1i = torch.inverse(self.w1)
        self._tables = {}
        for c, t in (tables or {}).items():
            t = torch.as_tensor(t)
            if not 0 <= int(c) < k or t.shape != (2, TABLE_N) or t.dtype != torch.float32:
                raise ValueError(f"CameraBank: a table is (2, {TABLE_N}) fp32 for a curve of 0 .. {k - 1}")
            self._tables[int(c)] = t
        self._all = {}

    @classmethod
    def from_arrays(cls, forward1, forward2, curve_x, curve_y, tables: Optional[dict] = None) -> "CameraBank":
        return cls(forward1, forward2, curve_x, curve_y, tables)

    @classmethod
    def load(cls, folder: str) -> "CameraBank":
        """Reads ``tonecurves.mat`` (key ``ToneCurves``: a row per curve, reshaped (2, -1) in Fortran order into X and Y,
        utils_isp.py:505-507) and ``<camera>.mat`` (keys ``ForwardMatrix1``, ``ForwardMatrix2``) of every camera of ``CAMERAS``."""
        from scipy.io import loadmat

        def read(name, keys):
            path = os.path.join(folder, name)
            if not os.path.isfile(path):
                raise FileNotFoundError(f"camera profiles: {path} is missing (the folder is the reference's utils/cameraprofile)")
            m = loadmat(path)
            for key in keys:
                if key not in m:
                    raise KeyError(f"camera profiles: {path} has no key {key!r}")
            return [np.asarray(m[key], dtype=np.float64) for key in keys]

        (curves,) = read("tonecurves.mat", ["ToneCurves"])
        if curves.ndim != 2 or curves.shape[0] <= max(CURVES) or curves.shape[1] % 2:
            raise ValueError(f"camera profiles: ToneCurves of tonecurves.mat is {curves.shape}, not (more than {max(CURVES)} curves, 2 K)")
        xy = [np.reshape(curves[i], (2, -1), "F") for i in CURVES]
        mats = [read(name + ".mat", ["ForwardMatrix1", "ForwardMatrix2"]) for name in CAMERAS]
        return cls([m[0].reshape(3, 3) for m in mats], [m[1].reshape(3, 3) for m in mats], [c[0] for c in xy], [c[1] for c in xy])

    def table(self, curve: int) -> torch.Tensor:
        """(2, 1000001) fp32: ``ToneMapping.yi`` and ``yi_inv`` of curve ``curve`` (utils_isp.py:345-352), built once."""
        if curve not in self._tables:
            from scipy.interpolate import interp1d

            xi = np.linspace(0, 1, num=int(1 / DELTA + 1), endpoint=True)
            yi = interp1d(self.curve_x[curve], self.curve_y[curve], kind="cubic")(xi)
            yi_inv = interp1d(yi, xi, kind="cubic")(xi)
            self._tables[curve] = torch.stack([torch.from_numpy(yi).float(), torch.from_numpy(yi_inv).float()])
        return self._tables[curve]

    def tables(self, device="cpu") -> torch.Tensor:
        """All 22 tables as one flat fp32 tensor (88 MB), curve c's ``yi`` at element ``2 c * 1000001`` and its ``yi_inv`` after it;
        built, and moved to ``device``, on first use."""
        device = torch.device(device)
        if device not in self._all:
            self._all[device] = torch.cat([self.table(c).reshape(-1) for c in range(len(CURVES))]).to(device)
        return self._all[device]

    def params(self, draw: dict) -> CameraParams:
        """One sample's draws (the ``camera`` op of ``bsr_degrade.draw_plan``: ``camera``, ``curve``, ``fw``, ``d_r``, ``d_b``, ``e``,
        ``shot``, ``read``) as the parameter record, with the fp32 products and ``torch.inverse`` of utils_isp.py:508-536, 54."""
        f32 = lambda v: torch.tensor(float(v), dtype=torch.float32)
        fw = f32(draw["fw"])
        d = torch.stack([f32(draw["d_r"]), f32(1.0), f32(draw["d_b"])]).diag()
        w2 = torch.matmul(fw * self.forward1[draw["camera"]] + (1 - fw) * self.forward2[draw["camera"]], d)
        p2e = torch.pow(2, f32(draw["e"]))
        rec = torch.cat([self.w1i.reshape(-1), torch.inverse(w2).reshape(-1), w2.reshape(-1), self.w1.reshape(-1),
                         torch.stack([p2e, 1 / p2e, f32(draw["shot"]), f32(draw["read"])])])
        return CameraParams(rec, int(draw["curve"]), self)


# ---- the torch restatement --------------------------------------------------------------------------------------------------------
_DEMOSAIC = torch.tensor([
    [[0, 0, -1, 0, 0], [0, 0, 2, 0, 0], [-1, 2, 4, 2, -1], [0, 0, 2, 0, 0], [0, 0, -1, 0, 0]],                       # kgrb
    [[0, 0, 0.5, 0, 0], [0, -1, 0, -1, 0], [-1, 4, 5, 4, -1], [0, -1, 0, -1, 0], [0, 0, 0.5, 0, 0]],                 # krbg0
    [[0, 0, -1, 0, 0], [0, -1, 4, -1, 0], [0.5, 0, 5, 0, 0.5], [0, -1, 4, -1, 0], [0, 0, -1, 0, 0]],                 # krbg1 = krbg0^T
    [[0, 0, -1.5, 0, 0], [0, 2, 0, 2, 0], [-1.5, 0, 6, 0, -1.5], [0, 2, 0, 2, 0], [0, 0, -1.5, 0, 0]],               # krbbr
], dtype=torch.float64) / 8


def _mat(m: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    return torch.einsum("ij,jhw->ihw", m.to(x.dtype), x)


def _lut(table: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    return table[torch.round(x.clamp(0, 1) / DELTA).long().clamp(max=TABLE_N - 1)].to(x.dtype).clamp(0, 1)


def unprocess(x: torch.Tensor, p: CameraParams) -> torch.Tensor:
    """The unprocess chain of the header on a (3, h, w) image, all three channels (``ISPNet.reverse(x, False)``)."""
    r = p.rec.to(x.dtype)
    x = x.clamp(0, 1)
    x = torch.where(x > 0.04045, ((200.0 * x + 11.0) / 211.0) ** 2.4, x.clamp(min=1e-8) / 12.92).clamp(0, 1)
    x = _lut(p.bank.table(p.curve)[1], x)
    x = _mat(r[9:18].view(3, 3), _mat(r[0:9].view(3, 3), x))
    return (x / r[36]).clamp(0, 1)


def process(x: torch.Tensor, p: CameraParams) -> torch.Tensor:
    """The process chain of the header on a (3, h, w) camera image (``ISPNet.forward(x, False)``)."""
    r = p.rec.to(x.dtype)
    x = (x * r[36]).clamp(0, 1)
    x = _mat(r[27:36].view(3, 3), _mat(r[18:27].view(3, 3), x))
    x = _lut(p.bank.table(p.curve)[0], x)
    x = torch.where(x > 0.0031308, 1.055 * x ** (1.0 / 2.4) - 0.055, 12.92 * x)
    return x.clamp(0, 1)


def mosaic(x: torch.Tensor) -> torch.Tensor:
    """(3, h, w) -> the RGGB plane (h, w) (``Demosaic.reverse``)."""
    raw = ops.empty_like(x[0])
    raw[0::2, 0::2], raw[0::2, 1::2], raw[1::2, 0::2], raw[1::2, 1::2] = x[0, 0::2, 0::2], x[1, 0::2, 1::2], x[1, 1::2, 0::2], x[2, 1::2, 1::2]
    return raw.clamp(0, 1)


def add_raw_noise(raw: torch.Tensor, p: CameraParams, z: torch.Tensor) -> torch.Tensor:
    r = p.rec.to(raw.dtype)
    return (raw + torch.sqrt(raw * r[38] + r[39]) * z.to(raw.dtype)).clamp(0, 1)


def demosaic(raw: torch.Tensor) -> torch.Tensor:
    """The RGGB plane (h, w) -> (3, h, w) (``Demosaic.forward``)."""
    out = raw[None].repeat(3, 1, 1)
    conv = F.conv2d(F.pad(raw[None, None], (2, 2, 2, 2), mode="reflect"), _DEMOSAIC.to(raw.dtype)[:, None])[0]
    out[1, 0::2, 0::2], out[1, 1::2, 1::2] = conv[0, 0::2, 0::2], conv[0, 1::2, 1::2]
    out[0, 0::2, 1::2], out[0, 1::2, 0::2], out[0, 1::2, 1::2] = conv[1, 0::2, 1::2], conv[2, 1::2, 0::2], conv[3, 1::2, 1::2]
    out[2, 0::2, 1::2], out[2, 1::2, 0::2], out[2, 0::2, 0::2] = conv[2, 0::2, 1::2], conv[1, 1::2, 0::2], conv[3, 0::2, 0::2]
    return out.clamp(0, 1)


# ---- the stage on lists of images -------------------------------------------------------------------------------------------------
def hip_isp(entry: str, src: torch.Tensor, dst: torch.Tensor, items, params: Sequence[CameraParams],
            normals: Optional[torch.Tensor] = None) -> None:
    """One launch of ``grl_isp_unprocess`` / ``grl_isp_process`` / ``grl_isp_roundtrip``.  ``src`` / ``dst``: flat fp32 CUDA arenas
    (they may be one tensor); ``items``: host tuples (src_off, dst_off, h, w, z_off) -- the table offsets come from the params;
    ``normals``: the flat fp32 normals on that device (unprocess).  As ``bsr_degrade.hip_cv_resize``, this wrapper vouches for the
    list: the maxima come from the items, the callers hand out disjoint destinations."""
    tables = params[0].bank.tables(src.device)
    if any(p.bank is not params[0].bank for p in params):
        raise ValueError("hip_isp: the params of one call come from one bank")
    rows = [(so, do, h, w, 2 * p.curve * TABLE_N, (2 * p.curve + 1) * TABLE_N, zo, 0) for (so, do, h, w, zo), p in zip(items, params)]
    recs = torch.stack([p.rec for p in params]).to(src.device)
    item_lists.launch(entry, src, dst, item_lists.table(rows, src.device), params=recs.data_ptr(), tables=tables.data_ptr(),
                      tables_elems=tables.numel(), normals=normals.data_ptr() if normals is not None else None,
                      normals_elems=normals.numel() if normals is not None else 0, C=3,
                      max_h=max(r[2] for r in rows), max_w=max(r[3] for r in rows))


def camera_noise(imgs: Sequence[torch.Tensor], hr: Optional[Sequence[torch.Tensor]], params: Sequence[CameraParams],
                 z: Sequence[torch.Tensor]):
    """``ISPModel.forward`` for every sample of a list: ``imgs[i]`` (3, h, w) the LQ, ``hr[i]`` (3, H, W) its HR (``hr=None``: the HR
    pass is not run), ``params[i]`` of ``CameraBank.params``, ``z[i]`` (h, w) unit normals.  Returns ``(lq, hr)``: new tensors of
    the inputs' shapes (``hr`` None without one).  CUDA: ``grl_isp_unprocess``, ``grl_isp_process`` and (with ``hr``)
    ``grl_isp_roundtrip``, one launch each.  CPU: the restatement in the tensors' dtype.  A side below 3 raises ValueError."""
    imgs, params, z = list(imgs), list(params), list(z)
    hr = None if hr is None else list(hr)
    if not imgs or len(params) != len(imgs) or len(z) != len(imgs) or (hr is not None and len(hr) != len(imgs)):
        raise ValueError("camera_noise: one params record, one normals plane (and one HR image) per image, at least one image")
    item_lists.check_images(imgs, "camera_noise (the demosaic reflects by 2)", (3,), MIN_SIDE)
    if hr is not None:
        item_lists.check_images(hr, "camera_noise, the HR images (the demosaic reflects by 2)", (3,), MIN_SIDE)
    if any(n.shape != im.shape[1:] for n, im in zip(z, imgs)):
        raise ValueError("camera_noise: the normals of an image are (h, w)")
    if not imgs[0].is_cuda:
        lq = [process(demosaic(add_raw_noise(mosaic(unprocess(im, p)), p, n)), p) for im, p, n in zip(imgs, params, z)]
        return lq, (None if hr is None else [process(unprocess(im, p), p) for im, p in zip(hr, params)])

    def run(entry, tensors, planes_out, normals=None):
        shapes = [((planes_out,) if planes_out > 1 else ()) + tuple(t.shape[-2:]) for t in tensors]
        (src, so), (dst, do) = item_lists.pack(tensors), item_lists.empty(shapes, tensors[0].device)
        hip_isp(entry, src, dst, [(a, d, *t.shape[-2:], d if normals is not None else 0) for a, d, t in zip(so, do, tensors)], params, normals)
        return item_lists.views(dst, do, shapes)

    raw = run("grl_isp_unprocess", imgs, 1, item_lists.pack(z)[0].float())
    return run("grl_isp_process", raw, 3), (None if hr is None else run("grl_isp_roundtrip", hr, 3))
