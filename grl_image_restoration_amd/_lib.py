"""ctypes binding of libgrl_hip.so (the C ABI declared in include/grl_hip.h).

There is deliberately NO fallback: if the shared library is missing or stale, or a kernel
returns an error, a RuntimeError is raised.  Build it with ``python __graft_entry__.py`` (or
``make -C grl_image_restoration_amd/csrc``).
"""
import ctypes as C
import os

from . import switches as SW

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgrl_hip.so")
ABI_VERSION = 46
DT_F32, DT_BF16, DT_F16 = 0, 1, 2

EPI_PLAIN, EPI_GELU, EPI_GROUPNORM, EPI_LN_RES, EPI_GELU_GRAD = 0, 1, 2, 3, 4

class _Strict(C.Structure):
    """ctypes silently turns unknown keyword arguments into plain attributes (leaving the C field
    zero); refuse them instead."""

    def __init__(self, **kw):
        bad = set(kw) - {f[0] for f in self._fields_}
        if bad:
            raise TypeError(f"{type(self).__name__}: unknown field(s) {sorted(bad)}")
        super().__init__(**kw)


class GrlLinearArgs(_Strict):
    _fields_ = [
        ("a", C.c_void_p),
        ("a_dtype", C.c_int32),
        ("lda", C.c_int64),
        ("pool_df", C.c_int32),
        ("pool_H", C.c_int32),
        ("pool_W", C.c_int32),
        ("w", C.c_void_p),
        ("bias", C.c_void_p),
        ("M", C.c_int32),
        ("Npad", C.c_int32),
        ("Kpad", C.c_int32),
        ("epi", C.c_int32),
        ("gscale", C.c_void_p),
        ("ln_g", C.c_void_p),
        ("ln_b", C.c_void_p),
        ("n_real", C.c_int32),
        ("ln_eps", C.c_float),
        ("res_scale", C.c_float),
        ("resid", C.c_void_p),
        ("ldr", C.c_int64),
        ("add2", C.c_void_p),
        ("add2_dtype", C.c_int32),
        ("ldadd2", C.c_int64),
        ("add2_scale", C.c_void_p),
        ("rows_per_image", C.c_int32),
        ("a_split", C.c_int32),
        ("a_scale", C.c_float),
        ("out_scale", C.c_float),
        ("out", C.c_void_p),
        ("out_dtype", C.c_int32),
        ("ldo", C.c_int64),
        ("out_plane_stride", C.c_int64),
        ("out_lo", C.c_void_p),
        ("w_regs", C.c_void_p),
        ("a_cols", C.c_int32),
        ("a_one", C.c_int32),
        ("n_store", C.c_int32),
        ("a_gelu", C.c_int32),
        ("a16_out", C.c_void_p),
        ("lda16", C.c_int64),
    ]


class GrlMlpArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("ldx", C.c_int64),
        ("blob", C.c_void_p),
        ("M", C.c_int32),
        ("Cpad", C.c_int32),
        ("Hpad", C.c_int32),
        ("b2", C.c_void_p),
        ("ln_g", C.c_void_p),
        ("ln_b", C.c_void_p),
        ("n_real", C.c_int32),
        ("ln_eps", C.c_float),
        ("res_scale", C.c_float),
        ("out", C.c_void_p),
        ("ldo", C.c_int64),
    ]


class GrlTailArgs(_Strict):
    _fields_ = [
        ("att", C.c_void_p),
        ("ldatt", C.c_int64),
        ("x", C.c_void_p),
        ("ldx", C.c_int64),
        ("cab", C.c_void_p),
        ("ldcab", C.c_int64),
        ("gate", C.c_void_p),
        ("rows_per_image", C.c_int32),
        ("pblob", C.c_void_p),
        ("pb", C.c_void_p),
        ("n1_g", C.c_void_p),
        ("n1_b", C.c_void_p),
        ("blob", C.c_void_p),
        ("M", C.c_int32),
        ("Cpad", C.c_int32),
        ("Hpad", C.c_int32),
        ("b2", C.c_void_p),
        ("n2_g", C.c_void_p),
        ("n2_b", C.c_void_p),
        ("n_real", C.c_int32),
        ("ln_eps", C.c_float),
        ("res_scale", C.c_float),
        ("out", C.c_void_p),
        ("ldo", C.c_int64),
        ("rblob", C.c_void_p),
    ]


class GrlQkvAnchorArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("ldx", C.c_int64),
        ("B", C.c_int32),
        ("H", C.c_int32),
        ("W", C.c_int32),
        ("Cpad", C.c_int32),
        ("blob", C.c_void_p),
        ("nslots", C.c_int32),
        ("nanc", C.c_int32),
        ("out", C.c_void_p),
        ("out_plane_stride", C.c_int64),
        ("anc", C.c_void_p),
        ("anc_plane_stride", C.c_int64),
        ("lo_blob", C.c_void_p),
    ]


class GrlCabConv2Args(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("ldx", C.c_int64),
        ("blob", C.c_void_p),
        ("bias", C.c_void_p),
        ("B", C.c_int32),
        ("H", C.c_int32),
        ("W", C.c_int32),
        ("wgs_per_image", C.c_int32),
        ("out", C.c_void_p),
        ("ldo", C.c_int64),
        ("pool_partial", C.c_void_p),
        ("pool_stride", C.c_int64),
    ]


class GrlQkvArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("ldx", C.c_int64),
        ("blob", C.c_void_p),
        ("M", C.c_int32),
        ("Cpad", C.c_int32),
        ("nslots", C.c_int32),
        ("out", C.c_void_p),
        ("out_plane_stride", C.c_int64),
    ]


class GrlTokenGrid(_Strict):
    _fields_ = [
        ("ptr", C.c_void_p),
        ("ld", C.c_int64),
        ("hstride", C.c_int64),
        ("col0", C.c_int32),
        ("Himg", C.c_int32),
        ("Wimg", C.c_int32),
        ("wh", C.c_int32),
        ("ww", C.c_int32),
        ("shy", C.c_int32),
        ("shx", C.c_int32),
        ("transposed", C.c_int32),
    ]


class GrlAttnArgs(_Strict):
    _fields_ = [
        ("q", GrlTokenGrid),
        ("k", GrlTokenGrid),
        ("v", GrlTokenGrid),
        ("o", GrlTokenGrid),
        ("B", C.c_int32),
        ("nh", C.c_int32),
        ("nwy", C.c_int32),
        ("nwx", C.c_int32),
        ("table", C.c_void_p),
        ("trows", C.c_int32),
        ("tstride", C.c_int32),
        ("masked", C.c_int32),
        ("ones_col", C.c_int32),
        ("head_dim", C.c_int32),
        ("out_dtype", C.c_int32),
        ("k_one31", C.c_int32),
        ("lazy_floor", C.c_void_p),
        ("lse", C.c_void_p),
        ("lse_stride", C.c_int64),
        ("q_lo", C.c_void_p),
        ("k_lo", C.c_void_p),
        ("v_lo", C.c_void_p),
        ("o_lo", C.c_void_p),
        ("lazy_ceil", C.c_void_p),
    ]


class GrlConvArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("x_dtype", C.c_int32),
        ("ldx", C.c_int64),
        ("w", C.c_void_p),
        ("w_tap_stride", C.c_int64),
        ("bias", C.c_void_p),
        ("B", C.c_int32),
        ("H", C.c_int32),
        ("W", C.c_int32),
        ("CinP", C.c_int32),
        ("CoutP", C.c_int32),
        ("x_split", C.c_int32),
        ("x_scale", C.c_float),
        ("out_scale", C.c_float),
        ("act", C.c_int32),
        ("slope", C.c_float),
        ("resid", C.c_void_p),
        ("ldr", C.c_int64),
        ("pool_partial", C.c_void_p),
        ("pool_stride", C.c_int64),
        ("out", C.c_void_p),
        ("out_dtype", C.c_int32),
        ("ldo", C.c_int64),
        ("shuffle_r", C.c_int32),
        ("shuffle_cg", C.c_int32),
        ("shuffle_ij0", C.c_int32),
        ("x_cols", C.c_int32),
        ("n_store", C.c_int32),
    ]


class GrlLnResArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("ldx", C.c_int64),
        ("resid", C.c_void_p),
        ("ldr", C.c_int64),
        ("gamma", C.c_void_p),
        ("beta", C.c_void_p),
        ("add2", C.c_void_p),
        ("add2_dtype", C.c_int32),
        ("ldadd2", C.c_int64),
        ("add2_scale", C.c_void_p),
        ("rows_per_image", C.c_int32),
        ("M", C.c_int32),
        ("n_real", C.c_int32),
        ("n_pad", C.c_int32),
        ("eps", C.c_float),
        ("res_scale", C.c_float),
        ("y", C.c_void_p),
        ("ldy", C.c_int64),
    ]


class GrlGemmTnArgs(_Strict):
    _fields_ = [
        ("a", C.c_void_p),
        ("lda", C.c_int64),
        ("b", C.c_void_p),
        ("b_dtype", C.c_int32),
        ("ldb", C.c_int64),
        ("M", C.c_int32),
        ("N", C.c_int32),
        ("K", C.c_int32),
        ("taps", C.c_int32),
        ("H", C.c_int32),
        ("W", C.c_int32),
        ("splits", C.c_int32),
        ("a_scale", C.c_float),
        ("out_scale", C.c_float),
        ("c", C.c_void_p),
        ("ldc", C.c_int64),
        ("c_tap_stride", C.c_int64),
        ("c_fix", C.c_void_p),
        ("b_ones", C.c_int32),
        ("reserved0", C.c_int32),
        ("c_bias", C.c_void_p),
        ("c_bias_fix", C.c_void_p),
        ("a_dtype", C.c_int32),
        ("reserved1", C.c_int32),
    ]


class GrlAttnBwdArgs(_Strict):
    _fields_ = [
        ("fwd", GrlAttnArgs),
        ("d_o", C.c_void_p),
        ("d_q", C.c_void_p),
        ("d_k", C.c_void_p),
        ("d_v", C.c_void_p),
        ("d_table", C.c_void_p),
        ("g_scale", C.c_float),
        ("d_table_fix", C.c_void_p),
        ("d_o_ld", C.c_int64),
    ]


class GrlAdamWArgs(_Strict):
    _fields_ = [
        ("params", C.c_void_p),
        ("grads", C.c_void_p),
        ("exp_avg", C.c_void_p),
        ("exp_avg_sq", C.c_void_p),
        ("numel", C.c_void_p),
        ("weight_decay_flags", C.c_void_p),
        ("chunk_tensor", C.c_void_p),
        ("chunk_offset", C.c_void_p),
        ("num_chunks", C.c_int32),
        ("lr", C.c_float),
        ("beta1", C.c_float),
        ("beta2", C.c_float),
        ("eps", C.c_float),
        ("weight_decay", C.c_float),
        ("bias_correction1", C.c_float),
        ("bias_correction2_sqrt", C.c_float),
        ("grad_scale", C.c_float),
        ("bias_corrections_dev", C.c_void_p),
        ("hyper_dev", C.c_void_p),
        ("grad_clip_dev", C.c_void_p),
        ("ema", C.c_void_p),
        ("ema_decay", C.c_float),
    ]


class GrlGradNormArgs(_Strict):
    _fields_ = [
        ("grads", C.c_void_p),
        ("numel", C.c_void_p),
        ("chunk_tensor", C.c_void_p),
        ("chunk_offset", C.c_void_p),
        ("num_chunks", C.c_int32),
        ("partials", C.c_void_p),
        ("base", C.c_int64),
    ]


class GrlGradClipArgs(_Strict):
    _fields_ = [
        ("partials", C.c_void_p),
        ("n_partials", C.c_int64),
        ("grad_scale", C.c_float),
        ("max_norm", C.c_float),
        ("out", C.c_void_p),
    ]


class GrlLnTrainArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int64),
        ("gamma", C.c_void_p),
        ("beta", C.c_void_p),
        ("y", C.c_void_p), ("ldy", C.c_int64),
        ("mean", C.c_void_p),
        ("rstd", C.c_void_p),
        ("dy", C.c_void_p), ("lddy", C.c_int64),
        ("dx", C.c_void_p), ("lddx", C.c_int64),
        ("dgamma", C.c_void_p),
        ("dbeta", C.c_void_p),
        ("M", C.c_int32), ("n", C.c_int32),
        ("eps", C.c_float),
        ("resid", C.c_void_p), ("ldr", C.c_int64),
        ("row_scale", C.c_void_p),
        ("rows_per_image", C.c_int32),
        ("alpha", C.c_float),
        ("stat_replicas", C.c_int32),
        ("reserved0", C.c_int32),
    ]


class GrlPlanesArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("scale", C.c_void_p),
        ("out32", C.c_void_p),
        ("out16", C.c_void_p),
        ("dy", C.c_void_p * 8),
        ("dx", C.c_void_p),
        ("dscale", C.c_void_p),
        ("T", C.c_int32), ("S_in", C.c_int32), ("S_out", C.c_int32), ("nh", C.c_int32), ("d", C.c_int32),
        ("src", C.c_int32 * 8), ("raw", C.c_int32 * 8), ("one_col", C.c_int32 * 8), ("want_dscale", C.c_int32 * 8),
        ("dscale_replicas", C.c_int32),
        ("reserved0", C.c_int32),
    ]


class GrlSeMlpArgs(_Strict):
    _fields_ = [
        ("pool", C.c_void_p),
        ("w1", C.c_void_p),
        ("b1", C.c_void_p),
        ("w2", C.c_void_p),
        ("b2", C.c_void_p),
        ("gate", C.c_void_p),
        ("hidden", C.c_void_p),
        ("d_gate", C.c_void_p),
        ("d_pool", C.c_void_p),
        ("d_w1", C.c_void_p),
        ("d_b1", C.c_void_p),
        ("d_w2", C.c_void_p),
        ("d_b2", C.c_void_p),
        ("B", C.c_int32), ("C", C.c_int32), ("Cmid", C.c_int32),
        ("parallel", C.c_int32),
    ]


class GrlSeRowsArgs(_Strict):
    _fields_ = [
        ("a", C.c_void_p), ("lda", C.c_int64),
        ("f", C.c_void_p), ("ldf", C.c_int64),
        ("g", C.c_void_p),
        ("h", C.c_void_p),
        ("out", C.c_void_p), ("ldo", C.c_int64),
        ("k", C.c_float),
        ("M", C.c_int32), ("C", C.c_int32), ("rows_per_image", C.c_int32),
    ]


class GrlCpbArgs(_Strict):
    _fields_ = [
        ("coords", C.c_void_p),
        ("w1", C.c_void_p),
        ("b1", C.c_void_p),
        ("w2", C.c_void_p),
        ("out", C.c_void_p),
        ("d_out", C.c_void_p),
        ("d_w1", C.c_void_p),
        ("d_b1", C.c_void_p),
        ("d_w2", C.c_void_p),
        ("G", C.c_int32),
        ("rows", C.c_int32),
        ("rows4", C.c_int32),
        ("nh", C.c_int32),
        ("hidden", C.c_int32),
    ]


METRIC_PSNR, METRIC_PSNR_Y, METRIC_SSIM, METRIC_SSIM_Y, METRIC_PSNRB, METRIC_PSNRB_Y = 1, 2, 4, 8, 16, 32
METRIC_COUNT = 6


class GrlMetricArgs(_Strict):
    _fields_ = [
        ("restored", C.c_void_p),
        ("restored_stride", C.c_int64 * 4),
        ("shape", C.c_int32 * 4),
        ("target", C.c_void_p),
        ("target_stride", C.c_int64 * 4),
        ("target_shape", C.c_int32 * 4),
        ("border", C.c_int32),
        ("metrics", C.c_int32),
        ("taps", C.c_double * 11),
        ("y_coef", C.c_float * 3),
        ("reserved0", C.c_int32),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_int64),
        ("out", C.c_void_p),
    ]


class GrlDemosaicArgs(_Strict):
    _fields_ = [
        ("plane", C.c_void_p * 4),
        ("stride", C.c_int64 * 3),
        ("N", C.c_int32),
        ("h", C.c_int32),
        ("w", C.c_int32),
        ("reserved0", C.c_int32),
        ("out", C.c_void_p),
    ]


class GrlResizeArgs(_Strict):
    _fields_ = [
        ("src", C.c_void_p),
        ("stride", C.c_int64 * 4),
        ("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("out_h", C.c_int32), ("out_w", C.c_int32),
        ("taps_h", C.c_int32), ("taps_w", C.c_int32),
        ("wh", C.c_void_p),
        ("ih", C.c_void_p),
        ("ww", C.c_void_p),
        ("iw", C.c_void_p),
        ("out", C.c_void_p),
        ("quantize", C.c_int32),
        ("out_f64", C.c_int32),
    ]


class GrlNiqeArgs(_Strict):
    _fields_ = [
        ("img", C.c_void_p),
        ("stride", C.c_int64 * 4),
        ("shape", C.c_int32 * 4),
        ("window", C.c_double * 49),
        ("grid", C.c_void_p),
        ("ngrid", C.c_int32),
        ("taps_h", C.c_int32), ("taps_w", C.c_int32),
        ("reserved0", C.c_int32),
        ("wh", C.c_void_p),
        ("ih", C.c_void_p),
        ("ww", C.c_void_p),
        ("iw", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_int64),
        ("out", C.c_void_p),
    ]


class GrlPatchArgs(_Strict):
    _fields_ = [
        ("store", C.c_void_p),
        ("offsets", C.c_void_p),
        ("dims", C.c_void_p),
        ("N", C.c_int32), ("C", C.c_int32),
        ("work", C.c_void_p),
        ("B", C.c_int32), ("P", C.c_int32), ("scale", C.c_int32),
        ("reserved0", C.c_int32),
        ("out", C.c_void_p),
    ]


class GrlPatchView(_Strict):
    _fields_ = [
        ("store", C.c_void_p),
        ("offsets", C.c_void_p),
        ("dims", C.c_void_p),
        ("N", C.c_int32), ("C", C.c_int32),
        ("scale", C.c_int32),
        ("Ctot", C.c_int32), ("c0", C.c_int32),
        ("reserved0", C.c_int32),
        ("out", C.c_void_p),
    ]


class GrlPatchViewsArgs(_Strict):
    _fields_ = [
        ("view", GrlPatchView * 4),
        ("work", C.c_void_p),
        ("B", C.c_int32), ("P", C.c_int32), ("V", C.c_int32),
        ("reserved0", C.c_int32),
    ]


class GrlBlurArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("stride", C.c_int64 * 4),
        ("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("taps", C.c_void_p),
        ("K", C.c_int32), ("pad", C.c_int32),
        ("add", C.c_void_p),
        ("add_stride", C.c_int64 * 3),
        ("out", C.c_void_p),
        ("center", C.c_void_p),
    ]


class GrlJpegArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("quality", C.c_void_p),
        ("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("workspace", C.c_void_p),
        ("out", C.c_void_p),
    ]


class GrlPack8Args(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("stride", C.c_int64 * 4),
        ("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("rep", C.c_int32),
        ("out", C.c_void_p),
    ]


class GrlUsmArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("taps", C.c_void_p),
        ("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("K", C.c_int32),
        ("quantise", C.c_int32),
        ("weight", C.c_float), ("threshold", C.c_float),
        ("workspace", C.c_void_p),
        ("out", C.c_void_p),
    ]


class GrlCvResizeArgs(_Strict):
    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("src_elems", C.c_int64), ("dst_elems", C.c_int64),
        ("items", C.c_void_p),
        ("n_items", C.c_int32), ("C", C.c_int32),
        ("max_ho", C.c_int32), ("max_wo", C.c_int32),
    ]


class GrlBlurItemsArgs(_Strict):
    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("taps", C.c_void_p),
        ("src_elems", C.c_int64), ("dst_elems", C.c_int64), ("taps_elems", C.c_int64),
        ("items", C.c_void_p),
        ("n_items", C.c_int32), ("C", C.c_int32),
        ("max_ho", C.c_int32), ("max_wo", C.c_int32),
        ("max_K", C.c_int32),
        ("reserved0", C.c_int32),
    ]


class GrlVggPrepArgs(_Strict):
    _fields_ = [
        ("image", C.c_void_p),
        ("stride", C.c_int64 * 4),
        ("tok", C.c_void_p),
        ("ldt", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("use_input_norm", C.c_int32), ("range_norm", C.c_int32),
        ("scale", C.c_float),
    ]


class GrlVggTapArgs(_Strict):
    _fields_ = [
        ("fx", C.c_void_p),
        ("fg", C.c_void_p),
        ("ldf", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
        ("pool", C.c_int32), ("pool_dtype", C.c_int32),
        ("px", C.c_void_p),
        ("pg", C.c_void_p),
        ("ldp", C.c_int64),
        ("partial", C.c_void_p),
        ("n_partial", C.c_int32), ("accumulate", C.c_int32),
        ("loss", C.c_void_p),
        ("layer_sum", C.c_void_p),
        ("coef", C.c_float),
        ("k", C.c_float),
        ("dpool", C.c_void_p),
        ("lddp", C.c_int64),
        ("dfx", C.c_void_p),
        ("lddf", C.c_int64),
    ]


class GrlVggGramArgs(_Strict):
    _fields_ = [
        ("f", C.c_void_p),
        ("ldf", C.c_int64),
        ("nb", C.c_int32), ("B", C.c_int32), ("hw", C.c_int32), ("C", C.c_int32),
        ("gram", C.c_void_p),
        ("ws", C.c_void_p),
        ("ws_bytes", C.c_int64),
        ("rowbound", C.c_void_p),
        ("diff", C.c_void_p),
        ("partial", C.c_void_p),
        ("n_partial", C.c_int32), ("accumulate", C.c_int32),
        ("loss", C.c_void_p),
        ("layer_sum", C.c_void_p),
        ("coef", C.c_float),
        ("k", C.c_float),
        ("d", C.c_void_p),
        ("ldd", C.c_int64),
    ]


class GrlLpipsPrepArgs(_Strict):
    _fields_ = [
        ("image", C.c_void_p),
        ("stride", C.c_int64 * 4),
        ("tok", C.c_void_p),
        ("ldt", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("reserved0", C.c_int32),
    ]


class GrlLpipsTapArgs(_Strict):
    _fields_ = [
        ("f", C.c_void_p),
        ("ldf", C.c_int64),
        ("w", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
        ("pool", C.c_int32), ("accumulate", C.c_int32),
        ("pool_out", C.c_void_p),
        ("ldp", C.c_int64),
        ("partial", C.c_void_p),
        ("out", C.c_void_p),
        ("n_partial", C.c_int32), ("reserved0", C.c_int32),
        ("gpartial", C.c_void_p),
        ("gmax", C.c_void_p),
    ]


class GrlLpipsTapBwdArgs(_Strict):
    _fields_ = [
        ("f", C.c_void_p),
        ("ldf", C.c_int64),
        ("w", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("C", C.c_int32),
        ("dpool", C.c_void_p),
        ("lddp", C.c_int64),
        ("d", C.c_void_p),
        ("ldd", C.c_int64),
        ("k", C.c_float),
        ("reserved0", C.c_int32),
    ]


class GrlLpipsPrepBwdArgs(_Strict):
    _fields_ = [
        ("tok", C.c_void_p),
        ("ldt", C.c_int64),
        ("dx", C.c_void_p),
        ("stride", C.c_int64 * 4),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("scale", C.c_float),
    ]


class GrlIspArgs(_Strict):
    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("src_elems", C.c_int64), ("dst_elems", C.c_int64),
        ("items", C.c_void_p),
        ("params", C.c_void_p),
        ("tables", C.c_void_p),
        ("tables_elems", C.c_int64),
        ("normals", C.c_void_p),
        ("normals_elems", C.c_int64),
        ("n_items", C.c_int32), ("C", C.c_int32),
        ("max_h", C.c_int32), ("max_w", C.c_int32),
    ]


class GrlColorJitterArgs(_Strict):
    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("src_elems", C.c_int64), ("dst_elems", C.c_int64),
        ("items", C.c_void_p),
        ("params", C.c_void_p),
        ("partial", C.c_void_p),
        ("n_partial", C.c_int64),
        ("means", C.c_void_p),
        ("n_items", C.c_int32), ("C", C.c_int32),
        ("max_h", C.c_int32), ("max_w", C.c_int32),
    ]


class GrlDihedralPackArgs(_Strict):
    _fields_ = [
        ("x", C.c_void_p),
        ("stride", C.c_int64 * 4),
        ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("out_a", C.c_void_p),
        ("out_b", C.c_void_p),
    ]


class GrlDihedralMergeArgs(_Strict):
    _fields_ = [
        ("member", C.c_void_p * 8),
        ("stride", (C.c_int64 * 4) * 8),
        ("dtype", C.c_int32),
        ("B", C.c_int32), ("C", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32),
        ("reserved0", C.c_int32),
        ("out", C.c_void_p),
    ]


class GrlRemixItem(_Strict):
    _fields_ = [
        ("src_a", C.c_int32), ("src_b", C.c_int32),
        ("x0", C.c_int32), ("y0", C.c_int32),
        ("lam", C.c_float),
    ]


class GrlBatchRemixArgs(_Strict):
    _fields_ = [
        ("lq", C.c_void_p),
        ("lq_stride", C.c_int64 * 4),
        ("gt", C.c_void_p),
        ("gt_stride", C.c_int64 * 4),
        ("B", C.c_int32), ("P", C.c_int32), ("Cl", C.c_int32), ("Cg", C.c_int32),
        ("b", C.c_int32), ("p", C.c_int32), ("s", C.c_int32),
        ("mix", C.c_int32),
        ("items", C.c_void_p),
        ("lq_out", C.c_void_p),
        ("gt_out", C.c_void_p),
    ]


class GrlSpectralNormArgs(_Strict):
    _fields_ = [
        ("w", C.c_void_p * 16),
        ("u", C.c_void_p * 16),
        ("v", C.c_void_p * 16),
        ("out", C.c_void_p * 16),
        ("u_keep", C.c_void_p * 16),
        ("v_keep", C.c_void_p * 16),
        ("sigma", C.c_void_p * 16),
        ("g", C.c_void_p * 16),
        ("cout", C.c_int32 * 16),
        ("k", C.c_int32 * 16),
        ("n_layers", C.c_int32), ("advance", C.c_int32),
        ("ws", C.c_void_p),
        ("ws_bytes", C.c_int64),
    ]


SN_MAX_LAYERS = 16


class GrlTileStitchArgs(_Strict):
    _fields_ = [
        ("canvas", C.c_void_p),
        ("tiles", C.c_void_p),
        ("win", C.c_void_p),
        ("b", C.c_int32), ("c", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("tile", C.c_int32), ("scale", C.c_int32),
        ("ny", C.c_int32), ("nx", C.c_int32),
        ("lo", C.c_int32), ("hi", C.c_int32),
        ("oy", C.c_int32 * 256),
        ("ox", C.c_int32 * 256),
    ]


STITCH_MAX_ORIGINS = 256


_I32, _I64, _PTR = C.c_int32, C.c_int64, C.c_void_p


def _launch(args_struct):
    """int f(void* stream, const GrlXArgs* args): the shape of almost every entry point."""
    return (C.c_int, [_PTR, C.POINTER(args_struct)])


# every symbol include/grl_hip.h declares, in the header's order: name -> (restype, argtypes).  lib() applies this table;
# tests/test_abi.py compares it with the prototypes of the header.
SIGNATURES = {
    "grl_linear_fwd": _launch(GrlLinearArgs),
    "grl_linear_split_blob_bytes": (_I64, [_I32, _I32]),
    "grl_mlp_fwd": _launch(GrlMlpArgs),
    "grl_mlp_blob_bytes": (_I64, [_I32, _I32]),
    "grl_block_tail_fwd": _launch(GrlTailArgs),
    "grl_tail_regs_blob_bytes": (_I64, []),
    "grl_proj_blob_bytes": (_I64, [_I32]),
    "grl_qkv_fwd": _launch(GrlQkvArgs),
    "grl_qkv_blob_bytes": (_I64, [_I32, _I32]),
    "grl_qkv_anchor_fwd": _launch(GrlQkvAnchorArgs),
    "grl_qkv_anchor_blob_bytes": (_I64, [_I32, _I32, _I32]),
    "grl_qkv_anchor_lo_blob_bytes": (_I64, [_I32, _I32]),
    "grl_attention_fwd": _launch(GrlAttnArgs),
    "grl_attention_rows_geometry_ok": (C.c_int, [C.POINTER(GrlAttnArgs)]),
    "grl_conv3x3_fwd": _launch(GrlConvArgs),
    "grl_conv3x3_num_workgroups": (C.c_int, [_I32, _I32, _I32]),
    "grl_cab_conv2_fwd": _launch(GrlCabConv2Args),
    "grl_cab_conv2_blob_bytes": (_I64, []),
    "grl_se_scale_fwd": (C.c_int, [_PTR, _PTR] + [_I32] * 6 + [_PTR] * 5),
    "grl_layernorm_fwd": (C.c_int, [_PTR, _PTR, _I64, _PTR, _I64, _PTR, _PTR, _I32, _I32, _I32, C.c_float]),
    "grl_layernorm_res_fwd": _launch(GrlLnResArgs),
    "grl_gemm_tn": _launch(GrlGemmTnArgs),
    "grl_attention_bwd": _launch(GrlAttnBwdArgs),
    "grl_adamw_step": _launch(GrlAdamWArgs),
    "grl_grad_sqnorm": _launch(GrlGradNormArgs),
    "grl_grad_clip_finish": _launch(GrlGradClipArgs),
    "grl_layernorm_train_fwd": _launch(GrlLnTrainArgs),
    "grl_layernorm_bwd": _launch(GrlLnTrainArgs),
    "grl_pack_conv3x3": (C.c_int, [_PTR] * 5 + [_I32] * 5),
    "grl_pack_linear": (C.c_int, [_PTR] * 6 + [_I32] * 4),
    "grl_sum4": (C.c_int, [_PTR] * 6 + [_I64]),
    "grl_head_planes_fwd": _launch(GrlPlanesArgs),
    "grl_head_planes_bwd": _launch(GrlPlanesArgs),
    "grl_se_mlp_fwd": _launch(GrlSeMlpArgs),
    "grl_se_mlp_bwd": _launch(GrlSeMlpArgs),
    "grl_se_colsum": _launch(GrlSeRowsArgs),
    "grl_se_apply": _launch(GrlSeRowsArgs),
    "grl_cpb_table_fwd": _launch(GrlCpbArgs),
    "grl_cpb_table_bwd": _launch(GrlCpbArgs),
    "grl_image_metrics_workspace_bytes": (_I64, [_I32] * 4),
    "grl_image_metrics": _launch(GrlMetricArgs),
    "grl_demosaic_matlab": _launch(GrlDemosaicArgs),
    "grl_imresize": _launch(GrlResizeArgs),
    "grl_image_niqe_workspace_bytes": (_I64, [_I32] * 3),
    "grl_image_niqe_features": _launch(GrlNiqeArgs),
    "grl_sample_patches": _launch(GrlPatchArgs),
    "grl_sample_patch_views": _launch(GrlPatchViewsArgs),
    "grl_blur_depthwise": _launch(GrlBlurArgs),
    "grl_jpeg_workspace_bytes": (_I64, [_I32] * 4),
    "grl_jpeg_roundtrip": _launch(GrlJpegArgs),
    "grl_image_pack8": _launch(GrlPack8Args),
    "grl_usm_workspace_bytes": (_I64, [_I32] * 4),
    "grl_usm_sharp": _launch(GrlUsmArgs),
    "grl_cv_resize": _launch(GrlCvResizeArgs),
    "grl_blur_items": _launch(GrlBlurItemsArgs),
    "grl_conv4x4s2_fwd": _launch(GrlConvArgs),
    "grl_conv4x4s2_bwd_data": _launch(GrlConvArgs),
    "grl_pack_conv4x4": (C.c_int, [_PTR] * 3 + [_I32] * 5),
    "grl_upsample2x_bilinear_fwd": (C.c_int, [_PTR, _PTR, _I64, _PTR, _I64] + [_I32] * 4),
    "grl_upsample2x_bilinear_bwd": (C.c_int, [_PTR, _PTR, _I64, _PTR, _I64] + [_I32] * 4),
    "grl_vgg_prep_fwd": _launch(GrlVggPrepArgs),
    "grl_vgg_prep_bwd": _launch(GrlVggPrepArgs),
    "grl_vgg_tap_num_workgroups": (C.c_int, [_I32] * 4),
    "grl_vgg_tap_fwd": _launch(GrlVggTapArgs),
    "grl_vgg_tap_bwd": _launch(GrlVggTapArgs),
    "grl_vgg_gram_workspace_bytes": (_I64, [_I32] * 3),
    "grl_vgg_gram_loss_num_workgroups": (C.c_int, [_I32] * 2),
    "grl_vgg_gram_fwd": _launch(GrlVggGramArgs),
    "grl_vgg_gram_loss": _launch(GrlVggGramArgs),
    "grl_vgg_gram_bwd": _launch(GrlVggGramArgs),
    "grl_lpips_prep": _launch(GrlLpipsPrepArgs),
    "grl_lpips_tap_num_workgroups": (C.c_int, [_I32] * 4),
    "grl_lpips_tap": _launch(GrlLpipsTapArgs),
    "grl_lpips_tap_bwd": _launch(GrlLpipsTapBwdArgs),
    "grl_lpips_prep_bwd": _launch(GrlLpipsPrepBwdArgs),
    "grl_isp_unprocess": _launch(GrlIspArgs),
    "grl_isp_process": _launch(GrlIspArgs),
    "grl_isp_roundtrip": _launch(GrlIspArgs),
    "grl_color_jitter_num_workgroups": (C.c_int, [_I32] * 2),
    "grl_color_jitter": _launch(GrlColorJitterArgs),
    "grl_dihedral_pack": _launch(GrlDihedralPackArgs),
    "grl_dihedral_merge": _launch(GrlDihedralMergeArgs),
    "grl_batch_remix": _launch(GrlBatchRemixArgs),
    "grl_spectral_norm_fwd": _launch(GrlSpectralNormArgs),
    "grl_spectral_norm_bwd": _launch(GrlSpectralNormArgs),
    "grl_tile_stitch": _launch(GrlTileStitchArgs),
    "grl_debug_dirty_lds": (C.c_int, [_PTR]),
    "grl_abi_version": (C.c_int, []),
    "grl_build_info": (C.c_char_p, []),
}
EXPORTS = list(SIGNATURES)

_lib = None


def lib():
    """Loads the library once; raises if it is missing or built against another ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the GRL HIP extension is not built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` from the repo root. "
            "There is no CPU/PyTorch fallback for the hot path."
        )
    L = C.CDLL(LIB_PATH)
    if L.grl_abi_version() != ABI_VERSION:      # int f(void): right under ctypes' defaults, before the table is applied
        raise RuntimeError(f"stale {LIB_PATH}: ABI {L.grl_abi_version()} != {ABI_VERSION}; rebuild")
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(code: int, what: str):
    if code != 0:
        kind = {-1: "bad argument", -2: "unsupported shape"}.get(code, f"hipError {code}")
        raise RuntimeError(f"libgrl_hip: {what} failed: {kind}")


_DIRTY_LDS = SW.on("GRL_DIRTY_LDS")


def set_dirty_lds(flag: bool) -> bool:
    """Switch the dirty-LDS mode at run time (tests); returns the previous setting.  Read per call in stream_ptr()."""
    global _DIRTY_LDS
    prev, _DIRTY_LDS = _DIRTY_LDS, bool(flag)
    return prev


def stream_ptr():
    """The current torch HIP stream as the `stream` argument of a C-ABI launch (every wrapper evaluates this right before its
    call).  GRL_DIRTY_LDS=1 (debug): first fills the LDS of every CU with NaN bytes on that stream, so that the kernel about to be
    launched cannot profit from what its predecessor left there (grl_debug_dirty_lds)."""
    import torch

    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if _DIRTY_LDS:
        check(lib().grl_debug_dirty_lds(s), "grl_debug_dirty_lds")
    return s


def launch(name: str, args):
    """Calls entry point `name` of the shape int f(void* stream, const GrlXArgs* args) on the current stream and raises under
    that same name unless it returns 0."""
    fn = getattr(lib(), name)
    check(fn(stream_ptr(), C.byref(args)), name)
