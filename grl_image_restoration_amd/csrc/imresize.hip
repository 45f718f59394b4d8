// MATLAB's antialiased bicubic imresize as one separable resampling launch (include/grl_hip.h, grl_imresize): the reference's
// ``imresize`` (utils/matlab_functions.py:91-188), which builds the classical-SR LQ of every training item
// (data/datasets/restoration_sr.py:130-141), ``bicubic_degradation`` (utils/utils_bsr/utils_sisr.py:210-219) and NIQE's pyramid.
//
// The resampling is described by two tables per axis that the host computes in float64 (tasks.resize_tables, a restatement of
// calculate_weights_indices, matlab_functions.py:20-88, with the symmetric padding of lines 137-148 / 161-172 folded into the
// indices): for output index o, `taps` weights and `taps` zero-based input indices.  The kernel knows nothing of scales or cubics:
// it serves every factor, both directions, and any other separable table.  Rows first, columns second (the reference's order).
//
// Arithmetic: every weighted sum is accumulated in fp64 (fp32 sample x fp64 weight).  The strip between the two passes is HELD IN
// FP64, so a result is rounded once, to fp32, at the store; `quantize` then applies the reference's tensor_round to that fp32 value
// in fp32 (clamp to [0, 1], x 255, round half to even, / 255 with a correctly rounded division), as torch does.  `out_f64` stores the
// fp64 sum itself, unrounded (NIQE's half-scale plane, csrc/niqe.hip).
//
// Shape: a workgroup of 256 threads owns TOY x TOX output pixels of one (image, channel) plane.
//   1. the tile's slices of the four tables go to LDS (indices clamped to the image while loading; the column tables transposed, so
//      that lanes with adjacent output columns read adjacent words) and their index ranges [r0, r1] x [c0, c1] are reduced;
//   2. the input window r0..r1 x c0..c1 is staged in LDS by coalesced row reads (float4 where the column stride is 1 and the plane
//      is 16-byte aligned: the window then starts at c0 rounded down to a multiple of 4);
//   3. vertical pass: strip[oy][c] = sum_t wh[oy][t] * in[ih[oy][t]][c] for every staged column, lanes along c;
//   4. horizontal pass: out[oy][ox] = sum_t ww[ox][t] * strip[oy][iw[ox][t]], lanes along ox, stored coalesced.
// Partial tiles at the right and bottom edges load, compute and store only what exists.
//
// LDS byte map (dynamic, in this order; SH x SWP is the window capacity the launcher sizes from H / out_h, W / out_w and the taps,
// SWP a multiple of 4):
//   window  float  [SH][SWP]       strip  double [TOY][SWP]       wh  double [TOY][taps_h]     ww  double [taps_w][TOX]
//   ih      int    [TOY][taps_h]   iw     int    [taps_w][TOX]    range  int [4]  (r0, r1, c0, c1)
// The launcher takes the first of the tiles 16x64, 8x64, 16x32, 8x32, 4x32, 4x16, 2x16, 1x16 whose map fits 64 KiB.  At 1/4
// (16 taps) that is 8 x 32: window 51 x 156 fp32 = 31.8 KB, strip 10 KB, tables 7.7 KB -- 49.5 KB, three workgroups per CU; at 1/2
// (8 taps) 16 x 64: window 43 x 148 = 25.5 KB, strip 18.9 KB, tables 7.7 KB -- 52 KB.  The capacity bound holds for every MATLAB
// table (the first index advances by 1 / scale per output and 1 / scale < H / (out_h - 1)); a tile of a foreign table whose indices
// spread further, or taps so many that no tile fits (scales below about 1/30), takes the direct path: the same sums, samples and
// tables read from global memory.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int LDS_BUDGET = 64 * 1024;

struct Params {
    const float* in;
    int64_t sn, sc, sy, sx;
    int32_t C, H, W, out_h, out_w, taps_h, taps_w;
    int32_t toy, tox, nty, ntx, SH, SWP;    // SH = 0: no LDS map, every tile takes the direct path
    int32_t vec4, quantize, out_f64;
    const double *wh, *ww;
    const int32_t *ih, *iw;
    float* out;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the reference's tensor_round on an fp32 value, in fp32 (NaN propagates, as through torch's clamp)
__device__ __forceinline__ float round8(float v) {
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    return rintf(v * 255.0f) / 255.0f;
}

__global__ __launch_bounds__(NT) void imresize_kernel(Params p) {
    extern __shared__ float4 lds[];

    const int tiles = p.nty * p.ntx;
    const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
    const int n = plane / p.C, ch = plane - n * p.C;
    const int oy0 = (t / p.ntx) * p.toy, ox0 = (t % p.ntx) * p.tox;
    const int ny = min(p.toy, p.out_h - oy0), nx = min(p.tox, p.out_w - ox0);
    const float* const src = p.in + n * p.sn + ch * p.sc;
    float* const dst = p.out + (int64_t)plane * p.out_h * p.out_w * (p.out_f64 ? 2 : 1);    // fp64 planes are twice as long
    const int tid = threadIdx.x, th = p.taps_h, tw = p.taps_w;

    if (p.SH > 0) {
        float* const win = reinterpret_cast<float*>(lds);
        double* const strip = reinterpret_cast<double*>(win + p.SH * p.SWP);
        double* const wh = strip + p.toy * p.SWP;
        double* const ww = wh + p.toy * th;
        int* const ih = reinterpret_cast<int*>(ww + tw * p.tox);
        int* const iw = ih + p.toy * th;
        int* const rng = iw + tw * p.tox;

        // 1. tables and their index ranges
        if (tid == 0) { rng[0] = p.H; rng[1] = -1; rng[2] = p.W; rng[3] = -1; }
        __syncthreads();
        int lo = p.H, hi = -1;
        for (int i = tid; i < ny * th; i += NT) {
            const int64_t g = (int64_t)oy0 * th + i;
            const int v = clampi(p.ih[g], p.H - 1);
            wh[i] = p.wh[g];
            ih[i] = v;
            lo = min(lo, v); hi = max(hi, v);
        }
        if (hi >= 0) { atomicMin(&rng[0], lo); atomicMax(&rng[1], hi); }
        lo = p.W; hi = -1;
        for (int i = tid; i < nx * tw; i += NT) {
            const int x = i / tw, k = i - x * tw;
            const int64_t g = (int64_t)ox0 * tw + i;
            const int v = clampi(p.iw[g], p.W - 1);
            ww[k * p.tox + x] = p.ww[g];
            iw[k * p.tox + x] = v;
            lo = min(lo, v); hi = max(hi, v);
        }
        if (hi >= 0) { atomicMin(&rng[2], lo); atomicMax(&rng[3], hi); }
        __syncthreads();

        const int r0 = rng[0], r1 = rng[1], c1 = rng[3];
        const int c0 = p.vec4 ? (rng[2] & ~3) : rng[2];
        const int nr = r1 - r0 + 1, nc = c1 - c0 + 1;
        if (nr <= p.SH && nc <= p.SWP) {               // uniform over the workgroup
            // 2. the input window
            if (p.vec4) {
                const int nq = (nc + 3) >> 2;
                for (int i = tid; i < nr * nq; i += NT) {
                    const int r = i / nq, q = i - r * nq;
                    const int c = c0 + 4 * q;
                    const float* g = src + (int64_t)(r0 + r) * p.sy + c;
                    float4 v;
                    if (c + 3 < p.W) {
                        v = *reinterpret_cast<const float4*>(g);
                    } else {                               // the image's last, partial quad
                        v.x = g[0];
                        v.y = c + 1 < p.W ? g[1] : 0.f;
                        v.z = c + 2 < p.W ? g[2] : 0.f;
                        v.w = 0.f;
                    }
                    *reinterpret_cast<float4*>(win + r * p.SWP + 4 * q) = v;
                }
            } else {
                for (int i = tid; i < nr * nc; i += NT) {
                    const int r = i / nc, c = i - r * nc;
                    win[r * p.SWP + c] = src[(int64_t)(r0 + r) * p.sy + (int64_t)(c0 + c) * p.sx];
                }
            }
            __syncthreads();
            // 3. vertical pass over every staged column
            for (int i = tid; i < ny * nc; i += NT) {
                const int oy = i / nc, c = i - oy * nc;
                const double* w = wh + oy * th;
                const int* ix = ih + oy * th;
                double acc = 0.0;
                for (int k = 0; k < th; ++k) acc += w[k] * (double)win[(ix[k] - r0) * p.SWP + c];
                strip[oy * p.SWP + c] = acc;
            }
            __syncthreads();
            // 4. horizontal pass
            const int lx = tid % p.tox;
            if (lx < nx) {
                for (int oy = tid / p.tox; oy < ny; oy += NT / p.tox) {
                    const double* s = strip + oy * p.SWP - c0;
                    double acc = 0.0;
                    for (int k = 0; k < tw; ++k) acc += ww[k * p.tox + lx] * s[iw[k * p.tox + lx]];
                    const int64_t o = (int64_t)(oy0 + oy) * p.out_w + ox0 + lx;
                    const float v = (float)acc;
                    if (p.out_f64) reinterpret_cast<double*>(dst)[o] = acc;
                    else dst[o] = p.quantize ? round8(v) : v;
                }
            }
            return;
        }
    }

    // direct path: the same two sums per output pixel, samples and tables from global memory
    const int lx = tid % p.tox;
    if (lx >= nx) return;
    const double* gww = p.ww + (int64_t)(ox0 + lx) * tw;
    const int32_t* giw = p.iw + (int64_t)(ox0 + lx) * tw;
    for (int oy = tid / p.tox; oy < ny; oy += NT / p.tox) {
        const double* gwh = p.wh + (int64_t)(oy0 + oy) * th;
        const int32_t* gih = p.ih + (int64_t)(oy0 + oy) * th;
        double acc = 0.0;
        for (int k = 0; k < tw; ++k) {
            const float* col = src + (int64_t)clampi(giw[k], p.W - 1) * p.sx;
            double v = 0.0;
            for (int j = 0; j < th; ++j) v += gwh[j] * (double)col[(int64_t)clampi(gih[j], p.H - 1) * p.sy];
            acc += gww[k] * v;
        }
        const int64_t o = (int64_t)(oy0 + oy) * p.out_w + ox0 + lx;
        const float v = (float)acc;
        if (p.out_f64) reinterpret_cast<double*>(dst)[o] = acc;
        else dst[o] = p.quantize ? round8(v) : v;
    }
}

// rows / columns of the input that `tile` consecutive outputs of a MATLAB table can reach (see the header comment)
int64_t reach(int64_t tile, int64_t in_len, int64_t out_len, int64_t taps) {
    const int64_t r = (tile * in_len + out_len - 1) / out_len + taps + 3;
    return r < in_len ? r : in_len;
}

int64_t lds_bytes(int64_t toy, int64_t tox, int64_t SH, int64_t SWP, int64_t th, int64_t tw) {
    return 4 * SH * SWP + 8 * toy * SWP + 12 * (toy * th + tw * tox) + 16;
}

}  // namespace

extern "C" int grl_imresize(void* stream, const GrlResizeArgs* a) {
    if (!a || !a->src || !a->out || !a->wh || !a->ih || !a->ww || !a->iw) return GRL_ERR_BAD_ARG;
    if (a->N <= 0 || a->C <= 0 || a->H <= 0 || a->W <= 0 || a->out_h <= 0 || a->out_w <= 0) return GRL_ERR_BAD_ARG;
    if (a->taps_h < 1 || a->taps_w < 1) return GRL_ERR_BAD_ARG;
    if ((uint64_t)a->wh % 8 || (uint64_t)a->ww % 8 || (uint64_t)a->ih % 4 || (uint64_t)a->iw % 4 || (uint64_t)a->out % 4 ||
        (uint64_t)a->src % 4)
        return GRL_ERR_BAD_ARG;
    if (a->out_f64 && (a->quantize || (uint64_t)a->out % 8)) return GRL_ERR_BAD_ARG;

    static const int TILES[][2] = {{16, 64}, {8, 64}, {16, 32}, {8, 32}, {4, 32}, {4, 16}, {2, 16}, {1, 16}};
    Params p;
    p.in = a->src;
    p.sn = a->stride[0]; p.sc = a->stride[1]; p.sy = a->stride[2]; p.sx = a->stride[3];
    p.C = a->C; p.H = a->H; p.W = a->W; p.out_h = a->out_h; p.out_w = a->out_w; p.taps_h = a->taps_h; p.taps_w = a->taps_w;
    p.vec4 = p.sx == 1 && (uint64_t)a->src % 16 == 0 && p.sn % 4 == 0 && p.sc % 4 == 0 && p.sy % 4 == 0;
    p.quantize = a->quantize != 0;
    p.out_f64 = a->out_f64 != 0;
    p.wh = a->wh; p.ww = a->ww; p.ih = a->ih; p.iw = a->iw;
    p.out = a->out;
    p.toy = 8; p.tox = 32; p.SH = 0; p.SWP = 0;
    size_t shmem = 0;
    for (const auto& tl : TILES) {
        const int64_t SH = reach(tl[0], a->H, a->out_h, a->taps_h);
        const int64_t SWP = (reach(tl[1], a->W, a->out_w, a->taps_w) + 3 + 3) & ~(int64_t)3;   // + the shift to a quad start
        const int64_t bytes = lds_bytes(tl[0], tl[1], SH, SWP, a->taps_h, a->taps_w);
        if (bytes <= LDS_BUDGET) {
            p.toy = tl[0]; p.tox = tl[1]; p.SH = (int32_t)SH; p.SWP = (int32_t)SWP;
            shmem = (size_t)bytes;
            break;
        }
    }
    p.nty = (a->out_h + p.toy - 1) / p.toy;
    p.ntx = (a->out_w + p.tox - 1) / p.tox;
    const int64_t grid = (int64_t)a->N * a->C * p.nty * p.ntx;
    if (grid > 0x7fffffff) return GRL_ERR_BAD_ARG;

    hipLaunchKernelGGL(imresize_kernel, dim3((unsigned)grid), dim3(NT), shmem, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
