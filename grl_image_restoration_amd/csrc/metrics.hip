// Image-quality metrics of the reference's validation step (include/grl_hip.h, grl_image_metrics): PSNR, SSIM and PSNR-B on the RGB
// planes and on the matlab Y plane, for whole (B, C, H, W) fp32 images in one tile pass plus a per-image reduction.
//
// Tile pass: a workgroup owns TH x TW output pixels of one image and stages that tile plus a 5-pixel halo of both images in LDS as
// 8-bit values -- tensor_round makes every value k / 255, and the Y plane is an integer grid too, so one byte per pixel and plane holds
// the rounded RGB planes and Y after one global read.  From the bytes it forms, in exact integer arithmetic, the squared-error sums
// and PSNR-B's four neighbour-difference sums (each difference belongs to the tile of its left / upper pixel), and, per plane, the
// five Gaussian moments (x, y, x^2, y^2, xy) by a horizontal then a vertical 11-tap pass in fp64, then the SSIM map.  fp64 keeps the
// E[x^2] - E[x]^2 cancellation of the variance terms below 1e-9 of SSIM (in fp32 it is ~1e-5 on smooth images).  The partial sums
// of a workgroup go to its own workspace row; the second launch adds the rows of an image in a fixed order and forms the metrics,
// so the result is bitwise reproducible.
#include "common.h"

namespace {

constexpr int TW = 64, TH = 32, HALO = 5;
constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO, LP = LW + 2;   // staged tile: 42 x 74, rows padded to 76
constexpr int RPT = TH / 4;                                          // output rows per thread (4 waves stacked vertically)
// per-workgroup partial sums: plane pl (0..2 R, G, B or the grey plane; 3 Y) has 5 integer slots (units of 1/255^2):
//   squared error, boundary horizontal, boundary vertical, non-boundary horizontal, non-boundary vertical differences of `restored`;
//   then the SSIM map sums of the colour planes and of Y
constexpr int NINT = 20, SLOT_SSIM = 20, SLOT_SSIM_Y = 21, NSLOT = 22;

struct Params {
    const float* img[2];     // restored, target (already offset by the shave border)
    int64_t st[2][4];        // element strides b, c, h, w
    int32_t B, C, H, W;      // H, W after the shave
    int32_t metrics, ntx, nty;
    double taps[11];
    float y_coef[3];
    double* ws;
    double* out;
};

__device__ __forceinline__ uint32_t round8(float v) {
    return (uint32_t)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f);   // tensor_round: clamp, round(x 255)
}

__device__ __forceinline__ float unit(uint32_t k) { return (float)k / 255.f; }

// utils_image.py:43-79 (rgb2ycbcr, only_y) on rounded inputs, in the fp32 operation order of torch's CPU product
__device__ __forceinline__ uint32_t luma(uint32_t r, uint32_t g, uint32_t b, const float* w) {
    const float tr = unit(r) * 255.f, tg = unit(g) * 255.f, tb = unit(b) * 255.f;
    return (uint32_t)rintf(__builtin_fmaf(tb, w[2], __builtin_fmaf(tg, w[1], tr * w[0])) + 16.f);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(256) void metrics_tile_kernel(Params p) {
    __shared__ uint8_t q[2][4][LH][LP];    // 8-bit planes of restored / target: R, G, B (or grey), Y
    __shared__ float f[2][LH][LP];         // the plane SSIM is working on, as the fp32 values the reference sees
    __shared__ double red[4][NSLOT];
    __shared__ double tz[32];              // taps at 10..20, zeros around: the vertical pass indexes them by (row - output row)

    if (threadIdx.x < 32) tz[threadIdx.x] = (threadIdx.x >= 10 && threadIdx.x <= 20) ? p.taps[threadIdx.x - 10] : 0.0;
    const int tiles = p.ntx * p.nty;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int y0 = (t / p.ntx) * TH, x0 = (t % p.ntx) * TW;
    const int C = p.C;
    const bool want_y = (p.metrics & (GRL_METRIC_PSNR_Y | GRL_METRIC_SSIM_Y | GRL_METRIC_PSNRB_Y)) != 0;

    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int r = i / LW, c = i - r * LW;
        const int gy = y0 - HALO + r, gx = x0 - HALO + c;
        const bool in = gy >= 0 && gy < p.H && gx >= 0 && gx < p.W;   // zero padding of conv2d outside the (shaved) image
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            uint32_t k[3] = {0, 0, 0};
            const float* src = p.img[s] + b * p.st[s][0] + gy * p.st[s][2] + gx * p.st[s][3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                if (ch < C) {
                    if (in) k[ch] = round8(src[ch * p.st[s][1]]);
                    q[s][ch][r][c] = (uint8_t)k[ch];
                }
            if (want_y) q[s][3][r][c] = in ? (uint8_t)luma(k[0], k[1], k[2], p.y_coef) : 0;
        }
    }
    __syncthreads();

    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int j = x0 + tx, lx = tx + HALO;

    // squared errors and PSNR-B's difference sums (psnrb.py:22-100): exact integers
    uint32_t acc[NINT];
#pragma unroll
    for (int s = 0; s < NINT; ++s) acc[s] = 0;
    for (int rr = 0; rr < RPT; ++rr) {
        const int i = y0 + ty * RPT + rr, ly = ty * RPT + rr + HALO;
        if (j >= p.W || i >= p.H) continue;
#pragma unroll
        for (int pl = 0; pl < 4; ++pl) {
            if (!(pl < C || (pl == 3 && want_y))) continue;
            const int a = q[0][pl][ly][lx], d = a - (int)q[1][pl][ly][lx];
            acc[pl * 5] += (uint32_t)(d * d);
            if (j < p.W - 1) {                                  // block boundary between columns j and j+1: j % 8 == 7
                const int h = a - (int)q[0][pl][ly][lx + 1];
                const uint32_t hh = (uint32_t)(h * h);
                const bool blk = (j & 7) == 7;
                acc[pl * 5 + 1] += blk ? hh : 0u;
                acc[pl * 5 + 3] += blk ? 0u : hh;
            }
            if (i < p.H - 1) {
                const int v = a - (int)q[0][pl][ly + 1][lx];
                const uint32_t vv = (uint32_t)(v * v);
                const bool blk = (i & 7) == 7;
                acc[pl * 5 + 2] += blk ? vv : 0u;
                acc[pl * 5 + 4] += blk ? 0u : vv;
            }
        }
    }

    // SSIM (ssim.py:33-69): separable Gaussian moments in fp64; thread (tx, ty) owns column j, rows ty*RPT .. ty*RPT+RPT-1 of the tile
    double ssum = 0.0, ssum_y = 0.0;
    for (int pl = 0; pl < 4; ++pl) {
        const bool on = pl < C ? (p.metrics & GRL_METRIC_SSIM) != 0 : (pl == 3 && (p.metrics & GRL_METRIC_SSIM_Y) != 0);
        if (!on) continue;                                      // uniform over the workgroup
        __syncthreads();                                        // the previous plane's readers are done with f
        for (int i = threadIdx.x; i < LH * LW; i += 256) {
            const int r = i / LW, c = i - r * LW;
            f[0][r][c] = unit(q[0][pl][r][c]);
            f[1][r][c] = unit(q[1][pl][r][c]);
        }
        __syncthreads();
        double m[RPT][5];
#pragma unroll
        for (int o = 0; o < RPT; ++o)
#pragma unroll
            for (int e = 0; e < 5; ++e) m[o][e] = 0.0;
#pragma unroll 2
        for (int rr = 0; rr < RPT + 2 * HALO; ++rr) {
            const int ly = ty * RPT + rr;
            double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0, h4 = 0.0;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const double x = f[0][ly][tx + k], y = f[1][ly][tx + k], w = tz[10 + k];
                h0 += w * x;
                h1 += w * y;
                h2 += w * (x * x);
                h3 += w * (y * y);
                h4 += w * (x * y);
            }
#pragma unroll
            for (int o = 0; o < RPT; ++o) {
                const double w = tz[10 + rr - o];
                m[o][0] += w * h0;
                m[o][1] += w * h1;
                m[o][2] += w * h2;
                m[o][3] += w * h3;
                m[o][4] += w * h4;
            }
        }
        const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
        double s = 0.0;
#pragma unroll
        for (int o = 0; o < RPT; ++o) {
            const double mu1 = m[o][0], mu2 = m[o][1];
            const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
            const double s1 = m[o][2] - mu1_sq, s2 = m[o][3] - mu2_sq, s12 = m[o][4] - mu1_mu2;
            const double v = ((2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
            if (j < p.W && y0 + ty * RPT + o < p.H) s += v;
        }
        if (pl == 3) ssum_y += s;
        else ssum += s;
    }

    // workgroup sums in a fixed order: integer slots exact in uint32 (<= 2048 pixels x 255^2), then fp64
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < NINT; ++s) {
        const uint32_t v = wave_sum(acc[s]);
        if (lane == 0) red[ty][s] = (double)v;
    }
    const double sv = wave_sum(ssum), svy = wave_sum(ssum_y);
    if (lane == 0) {
        red[ty][SLOT_SSIM] = sv;
        red[ty][SLOT_SSIM_Y] = svy;
    }
    __syncthreads();
    if (threadIdx.x < NSLOT) {
        const int s = threadIdx.x;
        p.ws[(int64_t)blockIdx.x * NSLOT + s] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
    }
}

__device__ double psnrb_term(const double* sl, double H, double W, double N) {
    // psnrb.py:22-115 for one plane, including its normalising counts for sides that are not multiples of 8
    const double inv = 1.0 / (255.0 * 255.0);
    const double mse = sl[0] * inv / N;
    const double n_bh = H * (floor(W / 8.0) - 1.0), n_bv = W * (floor(H / 8.0) - 1.0);
    const double bd = (sl[1] + sl[2]) * inv / (n_bh + n_bv);
    const double nbd = (sl[3] + sl[4]) * inv / ((H * (W - 1.0) - n_bh) + (W * (H - 1.0) - n_bv));
    const double scaler = 3.0 / log2(fmin(H, W));
    const double bef = bd <= nbd ? 0.0 : scaler * (bd - nbd);
    return 10.0 * log10(1.0 / (mse + bef));
}

__global__ __launch_bounds__(256) void metrics_final_kernel(Params p) {
    __shared__ double red[4][NSLOT];
    const int b = blockIdx.x, tiles = p.ntx * p.nty;
    const double* ws = p.ws + (int64_t)b * tiles * NSLOT;
    double v[NSLOT];
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) v[s] = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 256)
#pragma unroll
        for (int s = 0; s < NSLOT; ++s) v[s] += ws[(int64_t)t * NSLOT + s];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
        const double r = wave_sum(v[s]);
        if (lane == 0) red[wv][s] = r;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sl[NSLOT];
    for (int s = 0; s < NSLOT; ++s) sl[s] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
    const double H = p.H, W = p.W, N = H * W, inv = 1.0 / (255.0 * 255.0);
    const int C = p.C;
    double o[GRL_METRIC_COUNT];
    for (int i = 0; i < GRL_METRIC_COUNT; ++i) o[i] = __builtin_nan("");
    if (p.metrics & GRL_METRIC_PSNR) {
        double sse = 0.0;
        for (int c = 0; c < C; ++c) sse += sl[c * 5];
        o[0] = -10.0 * log10(sse * inv / (C * N));
    }
    if (p.metrics & GRL_METRIC_PSNR_Y) o[1] = -10.0 * log10(sl[15] * inv / N);
    if (p.metrics & GRL_METRIC_SSIM) o[2] = sl[SLOT_SSIM] / (C * N);
    if (p.metrics & GRL_METRIC_SSIM_Y) o[3] = sl[SLOT_SSIM_Y] / N;
    if (p.metrics & GRL_METRIC_PSNRB) {
        double tot = 0.0;
        for (int c = 0; c < C; ++c) tot += psnrb_term(sl + c * 5, H, W, N);
        o[4] = tot / C;
    }
    if (p.metrics & GRL_METRIC_PSNRB_Y) o[5] = psnrb_term(sl + 15, H, W, N);
    for (int i = 0; i < GRL_METRIC_COUNT; ++i) p.out[b * GRL_METRIC_COUNT + i] = o[i];
}

int64_t tiles_of(int32_t H, int32_t W, int32_t border) {
    const int64_t h = (int64_t)H - 2 * (int64_t)border, w = (int64_t)W - 2 * (int64_t)border;
    return ((h + TH - 1) / TH) * ((w + TW - 1) / TW);
}

}  // namespace

extern "C" int64_t grl_image_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t border) {
    if (B <= 0 || border < 0 || 2 * (int64_t)border >= H || 2 * (int64_t)border >= W) return 0;
    return (int64_t)B * tiles_of(H, W, border) * NSLOT * (int64_t)sizeof(double);
}

extern "C" int grl_image_metrics(void* stream, const GrlMetricArgs* a) {
    if (!a || !a->restored || !a->target || !a->out || !a->workspace) return GRL_ERR_BAD_ARG;
    for (int d = 0; d < 4; ++d)
        if (a->shape[d] != a->target_shape[d] || a->restored_stride[d] < 0 || a->target_stride[d] < 0) return GRL_ERR_BAD_ARG;
    const int32_t B = a->shape[0], C = a->shape[1], H = a->shape[2], W = a->shape[3], bd = a->border;
    const int all = (1 << GRL_METRIC_COUNT) - 1, ys = GRL_METRIC_PSNR_Y | GRL_METRIC_SSIM_Y | GRL_METRIC_PSNRB_Y;
    if (B <= 0 || (C != 1 && C != 3) || bd < 0 || 2 * (int64_t)bd >= H || 2 * (int64_t)bd >= W) return GRL_ERR_BAD_ARG;
    if (a->metrics <= 0 || (a->metrics & ~all) || (C == 1 && (a->metrics & ys))) return GRL_ERR_BAD_ARG;
    const int64_t tiles = tiles_of(H, W, bd), grid = (int64_t)B * tiles;
    if (grid > 0x7fffffff || a->workspace_bytes < grl_image_metrics_workspace_bytes(B, H, W, bd)) return GRL_ERR_BAD_ARG;

    Params p;
    const float* src[2] = {a->restored, a->target};
    const int64_t* st[2] = {a->restored_stride, a->target_stride};
    for (int s = 0; s < 2; ++s) {
        for (int d = 0; d < 4; ++d) p.st[s][d] = st[s][d];
        p.img[s] = src[s] + (int64_t)bd * (st[s][2] + st[s][3]);
    }
    p.B = B; p.C = C; p.H = H - 2 * bd; p.W = W - 2 * bd;
    p.metrics = a->metrics;
    p.ntx = (p.W + TW - 1) / TW;
    p.nty = (p.H + TH - 1) / TH;
    for (int k = 0; k < 11; ++k) p.taps[k] = a->taps[k];
    for (int k = 0; k < 3; ++k) p.y_coef[k] = a->y_coef[k];
    p.ws = (double*)a->workspace;
    p.out = a->out;
    hipLaunchKernelGGL(metrics_tile_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(metrics_final_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
