// NIQE's feature matrix (include/grl_hip.h, grl_image_niqe_features): the reference's niqe() (utils/metrics/niqe.py:400-473) up to
// `distparam`, for a (B, C, H, W) fp32 batch read in place through its strides.  Five launches on the caller's stream:
//
//   1. niqe_y_kernel        tensor_round of the image (engines/base_gan.py:149-168), the plane NIQE scores, cropped to whole 96 x 96
//                           blocks, as the integer level k in fp32.
//                           For C = 3 the reference calls to_y_channel, which assumes BGR, on a CHW **RGB** array (niqe.py:143-156,
//                           573): the plane is 24.966 R + 128.553 G + 65.481 B (+ 16), red and blue swapped against rgb2ycbcr.  That is
//                           what the published NIQE numbers were computed with, so luma_bgr() below reproduces it, rounding for rounding.
//   2. niqe_sums_kernel<96> scale 1: one workgroup per block
//   3. grl_imresize         the half-scale plane imresize(img / 255, 0.5) * 255 (niqe.py:469-471), taken as imresize(img, 0.5): the
//                           resampling is linear and the levels are exact in fp32, so the two differ by an fp64 rounding.  By
//                           the caller's tap tables (csrc/imresize.hip; the same resampler as everywhere),
//                           stored as the fp64 sums (out_f64): rounding it to fp32 moves MSCN by 1e-5 and, where r_gam is flat
//                           (alpha above ~6), the nearest-grid-point alpha with it
//   4. niqe_sums_kernel<48> scale 2 on that plane
//   5. niqe_final_kernel    sums -> the 18 AGGD features per block and scale (niqe.py:341-397)
//
// niqe_sums_kernel: a workgroup stages its block with the 3-pixel halo of the 7 x 7 window as fp32 (edge replicate at the borders
// of the cropped plane, real neighbours across block borders: scipy's mode="nearest" on the whole image), forms
// mu = sum w v, sigma = sqrt|sum w v^2 - mu^2| and MSCN = (v - mu) / (sigma + 1) in fp64, and sums, for the block and for its
// products with the four np.roll-ed copies (shifts (0,1), (1,0), (1,1), (1,-1), circular INSIDE the block, niqe.py:390-393), what
// estimate_aggd_param needs: count and sum of squares of the negative and of the positive samples, sum |x|, sum x^2.
//
// Flat windows.  mu and the variance are formed from the differences to the window's centre sample (mu = v + sum w (x - v),
// var = sum w (x - v)^2 - (sum w (x - v))^2), which is the same number to 1e-16 |v| while the weights sum to one, and exactly
// v and 0 where the window is flat.  The reference gets exact zeros there too, by another route (scipy returns mu in the image's
// fp32, which rounds 254.99999999999997 to 255), and so reports nan features for blocks inside a saturated or black region;
// sum w x - v in plain float64 would instead leave a constant 3e-14 of one sign and a finite beta_r in such blocks.
//
// LDS byte map for BS = 96 (static, 61 776 of the 65 536 bytes a workgroup may take):
//   in   float  [102][102]   41 616   the block and its halo (BS = 48: double [54][54], 23 328)
//   ms   double [25][96]     19 200   MSCN of one strip of 24 rows, preceded by the row above it (row -1 is row 95: the roll)
//   red  double [4][30]         960   the four waves' sums
// A whole 96 x 96 MSCN tile in fp64 is 72 KB and does not fit next to anything; fp32 MSCN would fit (36 KB) but moves the moments by
// 1e-7 and with them the nearest-grid-point alpha.  So the block goes through in 4 strips (2 for BS = 48); each strip recomputes the
// one MSCN row above it (25 rows of work for 24).  The shifted copies never exist: a product reads its two factors from `ms`.
//
// Order of every sum is fixed (a thread's pixels ascending, a butterfly over the wave, waves 0..3): two calls are bitwise equal, and
// a strided view gives the bits of its contiguous copy because everything after launch 1 reads the workspace planes.
#include "common.h"

namespace {

constexpr int HALO = 3, STRIP = 24, NT = 256;
constexpr int NQ = 5, NS = 6, NSUM = NQ * NS;       // quantities (block, 4 products) x sums (n-, ss-, n+, ss+, sum|x|, sum x^2)
constexpr int NFEAT = 18, BLOCK = 96;

__device__ __forceinline__ uint32_t round8(float v) {
    return (uint32_t)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f);   // tensor_round: clamp, round(x 255)
}

// what calculate_niqe makes of a rounded sample k / 255: p * 255 (fp32), to_y_channel's / 255 (fp32)
__device__ __forceinline__ float ref_unit(uint32_t k) { return (((float)k / 255.f) * 255.f) / 255.f; }

// niqe.py:75-111,143-156 on a CHW RGB array: np.dot(fp32 pixel, [24.966, 128.553, 65.481]) in float64 in that order, + 16, / 255,
// cast to fp32, x 255 in fp32, round half to even.  No contraction: every product and sum is rounded as numpy rounds it.
__device__ __forceinline__ uint32_t luma_bgr(uint32_t r, uint32_t g, uint32_t b) {
    const double ur = (double)ref_unit(r), ug = (double)ref_unit(g), ub = (double)ref_unit(b);
    double y = __dadd_rn(__dadd_rn(__dmul_rn(ur, 24.966), __dmul_rn(ug, 128.553)), __dmul_rn(ub, 65.481));
    y = __dadd_rn(y, 16.0);
    const float f = (float)__ddiv_rn(y, 255.0);
    return (uint32_t)rintf(__fmul_rn(f, 255.f));
}

struct YParams {
    const float* img;
    int64_t st[4];
    int32_t C, Hc, Wc;
    float* yk;      // (B, Hc, Wc) integer levels
};

__global__ __launch_bounds__(NT) void niqe_y_kernel(YParams p) {
    const int x = blockIdx.x * NT + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= p.Wc) return;
    const float* src = p.img + b * p.st[0] + y * p.st[2] + x * p.st[3];
    uint32_t k = round8(src[0]);
    if (p.C == 3) k = luma_bgr(k, round8(src[p.st[1]]), round8(src[2 * p.st[1]]));
    const int64_t o = ((int64_t)b * p.Hc + y) * p.Wc + x;
    p.yk[o] = (float)k;
}

template <typename T>
struct SParams {
    const T* plane;         // (B, h, w) contiguous: fp32 levels at scale 1, the fp64 half-scale plane at scale 2
    int32_t h, w, nbh, nbw, scale_idx;
    double win[49];
    double* sums;           // [B][nbw * nbh][2][NSUM]
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

template <int BS, typename T>
__global__ __launch_bounds__(NT) void niqe_sums_kernel(SParams<T> p) {
    constexpr int LW = BS + 2 * HALO;
    __shared__ T in[LW * LW];
    __shared__ double ms[(STRIP + 1) * BS];
    __shared__ double red[4][NSUM];

    const int nblk = p.nbh * p.nbw;
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int bw = blk / p.nbh, bh = blk - bw * p.nbh;             // columns outer, rows inner (niqe.py:458-465)
    const int y0 = bh * BS - HALO, x0 = bw * BS - HALO;
    const T* src = p.plane + (int64_t)b * p.h * p.w;
    const int tid = threadIdx.x;

    for (int i = tid; i < LW * LW; i += NT) {
        const int r = i / LW, c = i - r * LW;
        const int gy = min(max(y0 + r, 0), p.h - 1), gx = min(max(x0 + c, 0), p.w - 1);
        in[i] = src[(int64_t)gy * p.w + gx];
    }

    double acc[NSUM];
#pragma unroll
    for (int s = 0; s < NSUM; ++s) acc[s] = 0.0;

    for (int s0 = 0; s0 < BS; s0 += STRIP) {
        __syncthreads();                                           // `in` is staged / the previous strip's readers are done
        for (int i = tid; i < (STRIP + 1) * BS; i += NT) {
            const int rr = i / BS, c = i - rr * BS;
            int row = s0 - 1 + rr;
            if (row < 0) row += BS;
            const T* t = in + row * LW + c;                    // top-left of the 7 x 7 window of pixel (row, c)
            const double ctr = (double)t[HALO * LW + HALO];
            double s1 = 0.0, s2 = 0.0;                             // moments of (v - centre): see the note on flat windows
#pragma unroll
            for (int a = 0; a < 7; ++a)
#pragma unroll
                for (int e = 0; e < 7; ++e) {
                    const double d = (double)t[a * LW + e] - ctr, w = p.win[a * 7 + e];
                    s1 += w * d;
                    s2 += w * (d * d);
                }
            const double sigma = sqrt(fabs(s2 - s1 * s1));
            ms[i] = -s1 / (sigma + 1.0);                           // (v - mu) / (sigma + 1), mu = v + s1
        }
        __syncthreads();
        for (int i = tid; i < STRIP * BS; i += NT) {
            const int rr = i / BS, c = i - rr * BS;
            const int cl = c == 0 ? BS - 1 : c - 1, cr = c == BS - 1 ? 0 : c + 1;
            const double* cur = ms + (rr + 1) * BS;
            const double* up = ms + rr * BS;
            const double x = cur[c];
            const double q[NQ] = {x, x * cur[cl], x * up[c], x * up[cl], x * up[cr]};
#pragma unroll
            for (int k = 0; k < NQ; ++k) {
                const double v = q[k], vv = v * v;
                acc[k * NS + 0] += v < 0.0 ? 1.0 : 0.0;
                acc[k * NS + 1] += v < 0.0 ? vv : 0.0;
                acc[k * NS + 2] += v > 0.0 ? 1.0 : 0.0;
                acc[k * NS + 3] += v > 0.0 ? vv : 0.0;
                acc[k * NS + 4] += fabs(v);
                acc[k * NS + 5] += vv;
            }
        }
    }

    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int s = 0; s < NSUM; ++s) {
        const double r = wave_sum(acc[s]);
        if (lane == 0) red[wv][s] = r;
    }
    __syncthreads();
    if (tid < NSUM)
        p.sums[((int64_t)blockIdx.x * 2 + p.scale_idx) * NSUM + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

struct FParams {
    const double* sums;
    const double* grid;     // [5][ngrid]: gam, r_gam, gamma(1 / gam), gamma(2 / gam), gamma(3 / gam)
    int32_t ngrid;
    double* out;            // [B * blocks][2 * NFEAT]
};

// estimate_aggd_param / compute_feature (niqe.py:341-397): one workgroup per (block, scale), wave q fits quantity q.  A block
// without negative or without positive samples gives 0 / 0 = nan standard deviations, as the reference; its nan rhatnorm makes every
// distance nan, np.argmin then answers 0, and so does the search here (no `d < best` holds), so alpha is gam[0] and the betas nan.
__global__ __launch_bounds__(NQ * 64) void niqe_final_kernel(FParams p) {
#pragma clang fp contract(off)
    const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int scale_idx = blockIdx.x & 1;
    const double* s = p.sums + (int64_t)blockIdx.x * NSUM + q * NS;
    const double n = scale_idx ? (BLOCK / 2) * (BLOCK / 2) : BLOCK * BLOCK;
    const double left_std = sqrt(s[1] / s[0]), right_std = sqrt(s[3] / s[2]);
    const double gammahat = left_std / right_std;
    const double mabs = s[4] / n;
    const double rhat = (mabs * mabs) / (s[5] / n);
    const double g2 = gammahat * gammahat;
    const double rhatnorm = (rhat * (g2 * gammahat + 1.0) * (gammahat + 1.0)) / ((g2 + 1.0) * (g2 + 1.0));

    const double* r_gam = p.grid + p.ngrid;
    double best = __builtin_inf();
    int idx = 0;
    for (int k = lane; k < p.ngrid; k += 64) {
        const double e = r_gam[k] - rhatnorm, d = e * e;
        if (d < best) { best = d; idx = k; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {                            // the first minimum, as np.argmin
        const double ob = __shfl_xor(best, m);
        const int oi = __shfl_xor(idx, m);
        if (ob < best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if (lane != 0) return;
    const double alpha = p.grid[idx], ga1 = p.grid[2 * p.ngrid + idx], ga2 = p.grid[3 * p.ngrid + idx], ga3 = p.grid[4 * p.ngrid + idx];
    const double ratio = sqrt(ga1 / ga3);
    const double beta_l = left_std * ratio, beta_r = right_std * ratio;
    double* o = p.out + (int64_t)(blockIdx.x >> 1) * (2 * NFEAT) + scale_idx * NFEAT;
    if (q == 0) {
        o[0] = alpha;
        o[1] = (beta_l + beta_r) / 2.0;
    } else {
        o += 2 + 4 * (q - 1);
        o[0] = alpha;
        o[1] = (beta_r - beta_l) * (ga2 / ga1);                    // Eq. 8
        o[2] = beta_l;
        o[3] = beta_r;
    }
}

}  // namespace

extern "C" int64_t grl_image_niqe_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H < BLOCK || W < BLOCK) return 0;
    const int64_t nbh = H / BLOCK, nbw = W / BLOCK, px = nbh * nbw * BLOCK * BLOCK;
    return (int64_t)B * ((nbh * nbw * 2 * NSUM + px / 4) * (int64_t)sizeof(double) + px * (int64_t)sizeof(float));
}

extern "C" int grl_image_niqe_features(void* stream, const GrlNiqeArgs* a) {
    if (!a || !a->img || !a->grid || !a->wh || !a->ih || !a->ww || !a->iw || !a->workspace || !a->out) return GRL_ERR_BAD_ARG;
    const int32_t B = a->shape[0], C = a->shape[1], H = a->shape[2], W = a->shape[3];
    if (B <= 0 || B > 65535 || (C != 1 && C != 3) || H < BLOCK || W < BLOCK) return GRL_ERR_BAD_ARG;   // fewer than one block per side
    for (int d = 0; d < 4; ++d)
        if (a->stride[d] < 0) return GRL_ERR_BAD_ARG;
    if (a->ngrid < 1 || a->taps_h < 1 || a->taps_w < 1) return GRL_ERR_BAD_ARG;
    if ((uint64_t)a->workspace % 16 || (uint64_t)a->grid % 8 || (uint64_t)a->out % 8) return GRL_ERR_BAD_ARG;
    const int32_t nbh = H / BLOCK, nbw = W / BLOCK, Hc = nbh * BLOCK, Wc = nbw * BLOCK;
    const int64_t nblk = (int64_t)nbh * nbw, grid = (int64_t)B * nblk;
    if (Hc > 65535 || grid > 0x3fffffff || a->workspace_bytes < grl_image_niqe_workspace_bytes(B, H, W)) return GRL_ERR_BAD_ARG;

    double* sums = (double*)a->workspace;
    double* half = sums + grid * 2 * NSUM;
    float* yk = (float*)(half + (int64_t)B * (Hc / 2) * (Wc / 2));
    hipStream_t st = (hipStream_t)stream;

    YParams y;
    y.img = a->img;
    for (int d = 0; d < 4; ++d) y.st[d] = a->stride[d];
    y.C = C; y.Hc = Hc; y.Wc = Wc; y.yk = yk;
    hipLaunchKernelGGL(niqe_y_kernel, dim3((unsigned)((Wc + NT - 1) / NT), (unsigned)Hc, (unsigned)B), dim3(NT), 0, st, y);
    GRL_CHECK_LAUNCH();

    SParams<float> s;
    s.plane = yk; s.h = Hc; s.w = Wc; s.nbh = nbh; s.nbw = nbw; s.scale_idx = 0; s.sums = sums;
    for (int k = 0; k < 49; ++k) s.win[k] = a->window[k];
    hipLaunchKernelGGL((niqe_sums_kernel<BLOCK, float>), dim3((unsigned)grid), dim3(NT), 0, st, s);
    GRL_CHECK_LAUNCH();

    GrlResizeArgs r;
    r.src = yk;
    r.stride[0] = (int64_t)Hc * Wc; r.stride[1] = (int64_t)Hc * Wc; r.stride[2] = Wc; r.stride[3] = 1;
    r.N = B; r.C = 1; r.H = Hc; r.W = Wc; r.out_h = Hc / 2; r.out_w = Wc / 2;
    r.taps_h = a->taps_h; r.taps_w = a->taps_w;
    r.wh = a->wh; r.ih = a->ih; r.ww = a->ww; r.iw = a->iw;
    r.out = (float*)half; r.quantize = 0; r.out_f64 = 1;
    const int rc = grl_imresize(stream, &r);
    if (rc != 0) return rc;

    SParams<double> s2;
    s2.plane = half; s2.h = Hc / 2; s2.w = Wc / 2; s2.nbh = nbh; s2.nbw = nbw; s2.scale_idx = 1; s2.sums = sums;
    for (int k = 0; k < 49; ++k) s2.win[k] = a->window[k];
    hipLaunchKernelGGL((niqe_sums_kernel<BLOCK / 2, double>), dim3((unsigned)grid), dim3(NT), 0, st, s2);
    GRL_CHECK_LAUNCH();

    FParams f;
    f.sums = sums; f.grid = a->grid; f.ngrid = a->ngrid; f.out = a->out;
    hipLaunchKernelGGL(niqe_final_kernel, dim3((unsigned)(grid * 2)), dim3(NQ * 64), 0, st, f);
    GRL_CHECK_LAUNCH();
    return 0;
}
