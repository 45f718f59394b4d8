// The style half of the GAN stage's PerceptualLoss (gfx950): Gram matrices of the tapped VGG19 features, their L1 distance and its
// adjoint.                                                                                         losses/losses.py:147-187
//
//   grl_vgg_gram_fwd    G_b = F_b^T F_b / (C*h*w) for the nb images of a token matrix [nb*h*w, C]     losses.py:174-187 (_gram_mat)
//   grl_vgg_gram_loss   D = G[:B] - G[B:], loss (+)= coef * sum |D|                                    losses.py:160-168 (criterion l1)
//   grl_vgg_gram_bwd    d[rows of image b] += k * F_b * sign(D_b)                                      autograd through both
//
// Operands.  The features are fp32 and stay fp32: both contractions run on gfx950's f32-input MFMA (v_mfma_f32_32x32x2_f32), whose
// result is bit for bit a k-ordered fmaf chain -- one rounding per product and nothing else.  The forward cuts the token axis into
// chunks of at most 2048 tokens, so a chain is never longer than that; the chunks' fp32 partials are added in float64, in chunk
// order, by a second kernel.  (fp16 operands cost ~7e-5 on entries whose differences D average 1e-3; the hi + lo split of
// linear_split.hip would take three 16-bit MFMAs and a conversion pass per operand to reach what one f32 MFMA gives directly.
// Measured: 26 - 79 TFLOP/s of the f32 MFMA's 155 at 16 images of 256 x 256)
//
// Forward.  One WAVE per (image, token chunk, pair of 64-column blocks ti <= tj): two (four off the diagonal) dword loads per lane
// and k-pair straight from global memory -- lane l holds F[k + (l >> 5)][c0 + (l & 31)], which is at once the A operand of column
// block c0 (A[i][k] = F[k][c0 + i]) and the B operand of it -- and three (four) MFMAs on 32 x 32 accumulators.  Only tiles on or
// above the diagonal are computed; the reduction writes every sum to (i, j) and (j, i), so G is exactly symmetric.  A chunk lies
// inside one image (the image is a grid dimension): no K-tile straddles two images.  No atomics anywhere: the same bits every run.
// Diagonal waves also keep max_t |F[t, c]| per column; grl_vgg_gram_fwd adds these maxima over c into rowbound[b] >= max_t sum_c
// |F_b[t, c]|, which bounds every entry of F_b * Sigma for a Sigma of entries -1 / 0 / 1 (the operand scale of the backward pass).
//
// Backward.  One wave per (image, 32 tokens, NT * 32 output columns), NT = 4, 2 or 1 by the size of the grid.  Lane l reads four consecutive channels of token l & 31 with
// one 16-byte load, channels c0 + 4 * (l >> 5) .. + 3, and uses element s in MFMA s of that step: the k order inside a step is
// permuted the same way for both operands (B: row c0 + 4 * (l >> 5) + s of sign(D)).  sign(D) is formed from D in registers.
#include "common.h"
#include "grl_hip_internal.h"

namespace {

constexpr int VT = 256;          // threads per workgroup of the streaming kernels
constexpr int KC_MAX = 2048;     // longest fmaf chain of the forward (tokens per chunk)
constexpr int KC_MIN = 128;
constexpr int KU = 8;            // k-pairs per batch of loads in the forward
constexpr int WAVES_WANTED = 1024;   // one wave per SIMD of 256 CUs: chunks are halved until the grid has that many (or KC_MIN).  Measured at
                                     // 16 x 256 x 256 images: 512 / 1024 / 2048 / 4096 wanted -> 122 / 85 / 102 / 138 us at conv1_2 (more waves
                                     // write and re-read more partials than their overlap hides)

struct GramPlan {
    int nT, pairs, kc, splits;
};

GramPlan gram_plan(int nb, int hw, int C_) {
    GramPlan g;
    g.nT = C_ / 64;
    g.pairs = g.nT * (g.nT + 1) / 2;
    g.kc = KC_MAX;
    while (g.kc > KC_MIN && (int64_t)g.pairs * ((hw + g.kc - 1) / g.kc) * nb < WAVES_WANTED) g.kc >>= 1;
    g.splits = (hw + g.kc - 1) / g.kc;
    return g;
}

int64_t partial_floats(const GramPlan& g, int nb) { return (int64_t)nb * g.splits * g.pairs * 4096; }
int64_t colmax_floats(const GramPlan& g, int nb, int C_) { return (int64_t)nb * g.splits * C_; }

__device__ __forceinline__ f32x16 mfma_f32(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// row of register `reg` of a 32 x 32 accumulator in lane half h (the column is lane & 31)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__device__ __forceinline__ void store_tile(float* dst, const f32x16& a, int si, int sj, int r, int h) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) dst[(si * 32 + acc_row(reg, h)) * 64 + sj * 32 + r] = a[reg];
}

// `full` k-pairs of one pair of column blocks, KU at a time: the loads of batch n + 1 are issued before the MFMAs of batch n, so a wave
// keeps its MFMAs going while its next rows travel.  On the diagonal (DIAG) the x columns are the y columns and a10 is not formed.
template <bool DIAG>
__device__ __forceinline__ void gram_chunk(const float*& px, const float*& py, int64_t ldf, int full, f32x16& a00, f32x16& a01, f32x16& a10,
                                           f32x16& a11, float& m0, float& m1) {
    float x0[KU], x1[KU], y0[KU], y1[KU];
    auto load = [&](float* u0, float* u1, float* v0, float* v1) {
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            u0[u] = px[(int64_t)(2 * u) * ldf];
            u1[u] = px[(int64_t)(2 * u) * ldf + 32];
            if (!DIAG) {
                v0[u] = py[(int64_t)(2 * u) * ldf];
                v1[u] = py[(int64_t)(2 * u) * ldf + 32];
            }
        }
        px += (int64_t)(2 * KU) * ldf;
        if (!DIAG) py += (int64_t)(2 * KU) * ldf;
    };
    auto step = [&](float p0, float p1, float q0, float q1) {
        if (DIAG) {
            m0 = fmaxf(m0, fabsf(p0));
            m1 = fmaxf(m1, fabsf(p1));
            a00 = mfma_f32(p0, p0, a00);
            a01 = mfma_f32(p0, p1, a01);
            a11 = mfma_f32(p1, p1, a11);
        } else {
            a00 = mfma_f32(p0, q0, a00);
            a01 = mfma_f32(p0, q1, a01);
            a10 = mfma_f32(p1, q0, a10);
            a11 = mfma_f32(p1, q1, a11);
        }
    };
    const int batches = full / KU;
    if (batches > 0) load(x0, x1, y0, y1);
    for (int n = 0; n < batches; ++n) {
        float nx0[KU], nx1[KU], ny0[KU], ny1[KU];
        const bool more = n + 1 < batches;
        if (more) load(nx0, nx1, ny0, ny1);
#pragma unroll
        for (int u = 0; u < KU; ++u) step(x0[u], x1[u], y0[u], y1[u]);
        if (more) {
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                x0[u] = nx0[u], x1[u] = nx1[u];
                if (!DIAG) y0[u] = ny0[u], y1[u] = ny1[u];
            }
        }
    }
    for (int i = batches * KU; i < full; ++i) {
        const float p0 = px[0], p1 = px[32], q0 = DIAG ? 0.0f : py[0], q1 = DIAG ? 0.0f : py[32];
        px += 2 * ldf;
        if (!DIAG) py += 2 * ldf;
        step(p0, p1, q0, q1);
    }
}

__global__ __launch_bounds__(64) void gram_partial_kernel(const float* __restrict__ f, int64_t ldf, int hw, int C_, int nT, int kc,
                                                          float* __restrict__ part, float* __restrict__ colmax) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int pair = blockIdx.x, split = blockIdx.y, b = blockIdx.z, pairs = gridDim.x, splits = gridDim.y;
    int ti = 0, rem = pair;
    while (rem >= nT - ti) {
        rem -= nT - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const bool diag = ti == tj;
    const int k0 = split * kc, k1 = min(hw, k0 + kc);
    const float* px = f + ((int64_t)b * hw + k0 + h) * ldf + ti * 64 + r;
    const float* py = f + ((int64_t)b * hw + k0 + h) * ldf + tj * 64 + r;
    f32x16 a00 = {0}, a01 = {0}, a10 = {0}, a11 = {0};
    float m0 = 0.0f, m1 = 0.0f;
    const int full = (k1 - k0) >> 1;
    if (diag) {
        gram_chunk<true>(px, py, ldf, full, a00, a01, a10, a11, m0, m1);
    } else {
        gram_chunk<false>(px, py, ldf, full, a00, a01, a10, a11, m0, m1);
    }
    if ((k1 - k0) & 1) {                                   // the chunk's last token: the upper lane half has no row
        if (diag) py = px;                                 // (the diagonal loop advances px alone)
        const float x0 = h ? 0.0f : px[0], x1 = h ? 0.0f : px[32], y0 = h ? 0.0f : py[0], y1 = h ? 0.0f : py[32];
        m0 = fmaxf(m0, fabsf(x0));
        m1 = fmaxf(m1, fabsf(x1));
        a00 = mfma_f32(x0, y0, a00);
        a01 = mfma_f32(x0, y1, a01);
        a10 = mfma_f32(x1, y0, a10);
        a11 = mfma_f32(x1, y1, a11);
    }
    float* dst = part + (((int64_t)b * splits + split) * pairs + pair) * 4096;
    store_tile(dst, a00, 0, 0, r, h);
    store_tile(dst, a01, 0, 1, r, h);
    store_tile(dst, a11, 1, 1, r, h);
    if (!diag) store_tile(dst, a10, 1, 0, r, h);           // (on the diagonal that tile is the mirror of a01: never read)
    if (diag) {
        m0 = fmaxf(m0, __shfl_xor(m0, 32));
        m1 = fmaxf(m1, __shfl_xor(m1, 32));
        if (h == 0) {
            float* cm = colmax + ((int64_t)b * splits + split) * C_ + ti * 64 + r;
            cm[0] = m0;
            cm[32] = m1;
        }
    }
}

// G[b][i][j] = G[b][j][i] = (float)(inv * sum over the chunks, in chunk order, in float64); one thread per (b, i, j >= i)
__global__ __launch_bounds__(VT) void gram_reduce_kernel(const float* __restrict__ part, int nb, int C_, int nT, int pairs, int splits, double inv,
                                                         float* __restrict__ gram) {
    const int64_t idx = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (idx >= (int64_t)nb * C_ * C_) return;
    const int j = (int)(idx % C_), i = (int)((idx / C_) % C_), b = (int)(idx / ((int64_t)C_ * C_));
    if (i > j) return;
    const int ti = i >> 6, tj = j >> 6;
    const int pair = ti * nT - ti * (ti - 1) / 2 + (tj - ti);
    const float* src = part + ((int64_t)b * splits * pairs + pair) * 4096 + (i & 63) * 64 + (j & 63);
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += (double)src[(int64_t)k * pairs * 4096];
    const float g = (float)(s * inv);
    gram[((int64_t)b * C_ + i) * C_ + j] = g;
    gram[((int64_t)b * C_ + j) * C_ + i] = g;
}

// rowbound[b] = sum over c (fixed order) of max over the chunks of |F_b[t, c]|; one workgroup per image
__global__ __launch_bounds__(VT) void gram_bound_kernel(const float* __restrict__ colmax, int C_, int splits, float* __restrict__ rowbound) {
    __shared__ float acc[VT];
    const int b = blockIdx.x;
    float s = 0.0f;
    for (int c = threadIdx.x; c < C_; c += VT) {
        float m = 0.0f;
        for (int k = 0; k < splits; ++k) m = fmaxf(m, colmax[((int64_t)b * splits + k) * C_ + c]);
        s += m;
    }
    acc[threadIdx.x] = s;
    __syncthreads();
    for (int o = VT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) rowbound[b] = acc[0];
}

// D = G[:B] - G[B:], four entries per thread; the L1 sum as vgg_tap_fwd forms it: fp64 from the thread upward, one partial per workgroup
__global__ __launch_bounds__(VT) void gram_diff_kernel(const float* __restrict__ gram, int64_t n4, float* __restrict__ diff, double* __restrict__ partial) {
    __shared__ double wsum[VT / 64];
    const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
    double d = 0.0;
    if (i < n4) {
        const float4 a = ((const float4*)gram)[i], g = ((const float4*)gram)[n4 + i];
        const float4 v = float4{a.x - g.x, a.y - g.y, a.z - g.z, a.w - g.w};
        ((float4*)diff)[i] = v;
        d = ((double)fabsf(v.x) + (double)fabsf(v.y)) + ((double)fabsf(v.z) + (double)fabsf(v.w));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// one workgroup: loss (+)= coef * sum(partial), in a fixed order
__global__ __launch_bounds__(VT) void gram_finish_kernel(const double* __restrict__ partial, int n, float* loss, float* layer_sum, double coef, int accumulate) {
    __shared__ double acc[VT];
    double d = 0.0;
    for (int i = threadIdx.x; i < n; i += VT) d += partial[i];
    acc[threadIdx.x] = d;
    __syncthreads();
    for (int o = VT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float term = (float)(coef * acc[0]);
        loss[0] = accumulate ? loss[0] + term : term;
        if (layer_sum != nullptr) layer_sum[0] = (float)acc[0];
    }
}

template <int NT>
__global__ __launch_bounds__(64) void gram_bwd_kernel(const float* __restrict__ f, int64_t ldf, const float* __restrict__ diff, int hw, int C_, float k,
                                                      float* __restrict__ d, int64_t ldd) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int t0 = blockIdx.x * 32, j0 = blockIdx.y * (NT * 32), b = blockIdx.z;
    const int trow = min(t0 + r, hw - 1);                  // a tile past the image's last token re-reads that token; its rows are not stored
    const float* frow = f + ((int64_t)b * hw + trow) * ldf + 4 * h;
    const float* drow = diff + ((int64_t)b * C_ + 4 * h) * C_ + j0 + r;
    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x16{0};
    for (int c0 = 0; c0 < C_; c0 += 16) {                 // two steps of 8 channels: all their loads are issued before the first MFMA
        float av[2][4], sg[2][4][NT];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float4 a4 = *(const float4*)(frow + c0 + 8 * q);
            av[q][0] = a4.x, av[q][1] = a4.y, av[q][2] = a4.z, av[q][3] = a4.w;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int n = 0; n < NT; ++n) sg[q][s][n] = drow[(int64_t)(c0 + 8 * q + s) * C_ + n * 32];
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const float v = sg[q][s][n];
                    acc[n] = mfma_f32(av[q][s], (float)((v > 0.0f) - (v < 0.0f)), acc[n]);      // sign(0) = 0 (and sign(NaN) = 0, as in vgg_tap_bwd)
                }
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = t0 + acc_row(reg, h);
        if (row < hw) {
            float* out = d + ((int64_t)b * hw + row) * ldd + j0 + r;
#pragma unroll
            for (int n = 0; n < NT; ++n) out[n * 32] += k * acc[n][reg];
        }
    }
}

int check_common(const GrlVggGramArgs& p) {
    if (p.hw <= 0 || p.C <= 0) return GRL_ERR_BAD_ARG;
    if (p.C != 64 && p.C != 128 && p.C != 256 && p.C != 512) return GRL_ERR_UNSUPPORTED;
    return 0;
}

int check_features(const GrlVggGramArgs& p, int images) {
    if (p.f == nullptr || images <= 0 || images > 65535 || (p.ldf % 4) || p.ldf < p.C || ((uintptr_t)p.f % 16)) return GRL_ERR_BAD_ARG;
    if ((int64_t)images * p.hw > 0x7fffffffLL) return GRL_ERR_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int64_t grl_vgg_gram_workspace_bytes(int32_t nb, int32_t hw, int32_t C_) {
    if (nb <= 0 || hw <= 0) return GRL_ERR_BAD_ARG;
    if (C_ != 64 && C_ != 128 && C_ != 256 && C_ != 512) return GRL_ERR_UNSUPPORTED;
    const GramPlan g = gram_plan(nb, hw, C_);
    return (partial_floats(g, nb) + colmax_floats(g, nb, C_)) * (int64_t)sizeof(float);
}

extern "C" int grl_vgg_gram_loss_num_workgroups(int32_t B, int32_t C_) {
    if (B <= 0 || C_ <= 0 || (C_ % 4)) return GRL_ERR_BAD_ARG;
    const int64_t wgs = ((int64_t)B * C_ * C_ / 4 + VT - 1) / VT;
    return wgs > 0x7fffffffLL ? GRL_ERR_UNSUPPORTED : (int)wgs;
}

extern "C" int grl_vgg_gram_fwd(void* stream, const GrlVggGramArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const GrlVggGramArgs& p = *args;
    int e = check_common(p);
    if (e == 0) e = check_features(p, p.nb);
    if (e != 0) return e;
    if (p.gram == nullptr || p.ws == nullptr || ((uintptr_t)p.gram % 16) || ((uintptr_t)p.ws % 16)) return GRL_ERR_BAD_ARG;
    const GramPlan g = gram_plan(p.nb, p.hw, p.C);
    if (p.ws_bytes < (partial_floats(g, p.nb) + colmax_floats(g, p.nb, p.C)) * (int64_t)sizeof(float)) return GRL_ERR_BAD_ARG;
    if (g.splits > 65535) return GRL_ERR_UNSUPPORTED;
    float* part = (float*)p.ws;
    float* colmax = part + partial_floats(g, p.nb);
    hipLaunchKernelGGL(gram_partial_kernel, dim3(g.pairs, g.splits, p.nb), dim3(64), 0, (hipStream_t)stream, p.f, p.ldf, p.hw, p.C, g.nT, g.kc, part, colmax);
    GRL_CHECK_LAUNCH();
    const int64_t n = (int64_t)p.nb * p.C * p.C;
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)((n + VT - 1) / VT)), dim3(VT), 0, (hipStream_t)stream, (const float*)part, p.nb, p.C, g.nT,
                       g.pairs, g.splits, 1.0 / ((double)p.C * (double)p.hw), p.gram);
    GRL_CHECK_LAUNCH();
    if (p.rowbound != nullptr) {
        hipLaunchKernelGGL(gram_bound_kernel, dim3(p.nb), dim3(VT), 0, (hipStream_t)stream, (const float*)colmax, p.C, g.splits, p.rowbound);
        GRL_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int grl_vgg_gram_loss(void* stream, const GrlVggGramArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const GrlVggGramArgs& p = *args;
    const int e = check_common(p);
    if (e != 0) return e;
    if (p.B <= 0 || p.nb != 2 * p.B || p.gram == nullptr || p.diff == nullptr || p.partial == nullptr || p.loss == nullptr) return GRL_ERR_BAD_ARG;
    if (((uintptr_t)p.gram % 16) || ((uintptr_t)p.diff % 16) || ((uintptr_t)p.partial % 8)) return GRL_ERR_BAD_ARG;
    const int wgs = grl_vgg_gram_loss_num_workgroups(p.B, p.C);
    if (wgs < 0) return wgs;
    if (p.n_partial < wgs) return GRL_ERR_BAD_ARG;
    hipLaunchKernelGGL(gram_diff_kernel, dim3((unsigned)wgs), dim3(VT), 0, (hipStream_t)stream, (const float*)p.gram, (int64_t)p.B * p.C * p.C / 4, p.diff,
                       p.partial);
    GRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(gram_finish_kernel, dim3(1), dim3(VT), 0, (hipStream_t)stream, (const double*)p.partial, wgs, p.loss, p.layer_sum, (double)p.coef,
                       p.accumulate);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_vgg_gram_bwd(void* stream, const GrlVggGramArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const GrlVggGramArgs& p = *args;
    int e = check_common(p);
    if (e == 0) e = check_features(p, p.B);
    if (e != 0) return e;
    if (p.diff == nullptr || p.d == nullptr || ((uintptr_t)p.diff % 16) || ((uintptr_t)p.d % 4) || p.ldd < p.C) return GRL_ERR_BAD_ARG;
    const unsigned tiles = (unsigned)((p.hw + 31) / 32);
    // the widest wave (NT * 32 output columns, NT <= 4 and NT * 32 <= C) whose grid still has four waves per SIMD; else the narrowest
    int nt = p.C == 64 ? 2 : 4;
    while (nt > 1 && (int64_t)tiles * (p.C / (32 * nt)) * p.B < 4 * WAVES_WANTED) nt >>= 1;
#define GRL_GRAM_BWD(NT)                                                                                                                            \
    hipLaunchKernelGGL(gram_bwd_kernel<NT>, dim3(tiles, p.C / (32 * NT), p.B), dim3(64), 0, (hipStream_t)stream, p.f, p.ldf, (const float*)p.diff, \
                       p.hw, p.C, p.k, p.d, p.ldd)
    if (nt == 4) {
        GRL_GRAM_BWD(4);
    } else if (nt == 2) {
        GRL_GRAM_BWD(2);
    } else {
        GRL_GRAM_BWD(1);
    }
#undef GRL_GRAM_BWD
    GRL_CHECK_LAUNCH();
    return 0;
}
