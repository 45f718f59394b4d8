// Spectral normalisation of the U-Net discriminator's conv1 .. conv8 (gfx950): all layers of a discriminator in a fixed number
// of launches, bit-reproducible.
//
//   grl_spectral_norm_fwd : replaces, per layer, torch.nn.utils.spectral_norm's forward pre-hook
//       (torch/nn/utils/spectral_norm.py, compute_weight; applied to conv1 .. conv8 by models/aux_archs/discriminator.py:92-144):
//       t = W^T u, v' = t / max(|t|, 1e-12), s = W v', u' = s / max(|s|, 1e-12), sigma = u' . s, out = W / sigma.
//   grl_spectral_norm_bwd : the derivative of out = W / sigma(W) with u', v' held constant (what autograd makes of it):
//       dW = G / sigma - (<G, W> / sigma^2) u' v'^T.
//
// Design.  Eight layers of 0.04 .. 2.1 M weights: 24 MB read twice and written once, against about a hundred launches of the torch
// chain.  A launch covers every layer: a workgroup finds its (layer, block) by walking the layer table in the kernel arguments.
//   launch 1  W^T u: a thread per column j walks down a chunk of 64 rows (coalesced along K); the chunks' partial sums go to the
//             workspace, tpart[chunk][j].  Columns x row chunks spread a layer over workgroups (512 x 4096: 128 of them).
//   launch 2  W v': a workgroup owns 8 rows.  It first sums the partials into t_j and |t|^2 (every workgroup of a layer does the
//             same arithmetic in the same order, so all of them hold the same norm), then walks K in tiles of 1024: v'_j into LDS,
//             each wave two rows against the tile, lanes along K.  The first workgroup of a layer writes v'.
//   launch 3  every workgroup sums |s|^2 and u' . s over the layer's s (again the same order everywhere), then scales its chunk
//             of W; the first one of a layer writes u' and sigma.
// Sums: a thread's own terms in index order, a wave's 64 by a shuffle tree, the four waves' in wave order, chunks in chunk order.
// Nothing depends on which workgroup finishes first: no atomics.  <G, W> (up to 2.1 M signed terms) is summed in double, per
// 4096-element chunk and then over the chunks, as grl_grad_sqnorm does.
#include "common.h"
#include <stdint.h>
#include "grl_hip_internal.h"

namespace {

constexpr int SN_ROWS1 = 64;      // rows per chunk of launch 1
constexpr int SN_ROWS2 = 8;       // rows per workgroup of launch 2
constexpr int SN_RPW = SN_ROWS2 / 4;   // ... per wave
constexpr int SN_TILE = 1024;     // columns per LDS tile of launch 2
constexpr int SN_SCALE = 8192;    // elements per workgroup of launch 3
constexpr int SN_CHUNK = 4096;    // elements per workgroup of the backward launches

__host__ __device__ inline int sn_cdiv(int64_t a, int b) { return (int)((a + b - 1) / b); }
__host__ __device__ inline int sn_nrc(int cout) { return sn_cdiv(cout, SN_ROWS1); }
// forward workspace of a layer, in floats: tpart [nrc][K], then s [Cout]
__host__ __device__ inline int64_t sn_ws_floats(int cout, int k) { return (int64_t)sn_nrc(cout) * k + cout; }

__host__ __device__ inline int sn_blocks1(int cout, int k) { return sn_cdiv(k, 256) * sn_nrc(cout); }
__host__ __device__ inline int sn_blocks2(int cout, int k) { return sn_cdiv(cout, SN_ROWS2); }
__host__ __device__ inline int sn_blocks3(int cout, int k) { return sn_cdiv((int64_t)cout * k, SN_SCALE); }
__host__ __device__ inline int sn_blocks_bwd(int cout, int k) { return sn_cdiv((int64_t)cout * k, SN_CHUNK); }

struct SnWhere {
    int layer, block;       // block within the layer
    int64_t ws_off;         // forward: the layer's first workspace float; backward: its first partial
};

// (layer, block) of workgroup `bid`; the grid holds exactly the sum of blocks_of over the layers
template <typename F>
__device__ __forceinline__ SnWhere sn_where(const GrlSpectralNormArgs& p, int bid, bool bwd, F blocks_of) {
    SnWhere w = {0, bid, 0};
    for (; w.layer < p.n_layers - 1; ++w.layer) {
        const int nb = blocks_of(p.cout[w.layer], p.k[w.layer]);
        if (w.block < nb) break;
        w.block -= nb;
        w.ws_off += bwd ? (int64_t)nb : sn_ws_floats(p.cout[w.layer], p.k[w.layer]);
    }
    return w;
}

// Sum of 256 values, one per thread, in a fixed order (csrc/grad.hip: block_sum_256).  `lds4` must not be in use by an earlier sum.
template <typename T>
__device__ __forceinline__ T sn_block_sum(T x, T* lds4) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d, 64);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

// ---- launch 1: partial sums of W^T u ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_wtu_kernel(GrlSpectralNormArgs p) {
    const SnWhere at = sn_where(p, blockIdx.x, false, sn_blocks1);
    const int K = p.k[at.layer], Cout = p.cout[at.layer];
    const int ncb = sn_cdiv(K, 256);
    const int cb = at.block % ncb, rc = at.block / ncb;
    const int j = cb * 256 + threadIdx.x;
    if (j >= K || rc >= sn_nrc(Cout)) return;
    const float* W = p.w[at.layer];
    const float* u = p.u[at.layer];
    const int i0 = rc * SN_ROWS1, i1 = min(Cout, i0 + SN_ROWS1);
    float acc = 0.f;
#pragma unroll 8
    for (int i = i0; i < i1; ++i) acc = fmaf(W[(int64_t)i * K + j], u[i], acc);
    ((float*)p.ws)[at.ws_off + (int64_t)rc * K + j] = acc;
}

// ---- launch 2: v' and s = W v' -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_wv_kernel(GrlSpectralNormArgs p) {
    __shared__ float tile[SN_TILE];
    __shared__ float red[4];
    const SnWhere at = sn_where(p, blockIdx.x, false, sn_blocks2);
    const int l = at.layer;
    const int K = p.k[l], Cout = p.cout[l], nrc = sn_nrc(Cout);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* W = p.w[l];
    const float* tpart = (const float*)p.ws + at.ws_off;
    float* s = (float*)p.ws + at.ws_off + (int64_t)nrc * K;
    float* v = p.v[l];
    float* v_keep = p.v_keep[l];
    const bool first = at.block == 0;

    auto t_of = [&](int j) {     // chunks in chunk order: the same value wherever it is evaluated
        float t = tpart[j];
#pragma unroll 4
        for (int c = 1; c < nrc; ++c) t += tpart[(int64_t)c * K + j];       // (the loads do not wait for the adds)
        return t;
    };
    float dn = 1.f;
    if (p.advance) {
        float sq = 0.f;
#pragma unroll 2
        for (int j = tid; j < K; j += 256) {
            const float t = t_of(j);
            sq = fmaf(t, t, sq);
        }
        dn = fmaxf(sqrtf(sn_block_sum(sq, red)), 1e-12f);
    }
    const int r0 = at.block * SN_ROWS2 + wave * SN_RPW;
    float acc[SN_RPW] = {};
    for (int j0 = 0; j0 < K; j0 += SN_TILE) {
        const int n = min(SN_TILE, K - j0);
        __syncthreads();          // the previous tile's readers are done
        for (int jj = tid; jj < n; jj += 256) {
            const int j = j0 + jj;
            const float x = p.advance ? t_of(j) / dn : v[j];
            if (first) {
                if (p.advance) v[j] = x;
                if (v_keep != nullptr) v_keep[j] = x;
            }
            tile[jj] = x;
        }
        __syncthreads();
#pragma unroll 4
        for (int jj = lane; jj < n; jj += 64) {
            const float x = tile[jj];
#pragma unroll
            for (int r = 0; r < SN_RPW; ++r)
                if (r0 + r < Cout) acc[r] = fmaf(W[(int64_t)(r0 + r) * K + j0 + jj], x, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < SN_RPW; ++r) {
        float a = acc[r];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) a += __shfl_down(a, d, 64);
        if (lane == 0 && r0 + r < Cout) s[r0 + r] = a;
    }
}

// ---- launch 3: u', sigma, out = W / sigma --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_scale_kernel(GrlSpectralNormArgs p) {
    __shared__ float red0[4], red1[4];
    const SnWhere at = sn_where(p, blockIdx.x, false, sn_blocks3);
    const int l = at.layer;
    const int K = p.k[l], Cout = p.cout[l];
    const int tid = threadIdx.x;
    const float* s = (const float*)p.ws + at.ws_off + (int64_t)sn_nrc(Cout) * K;
    float* u = p.u[l];
    float* u_keep = p.u_keep[l];
    const bool first = at.block == 0;
    float sigma;
    if (p.advance) {
        float sq = 0.f;
        for (int i = tid; i < Cout; i += 256) sq = fmaf(s[i], s[i], sq);
        const float dn = fmaxf(sqrtf(sn_block_sum(sq, red0)), 1e-12f);
        float d = 0.f;
        for (int i = tid; i < Cout; i += 256) {
            const float un = s[i] / dn;
            d = fmaf(un, s[i], d);
            if (first) {
                u[i] = un;
                if (u_keep != nullptr) u_keep[i] = un;
            }
        }
        sigma = sn_block_sum(d, red1);
    } else {
        float d = 0.f;
        for (int i = tid; i < Cout; i += 256) {
            d = fmaf(u[i], s[i], d);
            if (first && u_keep != nullptr) u_keep[i] = u[i];
        }
        sigma = sn_block_sum(d, red0);
    }
    if (first && tid == 0 && p.sigma[l] != nullptr) *p.sigma[l] = sigma;

    const float* W = p.w[l];
    float* out = p.out[l];
    const int64_t total = (int64_t)Cout * K, e0 = (int64_t)at.block * SN_SCALE;
    const int n = (int)min((int64_t)SN_SCALE, total - e0);
    int done = 0;
    if ((((uintptr_t)W | (uintptr_t)out) & 15) == 0) {      // (e0 is a multiple of 4: 16-byte pieces when both tensors allow)
        const float4* W4 = (const float4*)(W + e0);
        float4* out4 = (float4*)(out + e0);
        for (int q = tid; q < n / 4; q += 256) {
            const float4 a = W4[q];
            out4[q] = float4{a.x / sigma, a.y / sigma, a.z / sigma, a.w / sigma};
        }
        done = n / 4 * 4;
    }
    for (int e = done + tid; e < n; e += 256) out[e0 + e] = W[e0 + e] / sigma;
}

// ---- backward 1: per-chunk partials of <G, W> in double ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_dot_kernel(GrlSpectralNormArgs p) {
    __shared__ double red[4];
    const SnWhere at = sn_where(p, blockIdx.x, true, sn_blocks_bwd);
    const int l = at.layer;
    const float* W = p.w[l];
    const float* G = p.g[l];
    const int64_t total = (int64_t)p.cout[l] * p.k[l], e0 = (int64_t)at.block * SN_CHUNK;
    const int64_t end = min(total, e0 + SN_CHUNK);
    double acc = 0.0;
#pragma unroll 4
    for (int64_t e = e0 + threadIdx.x; e < end; e += 256) acc += (double)G[e] * (double)W[e];
    const double d = sn_block_sum(acc, red);
    if (threadIdx.x == 0) ((double*)p.ws)[at.ws_off + at.block] = d;
}

// ---- backward 2: dW = G / sigma - (<G, W> / sigma^2) u' v'^T -------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_bwd_kernel(GrlSpectralNormArgs p) {
    __shared__ double red[4];
    const SnWhere at = sn_where(p, blockIdx.x, true, sn_blocks_bwd);
    const int l = at.layer;
    const int K = p.k[l], Cout = p.cout[l];
    const int nb = sn_blocks_bwd(Cout, K);
    const double* part = (const double*)p.ws + at.ws_off;
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
    const double dot = sn_block_sum(acc, red);
    const float sigma = *p.sigma[l];
    const float coef = (float)(dot / ((double)sigma * (double)sigma));
    const float* G = p.g[l];
    const float* u = p.u[l];
    const float* v = p.v[l];
    float* dW = p.out[l];
    const unsigned total = (unsigned)Cout * (unsigned)K, e0 = (unsigned)at.block * SN_CHUNK;     // (Cout * K < 2^31: checked on the host)
    const unsigned end = min(total, e0 + SN_CHUNK);
#pragma unroll 4
    for (unsigned e = e0 + threadIdx.x; e < end; e += 256) {
        const unsigned i = e / (unsigned)K, j = e - i * (unsigned)K;
        dW[e] = G[e] / sigma - coef * u[i] * v[j];
    }
}

inline bool sn_aligned4(const void* q) { return ((uintptr_t)q & 3) == 0; }

// validates the table; returns 0 and the three grids / the workspace need, or an error
int sn_check(const GrlSpectralNormArgs* a, bool bwd, int64_t grid[3], int64_t* need_bytes) {
    if (a == nullptr || a->n_layers <= 0 || a->n_layers > GRL_SN_MAX_LAYERS || a->ws == nullptr) return GRL_ERR_BAD_ARG;
    if (a->advance != 0 && a->advance != 1) return GRL_ERR_BAD_ARG;
    grid[0] = grid[1] = grid[2] = 0;
    int64_t need = 0;
    for (int l = 0; l < a->n_layers; ++l) {
        if (a->cout[l] <= 0 || a->k[l] <= 0) return GRL_ERR_BAD_ARG;
        if (!a->w[l] || !a->u[l] || !a->v[l] || !a->out[l]) return GRL_ERR_BAD_ARG;
        if (bwd && (!a->g[l] || !a->sigma[l])) return GRL_ERR_BAD_ARG;
        if (!sn_aligned4(a->w[l]) || !sn_aligned4(a->u[l]) || !sn_aligned4(a->v[l]) || !sn_aligned4(a->out[l]) || !sn_aligned4(a->g[l]) ||
            !sn_aligned4(a->sigma[l]) || !sn_aligned4(a->u_keep[l]) || !sn_aligned4(a->v_keep[l]))
            return GRL_ERR_BAD_ARG;
        if ((int64_t)a->cout[l] * a->k[l] >= ((int64_t)1 << 31)) return GRL_ERR_UNSUPPORTED;
        if (bwd) {
            grid[0] += sn_blocks_bwd(a->cout[l], a->k[l]);
            need += (int64_t)sn_blocks_bwd(a->cout[l], a->k[l]) * 8;
        } else {
            grid[0] += sn_blocks1(a->cout[l], a->k[l]);
            grid[1] += sn_blocks2(a->cout[l], a->k[l]);
            grid[2] += sn_blocks3(a->cout[l], a->k[l]);
            need += sn_ws_floats(a->cout[l], a->k[l]) * 4;
        }
    }
    if (((uintptr_t)a->ws & 7) != 0 || a->ws_bytes < need) return GRL_ERR_BAD_ARG;
    for (int i = 0; i < 3; ++i)
        if (grid[i] >= ((int64_t)1 << 31)) return GRL_ERR_UNSUPPORTED;
    *need_bytes = need;
    return 0;
}

}  // namespace

extern "C" int grl_spectral_norm_fwd(void* stream, const GrlSpectralNormArgs* args) {
    int64_t grid[3], need;
    const int err = sn_check(args, false, grid, &need);
    if (err != 0) return err;
    hipStream_t s = (hipStream_t)stream;
    if (args->advance) {
        hipLaunchKernelGGL(sn_wtu_kernel, dim3((unsigned)grid[0]), dim3(256), 0, s, *args);
        GRL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sn_wv_kernel, dim3((unsigned)grid[1]), dim3(256), 0, s, *args);
    GRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(sn_scale_kernel, dim3((unsigned)grid[2]), dim3(256), 0, s, *args);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_spectral_norm_bwd(void* stream, const GrlSpectralNormArgs* args) {
    int64_t grid[3], need;
    const int err = sn_check(args, true, grid, &need);
    if (err != 0) return err;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sn_dot_kernel, dim3((unsigned)grid[0]), dim3(256), 0, s, *args);
    GRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(sn_bwd_kernel, dim3((unsigned)grid[0]), dim3(256), 0, s, *args);
    GRL_CHECK_LAUNCH();
    return 0;
}
