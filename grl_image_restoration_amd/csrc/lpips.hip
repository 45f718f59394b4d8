// LPIPS (net = "vgg", package version 0.1) between the 3x3 convolutions of its VGG16 trunk (gfx950):
//
//   grl_lpips_prep   x <- 2x - 1, then the scaling layer (x - shift) / scale with the float32 shift / scale buffers
//   grl_lpips_tap    one tapped layer: ReLU, the per-pixel unit normalisation across channels f / (sqrt(sum_c f_c^2) + 1e-10) of both
//                    images, sum_c w_c (f^0_c - f^1_c)^2, the spatial mean per image added into out[b] -- and the 2 x 2 max pool of
//                    the ReLU of both halves as the 16-bit operand of the next block
//
// The tap streams the fp32 pre-activation [2B*H*W, C] (restored rows first, then the target's) once.  A GROUP of G = min(64, C/4)
// lanes owns one 2 x 2 cell of pixels -- the pool window -- of BOTH images: lane l holds the float4 quads l, l + G (C = 512: two
// quads; else one) of the four pixels of the two images in registers, at most 16 quads.  From those registers come the two squared
// norms of a pixel (fp32 in the lane, xor-shuffles across the group), the weighted term evaluated AS WRITTEN -- normalise, subtract,
// square: a good restoration makes the two unit vectors nearly equal, and the expanded form would cancel -- and the NaN-keeping pool
// maximum.  Cells cover ceil(H/2) x ceil(W/2): the pixels MaxPool2d's floor drops take part in the mean and get no pool output.
// Sums: fp32 inside a pixel (<= 8 terms in a lane, 6 shuffle levels), fp64 from the pixel on: per group over its cells, per workgroup
// over its groups in a fixed order, one fp64 partial per (workgroup, image) -- blockIdx.y is the image, so no partial mixes two
// images -- and a finishing launch (one workgroup per image) that adds the partials in a fixed order.  No atomics: the same bits on
// every run.  w may have any sign.  NaN features reach out[b] and the pooled output as through torch's relu / max_pool2d.
//
// LPIPS as a training loss (ABI 43) adds the adjoints, for the restored half alone:
//
//   grl_lpips_tap (gmax != NULL)   the TRAIN instantiation of the tap template also leaves G = max over restored pixels and unmasked
//                                  channels of |d term / d f0_c| -- one fp32 partial per workgroup, reduced by the finishing launch
//   grl_lpips_tap_bwd              d = k * (the tap term's gradient) + the pool gradient routed to the first maximum of its window,
//                                  both under the select pre > 0; the forward's ownership, so norms, the dot product sum_j e_j u0_j
//                                  and the routing are register + xor-shuffle work inside a group.  The restored half's four pixels
//                                  stay in registers (the argmax needs them all); the target's are read pixel by pixel
//   grl_lpips_prep_bwd             dx_c = 2 * g_c / scale_c * (1 / S)
#include "common.h"
#include "grl_hip_internal.h"

namespace {

constexpr int LT = 256;       // threads per workgroup
constexpr int ITER = 4;       // cells per group and workgroup

// the package's ScalingLayer buffers are float32 tensors built from these decimals: the nearest floats, not the doubles
__constant__ float LPIPS_SHIFT[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float LPIPS_SCALE[3] = {0.458f, 0.448f, 0.450f};

__global__ __launch_bounds__(LT) void lpips_prep_kernel(GrlLpipsPrepArgs p) {
    const int64_t n = (int64_t)p.B * p.H * p.W;
    const int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % p.W), y = (int)((i / p.W) % p.H), b = (int)(i / ((int64_t)p.W * p.H));
    const float* src = p.image + b * p.stride[0] + y * p.stride[2] + x * p.stride[3];
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = 2.0f * src[c * p.stride[1]] - 1.0f;        // 2x is exact: one rounding, contracted or not
        v[c] = (t - LPIPS_SHIFT[c]) / LPIPS_SCALE[c];
    }
    *(float4*)(p.tok + i * p.ldt) = float4{v[0], v[1], v[2], 0.0f};
}

// torch's relu and max_pool2d keep a NaN; fmaxf would drop it
__device__ __forceinline__ float nan_max(float m, float a) { return (a > m || a != a) ? a : m; }
__device__ __forceinline__ float4 f4_max(float4 m, float4 a) {
    return float4{nan_max(m.x, a.x), nan_max(m.y, a.y), nan_max(m.z, a.z), nan_max(m.w, a.w)};
}
__device__ __forceinline__ float f4_sq(float4 a) { return (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w); }

// a * r as a rounded fp32 value of its own: equal features must give a difference of exactly 0, and under -ffp-contract=fast the
// subtraction that follows would otherwise take one product unrounded into a fused multiply-add (the empty asm is the fence)
__device__ __forceinline__ float unit(float a, float r) {
    float u = a * r;
    asm("" : "+v"(u));
    return u;
}

template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the plain conversion, as torch's .half(): the saturating pack_f16 turns a NaN into -65504 (v_med3_f32 answers the smaller of the
// other two), and a NaN feature has to reach the next block
__device__ __forceinline__ void store_half4(gemm_t* dst, float4 v) {
    uint2 pk;
    pk.x = pack_f16_raw(v.x, v.y);
    pk.y = pack_f16_raw(v.z, v.w);
    *(uint2*)dst = pk;
}

template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// the tap term's gradient at one channel before k: r * (e - (f / n) * dot), e = 2 w (u0 - u1), dot = sum_j e_j u0_j
__device__ __forceinline__ float tap_grad(float f, float e, float r, float inv_n, float dot) { return r * (e - (f * inv_n) * dot); }

// G lanes per cell, Q quads per lane: C = 4 * G * Q.  TRAIN: the gradient bound G_l as well (gpartial); the rest is the same code
template <int G, int Q, bool TRAIN>
__global__ __launch_bounds__(LT) void lpips_tap_kernel(GrlLpipsTapArgs p) {
    constexpr int GROUPS = LT / G;
    __shared__ double gsum[GROUPS];
    __shared__ float gtop[GROUPS];
    float top = 0.0f;
    const int Hc = (p.H + 1) >> 1, Wc = (p.W + 1) >> 1, Hp = p.H >> 1, Wp = p.W >> 1;
    const int64_t cells = (int64_t)Hc * Wc;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const int b = blockIdx.y;
    const int64_t rows = (int64_t)p.B * p.H * p.W;                 // the target's half starts here
    const int64_t prows = (int64_t)p.B * Hp * Wp;
    float4 wq[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) wq[q] = *(const float4*)(p.w + 4 * (lane + q * G));
    double acc = 0.0;
    for (int it = 0; it < ITER; ++it) {
        const int64_t cell = ((int64_t)blockIdx.x * ITER + it) * GROUPS + grp;
        if (cell >= cells) break;                                  // uniform within a group: the shuffles below stay inside it
        const int cy = (int)(cell / Wc), cx = (int)(cell % Wc);
        float4 m0[Q], m1[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) m0[q] = m1[q] = float4{0, 0, 0, 0};       // ReLU: the running maximum starts at 0
        float4 a0[4][Q], a1[4][Q];
        bool have[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = 2 * cy + (j >> 1), x = 2 * cx + (j & 1);
            have[j] = y < p.H && x < p.W;
            if (have[j]) {
                const int64_t row = ((int64_t)b * p.H + y) * p.W + x;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    a0[j][q] = *(const float4*)(p.f + row * p.ldf + 4 * (lane + q * G));
                    a1[j][q] = *(const float4*)(p.f + (rows + row) * p.ldf + 4 * (lane + q * G));
                }
            } else {
#pragma unroll
                for (int q = 0; q < Q; ++q) a0[j][q] = a1[j][q] = float4{0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                m0[q] = f4_max(m0[q], a0[j][q]);
                m1[q] = f4_max(m1[q], a1[j][q]);
                a0[j][q] = f4_max(float4{0, 0, 0, 0}, a0[j][q]);
                a1[j][q] = f4_max(float4{0, 0, 0, 0}, a1[j][q]);
                s0 += f4_sq(a0[j][q]);
                s1 += f4_sq(a1[j][q]);
            }
            s0 = group_sum<G>(s0);
            s1 = group_sum<G>(s1);
            const float r0 = 1.0f / (sqrtf(s0) + 1e-10f), r1 = 1.0f / (sqrtf(s1) + 1e-10f);      // the eps is outside the root
            float t = 0.0f;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float dx = unit(a0[j][q].x, r0) - unit(a1[j][q].x, r1), dy = unit(a0[j][q].y, r0) - unit(a1[j][q].y, r1);
                const float dz = unit(a0[j][q].z, r0) - unit(a1[j][q].z, r1), dw = unit(a0[j][q].w, r0) - unit(a1[j][q].w, r1);
                t += (wq[q].x * (dx * dx) + wq[q].y * (dy * dy)) + (wq[q].z * (dz * dz) + wq[q].w * (dw * dw));
            }
            t = group_sum<G>(t);
            if (have[j]) acc += (double)t;
            if constexpr (TRAIN) {
                // a pixel outside the image holds zeros: every channel is masked and it adds nothing
                const float n0 = sqrtf(s0), inv_n0 = n0 > 0.0f ? 1.0f / n0 : 0.0f;
                float e[Q][4], dot = 0.0f;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const float f0[4] = {a0[j][q].x, a0[j][q].y, a0[j][q].z, a0[j][q].w}, f1[4] = {a1[j][q].x, a1[j][q].y, a1[j][q].z, a1[j][q].w};
                    const float wv[4] = {wq[q].x, wq[q].y, wq[q].z, wq[q].w};
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        e[q][c] = 2.0f * wv[c] * (unit(f0[c], r0) - unit(f1[c], r1));
                        dot += e[q][c] * unit(f0[c], r0);
                    }
                }
                dot = group_sum<G>(dot);
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const float f0[4] = {a0[j][q].x, a0[j][q].y, a0[j][q].z, a0[j][q].w};
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (f0[c] > 0.0f) top = fmaxf(top, fabsf(tap_grad(f0[c], e[q][c], r0, inv_n0, dot)));
                }
            }
        }
        if (p.pool && cy < Hp && cx < Wp) {
            const int64_t prow = ((int64_t)b * Hp + cy) * Wp + cx;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                store_half4((gemm_t*)p.pool_out + prow * p.ldp + 4 * (lane + q * G), m0[q]);
                store_half4((gemm_t*)p.pool_out + (prows + prow) * p.ldp + 4 * (lane + q * G), m1[q]);
            }
        }
    }
    if constexpr (TRAIN) {
        top = group_max<G>(top);
        if (lane == 0) gtop[grp] = top;
    }
    if (lane == 0) gsum[grp] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double d = 0.0;
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) d += gsum[g];
        p.partial[(int64_t)b * gridDim.x + blockIdx.x] = d;
        if constexpr (TRAIN) {
            float m = 0.0f;
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) m = fmaxf(m, gtop[g]);
            p.gpartial[(int64_t)b * gridDim.x + blockIdx.x] = m;
        }
    }
}

// one workgroup per image: out[b] (+)= sum(partial[b]) / (H * W), in a fixed order; with gmax, workgroup 0 also leaves the maximum of
// all gridDim.x * n gradient-bound partials there
__global__ __launch_bounds__(LT) void lpips_tap_finish_kernel(const double* __restrict__ partial, int n, double* out, double pixels, int accumulate,
                                                              const float* __restrict__ gpartial, float* gmax) {
    __shared__ double acc[LT];
    __shared__ float top[LT];
    const double* src = partial + (int64_t)blockIdx.x * n;
    double d = 0.0;
    for (int i = threadIdx.x; i < n; i += LT) d += src[i];
    acc[threadIdx.x] = d;
    __syncthreads();
    for (int o = LT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) acc[threadIdx.x] += acc[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double term = acc[0] / pixels;
        out[blockIdx.x] = accumulate ? out[blockIdx.x] + term : term;
    }
    if (gmax != nullptr && blockIdx.x == 0) {
        float m = 0.0f;
        for (int64_t i = threadIdx.x; i < (int64_t)gridDim.x * n; i += LT) m = fmaxf(m, gpartial[i]);
        top[threadIdx.x] = m;
        __syncthreads();
        for (int o = LT / 2; o > 0; o >>= 1) {
            if (threadIdx.x < o) top[threadIdx.x] = fmaxf(top[threadIdx.x], top[threadIdx.x + o]);
            __syncthreads();
        }
        if (threadIdx.x == 0) gmax[0] = top[0];
    }
}

// the adjoint of the tap for the restored half: the forward's ownership (a group of G lanes owns a 2 x 2 cell)
template <int G, int Q>
__global__ __launch_bounds__(LT) void lpips_tap_bwd_kernel(GrlLpipsTapBwdArgs p) {
    constexpr int GROUPS = LT / G;
    const int Hc = (p.H + 1) >> 1, Wc = (p.W + 1) >> 1, Hp = p.H >> 1, Wp = p.W >> 1;
    const int64_t cells = (int64_t)Hc * Wc;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const int b = blockIdx.y;
    const int64_t rows = (int64_t)p.B * p.H * p.W;                 // the target's half starts here
    float wv[Q][4];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float4 t = *(const float4*)(p.w + 4 * (lane + q * G));
        wv[q][0] = t.x, wv[q][1] = t.y, wv[q][2] = t.z, wv[q][3] = t.w;
    }
    for (int it = 0; it < ITER; ++it) {
        const int64_t cell = ((int64_t)blockIdx.x * ITER + it) * GROUPS + grp;
        if (cell >= cells) break;                                  // uniform within a group: the shuffles below stay inside it
        const int cy = (int)(cell / Wc), cx = (int)(cell % Wc);
        float a0[4][Q][4];                                         // the restored half's pre-activation: all four pixels (the argmax)
        bool have[4];
        int64_t row[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = 2 * cy + (j >> 1), x = 2 * cx + (j & 1);
            have[j] = y < p.H && x < p.W;
            row[j] = have[j] ? ((int64_t)b * p.H + y) * p.W + x : 0;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float4 t = have[j] ? *(const float4*)(p.f + row[j] * p.ldf + 4 * (lane + q * G)) : float4{0, 0, 0, 0};
                a0[j][q][0] = t.x, a0[j][q][1] = t.y, a0[j][q][2] = t.z, a0[j][q][3] = t.w;
            }
        }
        // the pool gradient goes to the first maximum in (dy, dx) row-major order, and only to a positive one (ReLU): strict > from a
        // start of 0; at = -1 where the window holds none.  Cells past MaxPool's floor (odd H or W) have no pool term
        float dp[Q][4];
        int at[Q][4];
        const bool pooled = p.dpool != nullptr && cy < Hp && cx < Wp;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            float4 t = float4{0, 0, 0, 0};
            if (pooled) t = *(const float4*)(p.dpool + (((int64_t)b * Hp + cy) * Wp + cx) * p.lddp + 4 * (lane + q * G));
            dp[q][0] = t.x, dp[q][1] = t.y, dp[q][2] = t.z, dp[q][3] = t.w;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float best = 0.0f;
                at[q][c] = -1;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (a0[j][q][c] > best) best = a0[j][q][c], at[q][c] = j;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float f0[Q][4], f1[Q][4], s0 = 0.0f, s1 = 0.0f;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float4 t = have[j] ? *(const float4*)(p.f + (rows + row[j]) * p.ldf + 4 * (lane + q * G)) : float4{0, 0, 0, 0};
                const float4 r1q = f4_max(float4{0, 0, 0, 0}, t);
                const float4 r0q = f4_max(float4{0, 0, 0, 0}, float4{a0[j][q][0], a0[j][q][1], a0[j][q][2], a0[j][q][3]});
                f0[q][0] = r0q.x, f0[q][1] = r0q.y, f0[q][2] = r0q.z, f0[q][3] = r0q.w;
                f1[q][0] = r1q.x, f1[q][1] = r1q.y, f1[q][2] = r1q.z, f1[q][3] = r1q.w;
                s0 += f4_sq(r0q);
                s1 += f4_sq(r1q);
            }
            s0 = group_sum<G>(s0);
            s1 = group_sum<G>(s1);
            const float n0 = sqrtf(s0), inv_n0 = n0 > 0.0f ? 1.0f / n0 : 0.0f;
            const float r0 = 1.0f / (n0 + 1e-10f), r1 = 1.0f / (sqrtf(s1) + 1e-10f);             // the eps is outside the root
            float e[Q][4], dot = 0.0f;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    e[q][c] = 2.0f * wv[q][c] * (unit(f0[q][c], r0) - unit(f1[q][c], r1));     // normalise, then subtract, as the forward
                    dot += e[q][c] * unit(f0[q][c], r0);
                }
            }
            dot = group_sum<G>(dot);
            if (have[j]) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    float d[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float g = p.k * tap_grad(f0[q][c], e[q][c], r0, inv_n0, dot) + (at[q][c] == j ? dp[q][c] : 0.0f);
                        d[c] = a0[j][q][c] > 0.0f ? g : 0.0f;      // a select: an all-zero pixel gives exact zeros
                    }
                    *(float4*)(p.d + row[j] * p.ldd + 4 * (lane + q * G)) = float4{d[0], d[1], d[2], d[3]};
                }
            }
        }
    }
}

__global__ __launch_bounds__(LT) void lpips_prep_bwd_kernel(GrlLpipsPrepBwdArgs p) {
    const int64_t n = (int64_t)p.B * p.H * p.W;
    const int64_t i = (int64_t)blockIdx.x * LT + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % p.W), y = (int)((i / p.W) % p.H), b = (int)(i / ((int64_t)p.W * p.H));
    const float4 g = *(const float4*)(p.tok + i * p.ldt);
    const float v[3] = {g.x, g.y, g.z};
    float* dst = p.dx + b * p.stride[0] + y * p.stride[2] + x * p.stride[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c * p.stride[1]] = (2.0f * v[c] / LPIPS_SCALE[c]) * p.scale;       // scale: 1 / S, a power of two
}

int group_lanes(int32_t C_) { return C_ / 4 < 64 ? C_ / 4 : 64; }

// workgroups per image, or an error
int64_t tap_wgs(int32_t B, int32_t H, int32_t W, int32_t C_) {
    if (B <= 0 || H <= 0 || W <= 0) return GRL_ERR_BAD_ARG;
    if (C_ != 64 && C_ != 128 && C_ != 256 && C_ != 512) return GRL_ERR_UNSUPPORTED;
    if (B > 65535) return GRL_ERR_UNSUPPORTED;
    const int64_t cells = (int64_t)((H + 1) / 2) * ((W + 1) / 2);
    const int64_t per_wg = (int64_t)(LT / group_lanes(C_)) * ITER;
    const int64_t wgs = (cells + per_wg - 1) / per_wg;
    return wgs * B > 0x7fffffffLL ? (int64_t)GRL_ERR_UNSUPPORTED : wgs;
}

}  // namespace

extern "C" int grl_lpips_prep(void* stream, const GrlLpipsPrepArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const GrlLpipsPrepArgs& p = *args;
    if (p.image == nullptr || p.tok == nullptr || p.B <= 0 || p.H <= 0 || p.W <= 0) return GRL_ERR_BAD_ARG;
    if (p.ldt < 4 || (p.ldt % 4) || ((uintptr_t)p.tok % 16) || ((uintptr_t)p.image % 4)) return GRL_ERR_BAD_ARG;
    for (int d = 0; d < 4; ++d)
        if (p.stride[d] < 0) return GRL_ERR_BAD_ARG;
    const int64_t n = (int64_t)p.B * p.H * p.W;
    if ((n + LT - 1) / LT > 0x7fffffffLL) return GRL_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lpips_prep_kernel, dim3((unsigned)((n + LT - 1) / LT)), dim3(LT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_lpips_tap_num_workgroups(int32_t B, int32_t H, int32_t W, int32_t C_) {
    const int64_t wgs = tap_wgs(B, H, W, C_);
    return wgs < 0 ? (int)wgs : (int)(wgs * B);
}

extern "C" int grl_lpips_tap(void* stream, const GrlLpipsTapArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const GrlLpipsTapArgs& p = *args;
    const int64_t wgs = tap_wgs(p.B, p.H, p.W, p.C);
    if (wgs < 0) return (int)wgs;
    if (p.f == nullptr || p.w == nullptr || p.partial == nullptr || p.out == nullptr) return GRL_ERR_BAD_ARG;
    if ((p.ldf % 4) || p.ldf < p.C || ((uintptr_t)p.f % 16) || ((uintptr_t)p.w % 16)) return GRL_ERR_BAD_ARG;
    if (p.n_partial < wgs * p.B || ((uintptr_t)p.partial % 8) || ((uintptr_t)p.out % 8)) return GRL_ERR_BAD_ARG;
    const bool train = p.gmax != nullptr;
    if (train && (p.gpartial == nullptr || ((uintptr_t)p.gpartial % 4) || ((uintptr_t)p.gmax % 4))) return GRL_ERR_BAD_ARG;
    if (p.pool) {
        if (p.pool_out == nullptr || p.H < 2 || p.W < 2) return GRL_ERR_BAD_ARG;
        if ((p.ldp % 4) || p.ldp < p.C || ((uintptr_t)p.pool_out % 8)) return GRL_ERR_BAD_ARG;
    }
    const dim3 grid((unsigned)wgs, (unsigned)p.B);
    hipStream_t s = (hipStream_t)stream;
    if (train) {
        switch (p.C) {
            case 64: hipLaunchKernelGGL((lpips_tap_kernel<16, 1, true>), grid, dim3(LT), 0, s, p); break;
            case 128: hipLaunchKernelGGL((lpips_tap_kernel<32, 1, true>), grid, dim3(LT), 0, s, p); break;
            case 256: hipLaunchKernelGGL((lpips_tap_kernel<64, 1, true>), grid, dim3(LT), 0, s, p); break;
            default: hipLaunchKernelGGL((lpips_tap_kernel<64, 2, true>), grid, dim3(LT), 0, s, p); break;
        }
    } else {
        switch (p.C) {
            case 64: hipLaunchKernelGGL((lpips_tap_kernel<16, 1, false>), grid, dim3(LT), 0, s, p); break;
            case 128: hipLaunchKernelGGL((lpips_tap_kernel<32, 1, false>), grid, dim3(LT), 0, s, p); break;
            case 256: hipLaunchKernelGGL((lpips_tap_kernel<64, 1, false>), grid, dim3(LT), 0, s, p); break;
            default: hipLaunchKernelGGL((lpips_tap_kernel<64, 2, false>), grid, dim3(LT), 0, s, p); break;
        }
    }
    GRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(lpips_tap_finish_kernel, dim3((unsigned)p.B), dim3(LT), 0, s, (const double*)p.partial, (int)wgs, p.out,
                       (double)p.H * (double)p.W, p.accumulate, (const float*)p.gpartial, train ? p.gmax : nullptr);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_lpips_tap_bwd(void* stream, const GrlLpipsTapBwdArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const GrlLpipsTapBwdArgs& p = *args;
    const int64_t wgs = tap_wgs(p.B, p.H, p.W, p.C);
    if (wgs < 0) return (int)wgs;
    if (p.f == nullptr || p.w == nullptr || p.d == nullptr) return GRL_ERR_BAD_ARG;
    if ((p.ldf % 4) || p.ldf < p.C || ((uintptr_t)p.f % 16) || ((uintptr_t)p.w % 16)) return GRL_ERR_BAD_ARG;
    if ((p.ldd % 4) || p.ldd < p.C || ((uintptr_t)p.d % 16)) return GRL_ERR_BAD_ARG;
    if (p.dpool != nullptr && ((p.lddp % 4) || p.lddp < p.C || ((uintptr_t)p.dpool % 16) || p.H < 2 || p.W < 2)) return GRL_ERR_BAD_ARG;
    const dim3 grid((unsigned)wgs, (unsigned)p.B);
    hipStream_t s = (hipStream_t)stream;
    switch (p.C) {
        case 64: hipLaunchKernelGGL((lpips_tap_bwd_kernel<16, 1>), grid, dim3(LT), 0, s, p); break;
        case 128: hipLaunchKernelGGL((lpips_tap_bwd_kernel<32, 1>), grid, dim3(LT), 0, s, p); break;
        case 256: hipLaunchKernelGGL((lpips_tap_bwd_kernel<64, 1>), grid, dim3(LT), 0, s, p); break;
        default: hipLaunchKernelGGL((lpips_tap_bwd_kernel<64, 2>), grid, dim3(LT), 0, s, p); break;
    }
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_lpips_prep_bwd(void* stream, const GrlLpipsPrepBwdArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const GrlLpipsPrepBwdArgs& p = *args;
    if (p.tok == nullptr || p.dx == nullptr || p.B <= 0 || p.H <= 0 || p.W <= 0) return GRL_ERR_BAD_ARG;
    if (p.ldt < 4 || (p.ldt % 4) || ((uintptr_t)p.tok % 16) || ((uintptr_t)p.dx % 4)) return GRL_ERR_BAD_ARG;
    for (int d = 0; d < 4; ++d)
        if (p.stride[d] < 0) return GRL_ERR_BAD_ARG;
    const int64_t n = (int64_t)p.B * p.H * p.W;
    if ((n + LT - 1) / LT > 0x7fffffffLL) return GRL_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lpips_prep_bwd_kernel, dim3((unsigned)((n + LT - 1) / LT)), dim3(LT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
