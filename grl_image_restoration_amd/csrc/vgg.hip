// Everything between the 3x3 convolutions of the VGG19 perceptual loss (gfx950):
//
//   grl_vgg_prep_fwd / _bwd   (x + 1) / 2, (x - mean) / std of VGGFeatureExtractor.forward     models/aux_archs/vgg.py:257-260
//                             with the float32 mean / std buffers                               models/aux_archs/vgg.py:240-246
//   grl_vgg_tap_fwd           L1Loss on one tapped pre-ReLU feature pair, its layer weight      losses/losses.py:139-143
//                             and the ReLU + MaxPool2d(2, 2) that follow the tapped layer       models/aux_archs/vgg.py:223,263-266
//   grl_vgg_tap_bwd           autograd through those three for the restored image's features
//
// All four stream channels-last token matrices [B*H*W, C] in 16-byte pieces and are bandwidth bound.  The tap kernels give one thread a
// 2 x 2 CELL of pixels x 4 channels: the cell is the pool window, so the maximum, the argmax of the backward pass and the L1 terms of
// four pixels come from the same eight 16-byte loads.  Cells cover ceil(H/2) x ceil(W/2): a cell on an odd last row / column holds
// the pixels that MaxPool2d's floor drops -- they take part in the L1 term and get no pool output / pool gradient.
// The L1 sum: fp32 inside a thread (<= 16 terms), fp64 from there on -- wave shuffles, one fp64 partial per workgroup, and a
// one-workgroup finishing launch that adds the partials in a fixed order and the layer's share into the loss scalar.  No atomics:
// the loss is the same bits on every run.  NaN features propagate as they do through torch's relu / max_pool2d / l1_loss: into the
// pooled output and the loss (a diverged generator shows as a NaN loss); the gradient is torch autograd's, element for element.
#include "common.h"
#include "grl_hip_internal.h"

namespace {

constexpr int VT = 256;       // threads per workgroup

// the reference's buffers are float32 tensors built from these decimals (vgg.py:241,245): the nearest floats, not the doubles
__constant__ float VGG_MEAN[3] = {0.485f, 0.456f, 0.406f};
__constant__ float VGG_STD[3] = {0.229f, 0.224f, 0.225f};

__global__ __launch_bounds__(VT) void vgg_prep_fwd_kernel(GrlVggPrepArgs p) {
    const int64_t n = (int64_t)p.B * p.H * p.W;
    const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % p.W), y = (int)((i / p.W) % p.H), b = (int)(i / ((int64_t)p.W * p.H));
    const float* src = p.image + b * p.stride[0] + y * p.stride[2] + x * p.stride[3];
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = src[c * p.stride[1]];
        if (p.range_norm) t = (t + 1.0f) * 0.5f;
        if (p.use_input_norm) t = (t - VGG_MEAN[c]) / VGG_STD[c];
        v[c] = t;
    }
    *(float4*)(p.tok + i * p.ldt) = float4{v[0], v[1], v[2], 0.0f};
}

__global__ __launch_bounds__(VT) void vgg_prep_bwd_kernel(GrlVggPrepArgs p) {
    const int64_t n = (int64_t)p.B * p.H * p.W;
    const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % p.W), y = (int)((i / p.W) % p.H), b = (int)(i / ((int64_t)p.W * p.H));
    const float4 g = *(const float4*)(p.tok + i * p.ldt);
    const float v[3] = {g.x, g.y, g.z};
    float* dst = p.image + b * p.stride[0] + y * p.stride[2] + x * p.stride[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = v[c];
        if (p.use_input_norm) t = t / VGG_STD[c];
        dst[c * p.stride[1]] = t * p.scale;        // scale: 1 / S (a power of two) and the 1/2 of range_norm
    }
}

struct Cell {
    int b, cy, cx, c;
};

__device__ __forceinline__ Cell cell_of(int64_t i, int Hc, int Wc, int C4) {
    Cell q;
    q.c = (int)(i % C4) * 4;
    const int64_t cell = i / C4;
    q.cx = (int)(cell % Wc);
    q.cy = (int)((cell / Wc) % Hc);
    q.b = (int)(cell / ((int64_t)Wc * Hc));
    return q;
}

// running maximum as torch's max_pool2d keeps it: a NaN replaces the maximum and then stays (fmaxf would drop it, and a diverged
// generator would show a finite perceptual path)
__device__ __forceinline__ float nan_max(float m, float a) { return (a > m || a != a) ? a : m; }
__device__ __forceinline__ float4 f4_max(float4 m, float4 a) {
    return float4{nan_max(m.x, a.x), nan_max(m.y, a.y), nan_max(m.z, a.z), nan_max(m.w, a.w)};
}

__device__ __forceinline__ void store_pool(void* base, int dtype, int64_t row, int64_t ld, int c, float4 v) {
    if (dtype == GRL_DT_F32) {
        *(float4*)((float*)base + row * ld + c) = v;
    } else {
        uint2 pk;
        pk.x = pack_f16(v.x, v.y);
        pk.y = pack_f16(v.z, v.w);
        *(uint2*)((gemm_t*)base + row * ld + c) = pk;
    }
}

__global__ __launch_bounds__(VT) void vgg_tap_fwd_kernel(GrlVggTapArgs p) {
    __shared__ double wsum[VT / 64];
    const int Hc = (p.H + 1) >> 1, Wc = (p.W + 1) >> 1, Hp = p.H >> 1, Wp = p.W >> 1, C4 = p.C >> 2;
    const int64_t n = (int64_t)p.B * Hc * Wc * C4;
    const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
    float s = 0.0f;
    if (i < n) {
        const Cell q = cell_of(i, Hc, Wc, C4);
        float4 mx = float4{0, 0, 0, 0}, mg = float4{0, 0, 0, 0};      // ReLU: the running maximum starts at 0
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = 2 * q.cy + (j >> 1), x = 2 * q.cx + (j & 1);
            if (y < p.H && x < p.W) {
                const int64_t row = ((int64_t)q.b * p.H + y) * p.W + x;
                const float4 a = *(const float4*)(p.fx + row * p.ldf + q.c), g = *(const float4*)(p.fg + row * p.ldf + q.c);
                s += fabsf(a.x - g.x);
                s += fabsf(a.y - g.y);
                s += fabsf(a.z - g.z);
                s += fabsf(a.w - g.w);
                mx = f4_max(mx, a);
                mg = f4_max(mg, g);
            }
        }
        if (p.pool && q.cy < Hp && q.cx < Wp) {
            const int64_t prow = ((int64_t)q.b * Hp + q.cy) * Wp + q.cx;
            store_pool(p.px, p.pool_dtype, prow, p.ldp, q.c, mx);
            store_pool(p.pg, p.pool_dtype, prow, p.ldp, q.c, mg);
        }
    }
    double d = (double)s;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) p.partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// one workgroup: loss (+)= coef * sum(partial), in a fixed order
__global__ __launch_bounds__(VT) void vgg_tap_finish_kernel(const double* __restrict__ partial, int n, float* loss, float* layer_sum, double coef,
                                                            int accumulate) {
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

__global__ __launch_bounds__(VT) void vgg_tap_bwd_kernel(GrlVggTapArgs p) {
    const int Hc = (p.H + 1) >> 1, Wc = (p.W + 1) >> 1, Hp = p.H >> 1, Wp = p.W >> 1, C4 = p.C >> 2;
    const int64_t n = (int64_t)p.B * Hc * Wc * C4;
    const int64_t i = (int64_t)blockIdx.x * VT + threadIdx.x;
    if (i >= n) return;
    const Cell q = cell_of(i, Hc, Wc, C4);
    const bool pooled = p.dpool != nullptr && q.cy < Hp && q.cx < Wp;      // (then all four pixels of the cell exist)
    float a[4][4], sg[4][4];
    bool have[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = 2 * q.cy + (j >> 1), x = 2 * q.cx + (j & 1);
        have[j] = y < p.H && x < p.W;
        if (have[j]) {
            const int64_t row = ((int64_t)q.b * p.H + y) * p.W + x;
            const float4 fa = *(const float4*)(p.fx + row * p.ldf + q.c), fg = *(const float4*)(p.fg + row * p.ldf + q.c);
            const float va[4] = {fa.x, fa.y, fa.z, fa.w}, vg[4] = {fg.x, fg.y, fg.z, fg.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[j][e] = va[e];
                const float d = va[e] - vg[e];
                sg[j][e] = p.k * (float)((d > 0.0f) - (d < 0.0f));        // sign(0) = 0 (and sign(NaN) = 0, as torch's abs backward has it)
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) a[j][e] = sg[j][e] = 0.0f;
        }
    }
    if (pooled) {
        const int64_t prow = ((int64_t)q.b * Hp + q.cy) * Wp + q.cx;
        const float4 d4 = *(const float4*)(p.dpool + prow * p.lddp + q.c);
        const float dp[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // the first maximum in (dy, dx) row-major order, and only a positive one (ReLU): strict > from a start of 0.  A NaN takes
            // the window as in torch's max_pool2d, and torch's ReLU backward (result <= 0 ? 0 : grad) lets its gradient through
            float best = 0.0f;
            int at = -1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (a[j][e] > best || a[j][e] != a[j][e]) {
                    best = a[j][e];
                    at = j;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) sg[j][e] += (at == j) ? dp[e] : 0.0f;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (have[j]) {
            const int y = 2 * q.cy + (j >> 1), x = 2 * q.cx + (j & 1);
            const int64_t row = ((int64_t)q.b * p.H + y) * p.W + x;
            *(float4*)(p.dfx + row * p.lddf + q.c) = float4{sg[j][0], sg[j][1], sg[j][2], sg[j][3]};
        }
    }
}

int64_t tap_threads(int32_t B, int32_t H, int32_t W, int32_t C_) { return (int64_t)B * ((H + 1) / 2) * ((W + 1) / 2) * (C_ / 4); }

int check_prep(const GrlVggPrepArgs& p) {
    if (p.image == nullptr || p.tok == nullptr || p.B <= 0 || p.H <= 0 || p.W <= 0) return GRL_ERR_BAD_ARG;
    if (p.ldt < 4 || (p.ldt % 4) || ((uintptr_t)p.tok % 16) || ((uintptr_t)p.image % 4)) return GRL_ERR_BAD_ARG;
    for (int d = 0; d < 4; ++d)
        if (p.stride[d] < 0) return GRL_ERR_BAD_ARG;
    if (((int64_t)p.B * p.H * p.W + VT - 1) / VT > 0x7fffffffLL) return GRL_ERR_UNSUPPORTED;
    return 0;
}

int check_tap(const GrlVggTapArgs& p) {
    if (p.fx == nullptr || p.fg == nullptr || p.B <= 0 || p.H <= 0 || p.W <= 0 || p.C <= 0) return GRL_ERR_BAD_ARG;
    if ((p.C % 4) || (p.ldf % 4) || p.ldf < p.C || ((uintptr_t)p.fx % 16) || ((uintptr_t)p.fg % 16)) return GRL_ERR_BAD_ARG;
    if ((tap_threads(p.B, p.H, p.W, p.C) + VT - 1) / VT > 0x7fffffffLL) return GRL_ERR_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int grl_vgg_prep_fwd(void* stream, const GrlVggPrepArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const int e = check_prep(*args);
    if (e != 0) return e;
    const int64_t n = (int64_t)args->B * args->H * args->W;
    hipLaunchKernelGGL(vgg_prep_fwd_kernel, dim3((unsigned)((n + VT - 1) / VT)), dim3(VT), 0, (hipStream_t)stream, *args);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_vgg_prep_bwd(void* stream, const GrlVggPrepArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const int e = check_prep(*args);
    if (e != 0) return e;
    const int64_t n = (int64_t)args->B * args->H * args->W;
    hipLaunchKernelGGL(vgg_prep_bwd_kernel, dim3((unsigned)((n + VT - 1) / VT)), dim3(VT), 0, (hipStream_t)stream, *args);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_vgg_tap_num_workgroups(int32_t B, int32_t H, int32_t W, int32_t C_) {
    if (B <= 0 || H <= 0 || W <= 0 || C_ <= 0 || (C_ % 4)) return GRL_ERR_BAD_ARG;
    const int64_t wgs = (tap_threads(B, H, W, C_) + VT - 1) / VT;
    return wgs > 0x7fffffffLL ? GRL_ERR_UNSUPPORTED : (int)wgs;
}

extern "C" int grl_vgg_tap_fwd(void* stream, const GrlVggTapArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const GrlVggTapArgs& p = *args;
    const int e = check_tap(p);
    if (e != 0) return e;
    const int64_t wgs = (tap_threads(p.B, p.H, p.W, p.C) + VT - 1) / VT;
    if (p.partial == nullptr || p.loss == nullptr || p.n_partial < wgs || ((uintptr_t)p.partial % 8)) return GRL_ERR_BAD_ARG;
    if (p.pool) {
        if (p.px == nullptr || p.pg == nullptr || (p.H < 2) || (p.W < 2)) return GRL_ERR_BAD_ARG;
        if (p.pool_dtype != GRL_DT_F32 && p.pool_dtype != GRL_DT_F16) return GRL_ERR_UNSUPPORTED;
        const int al = p.pool_dtype == GRL_DT_F32 ? 16 : 8;
        if ((p.ldp % 4) || p.ldp < p.C || ((uintptr_t)p.px % al) || ((uintptr_t)p.pg % al)) return GRL_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL(vgg_tap_fwd_kernel, dim3((unsigned)wgs), dim3(VT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(vgg_tap_finish_kernel, dim3(1), dim3(VT), 0, (hipStream_t)stream, (const double*)p.partial, (int)wgs, p.loss, p.layer_sum,
                       (double)p.coef, p.accumulate);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_vgg_tap_bwd(void* stream, const GrlVggTapArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const GrlVggTapArgs& p = *args;
    const int e = check_tap(p);
    if (e != 0) return e;
    if (p.dfx == nullptr || (p.lddf % 4) || p.lddf < p.C || ((uintptr_t)p.dfx % 16)) return GRL_ERR_BAD_ARG;
    if (p.dpool != nullptr && ((p.lddp % 4) || p.lddp < p.C || ((uintptr_t)p.dpool % 16) || p.H < 2 || p.W < 2)) return GRL_ERR_BAD_ARG;
    const int64_t wgs = (tap_threads(p.B, p.H, p.W, p.C) + VT - 1) / VT;
    hipLaunchKernelGGL(vgg_tap_bwd_kernel, dim3((unsigned)wgs), dim3(VT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
