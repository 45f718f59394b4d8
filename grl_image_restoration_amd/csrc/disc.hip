// The two contractions of the U-Net discriminator that the 3x3 kernels do not cover (gfx950):
//
//   grl_conv4x4s2_fwd       Conv2d(Cin, Cout, 4, 2, 1, bias=False) (+ LeakyReLU)   models/aux_archs/discriminator.py:102-104,118-120
//   grl_conv4x4s2_bwd_data  its transposed convolution (autograd through F.conv2d in engines/base_gan.py:86-147)
//   grl_pack_conv4x4        the fp16 operand of either, from nn.Conv2d.weight
//   grl_upsample2x_bilinear_fwd / _bwd   F.interpolate(scale_factor=2, mode="bilinear", align_corners=False) and its adjoint
//                           models/aux_archs/discriminator.py:123,128,133
// (the weight gradient is grl_gemm_tn with taps = 16, csrc/grad.hip)
//
// Convolutions: implicit GEMM on fp16 MFMA operands with fp32 accumulation, like csrc/conv.hip, on channels-last token matrices.
// A workgroup (4 waves) owns 64 consecutive output pixels x 64 output channels; wave w owns pixels 16 w .. 16 w + 15.  The
// reduction runs over (tap, channel chunk of KC): for each step the loader GATHERS the 64 source pixels of the tap -- forward:
// x[2 oy + ky - 1, 2 ox + kx - 1], zero outside -- converts them to fp16 and stages them in LDS next to the tap's [64][KC] weight
// slice; the space-to-depth copy is never formed and all 16 taps are live.  The global loads of step s + 1 are in flight during
// the MFMAs of step s.  The product is computed transposed (rows = output channel, columns = pixel) so a lane owns 4 consecutive
// channels of one pixel and stores 16 bytes.
// Data gradient: the pixels of dx fall into four parity classes (py, px) = (iy & 1, ix & 1); each class is a 2 x 2-tap convolution
// of dy:  dx[2 qy + py, 2 qx + px, ci] = sum_{ty, tx, co} W[co][ci][1 - py + 2 ty][1 - px + 2 tx] * dy[qy + py - ty, qx + px - tx, co].
// The same kernel runs it with blockIdx.z = class, 4 taps, the transposed pack and a strided output row.
#include "common.h"
#include "grl_hip_internal.h"

namespace {

constexpr int DM = 64;    // output pixels per workgroup
constexpr int DN = 64;    // output channels per workgroup
constexpr int DTHREADS = 256;

template <int KC, bool BWD>
__global__ __launch_bounds__(DTHREADS) void conv4x4s2_kernel(GrlConvArgs p) {
    constexpr int ROWB = KC * 2 + 16;            // padded LDS row (bytes), as csrc/conv.hip
    constexpr int SEG_ROW = KC / 8;              // 16-B segments per row
    constexpr int SPT = DM * SEG_ROW / DTHREADS; // segments per thread and operand (KC 64: 2, KC 32: 1)
    constexpr int KS = KC / 32;                  // MFMA k-steps per chunk
    __shared__ __attribute__((aligned(16))) char in_s[DM * ROWB];
    __shared__ __attribute__((aligned(16))) char wt_s[DN * ROWB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, g4 = lane >> 4;
    const int Ho = p.H >> 1, Wo = p.W >> 1;      // the half-resolution grid: outputs (forward) / dy and the class grid (data gradient)
    const int64_t M = (int64_t)p.B * Ho * Wo;
    const int64_t m0 = (int64_t)blockIdx.x * DM;
    const int n0 = blockIdx.y * DN;
    const int py = BWD ? (int)(blockIdx.z >> 1) : 0, px = BWD ? (int)(blockIdx.z & 1) : 0;
    const int nkc = p.CinP / KC;
    const int ntaps = BWD ? 4 : 16;
    const int steps = ntaps * nkc;
    const int xc = p.x_cols > 0 ? p.x_cols : p.CinP;          // real source channels (multiple of 4): the rest read as zeros
    const float xsc = p.x_scale != 0.0f ? p.x_scale : 1.0f;
    const float osc = p.out_scale != 0.0f ? p.out_scale : 1.0f;

    // the (fixed) pixel and channel segment of each staging slot of this thread
    int sb[SPT], sy[SPT], sx[SPT], spix[SPT], scc[SPT];
    bool sval[SPT];
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int s = tid + i * DTHREADS;
        spix[i] = s / SEG_ROW;
        scc[i] = s % SEG_ROW;
        const int64_t m = m0 + spix[i];
        sval[i] = m < M;
        const int64_t mm = sval[i] ? m : 0;
        sx[i] = (int)(mm % Wo);
        sy[i] = (int)((mm / Wo) % Ho);
        sb[i] = (int)(mm / ((int64_t)Wo * Ho));
    }

    f32x4 acc[DN / 16];
#pragma unroll
    for (int nt = 0; nt < DN / 16; ++nt) acc[nt] = f32x4{0, 0, 0, 0};

    gemm_x8 apre[SPT], wpre[SPT];
    auto load_step = [&](int step) {
        const int tap = step / nkc, kc = step - tap * nkc;
        int wtap, oy, ox, SH, SW;
        if (BWD) {
            const int ty = tap >> 1, tx = tap & 1;
            wtap = (1 - py + 2 * ty) * 4 + (1 - px + 2 * tx);
            oy = py - ty; ox = px - tx;
            SH = Ho; SW = Wo;
        } else {
            wtap = tap;
            oy = (tap >> 2) - 1; ox = (tap & 3) - 1;
            SH = p.H; SW = p.W;
        }
        const gemm_t* wsrc = (const gemm_t*)p.w + (int64_t)wtap * p.w_tap_stride + kc * KC;
#pragma unroll
        for (int i = 0; i < SPT; ++i) {
            gemm_x8 wv = {0, 0, 0, 0, 0, 0, 0, 0};
            const int wr = n0 + spix[i];                   // (the slot's row index serves both operands: DM == DN)
            if (wr < p.CoutP) wv = *(const gemm_x8*)(wsrc + (int64_t)wr * p.CinP + scc[i] * 8);
            wpre[i] = wv;
            gemm_x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            const int gy = (BWD ? sy[i] : 2 * sy[i]) + oy, gx = (BWD ? sx[i] : 2 * sx[i]) + ox;
            const int ch0 = kc * KC + scc[i] * 8;
            if (sval[i] && (unsigned)gy < (unsigned)SH && (unsigned)gx < (unsigned)SW && ch0 < xc) {
                const int64_t row = ((int64_t)sb[i] * SH + gy) * SW + gx;
                const float4* q = (const float4*)((const float*)p.x + row * p.ldx + ch0);
                const float4 a0 = q[0];
                const float4 a1 = ch0 + 4 < xc ? q[1] : float4{0, 0, 0, 0};
                v[0] = to_f16(a0.x * xsc); v[1] = to_f16(a0.y * xsc); v[2] = to_f16(a0.z * xsc); v[3] = to_f16(a0.w * xsc);
                v[4] = to_f16(a1.x * xsc); v[5] = to_f16(a1.y * xsc); v[6] = to_f16(a1.z * xsc); v[7] = to_f16(a1.w * xsc);
            }
            apre[i] = v;
        }
    };

    load_step(0);
    for (int step = 0; step < steps; ++step) {
        __syncthreads();   // the previous step's readers are done
#pragma unroll
        for (int i = 0; i < SPT; ++i) {
            *(gemm_x8*)(in_s + spix[i] * ROWB + scc[i] * 16) = apre[i];
            *(gemm_x8*)(wt_s + spix[i] * ROWB + scc[i] * 16) = wpre[i];
        }
        __syncthreads();
        if (step + 1 < steps) load_step(step + 1);   // in flight during the MFMAs below
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const gemm_x8 af = *(const gemm_x8*)(in_s + (16 * wave + r16) * ROWB + (32 * ks + 8 * g4) * 2);
#pragma unroll
            for (int nt = 0; nt < DN / 16; ++nt) {
                const gemm_x8 wf = *(const gemm_x8*)(wt_s + (nt * 16 + r16) * ROWB + (32 * ks + 8 * g4) * 2);
                acc[nt] = mfma16_gemm(wf, af, acc[nt]);
            }
        }
    }

    // ---- epilogue: lane owns channels n0 + 16 nt + 4 g4 + [0..3] of pixel m0 + 16 wave + r16 ----
    const int64_t m = m0 + 16 * wave + r16;
    if (m >= M) return;
    int64_t orow = m;
    if (BWD) {
        const int qx = (int)(m % Wo), qy = (int)((m / Wo) % Ho), b = (int)(m / ((int64_t)Wo * Ho));
        orow = ((int64_t)b * p.H + (2 * qy + py)) * p.W + (2 * qx + px);
    }
    const int ncols = p.n_store > 0 ? p.n_store : p.CoutP;
#pragma unroll
    for (int nt = 0; nt < DN / 16; ++nt) {
        const int c = n0 + 16 * nt + 4 * g4;
        if (c >= ncols) continue;
        float v[4] = {acc[nt][0] * osc, acc[nt][1] * osc, acc[nt][2] * osc, acc[nt][3] * osc};
        if (p.act == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * p.slope;
        }
        *(float4*)((float*)p.out + orow * p.ldo + c) = float4{v[0], v[1], v[2], v[3]};
    }
}

// w [Cout][Cin][4][4] fp32 -> fp16 [16][rows_pad][cols_pad], tap = ky*4+kx;  transpose: rows = Cin side, columns = Cout side
__global__ __launch_bounds__(256) void pack_conv4x4_kernel(const float* __restrict__ w, gemm_t* __restrict__ out, int Cout, int Cin,
                                                           int rows_pad, int cols_pad, int transpose) {
    const int64_t n = (int64_t)16 * rows_pad * cols_pad;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int col = (int)(i % cols_pad), row = (int)((i / cols_pad) % rows_pad), tap = (int)(i / ((int64_t)cols_pad * rows_pad));
        const int co = transpose ? col : row, ci = transpose ? row : col;
        float v = 0.f;
        if (co < Cout && ci < Cin) v = w[((int64_t)co * Cin + ci) * 16 + tap];
        out[i] = to_f16(v);
    }
}

// one axis of the x2 bilinear map (align_corners=False): output o reads inputs i0, i1 with weights l0, l1 (torch clamps the source
// coordinate o / 2 - 0.25 at 0 and the upper index at n - 1)
__device__ __forceinline__ void up_axis(int o, int n, int& i0, int& i1, float& l0, float& l1) {
    const int i = o >> 1;
    if (o & 1) {
        i0 = i; i1 = min(i + 1, n - 1); l0 = 0.75f; l1 = 0.25f;
    } else if (i == 0) {
        i0 = 0; i1 = min(1, n - 1); l0 = 1.0f; l1 = 0.0f;
    } else {
        i0 = i - 1; i1 = i; l0 = 0.25f; l1 = 0.75f;
    }
}

__device__ __forceinline__ float4 f4_fma(float s, float4 a, float4 acc) {
    return float4{fmaf(s, a.x, acc.x), fmaf(s, a.y, acc.y), fmaf(s, a.z, acc.z), fmaf(s, a.w, acc.w)};
}
__device__ __forceinline__ float4 f4_mul(float s, float4 a) { return float4{s * a.x, s * a.y, s * a.z, s * a.w}; }

// one thread per (output pixel, 4 channels)
__global__ __launch_bounds__(256) void upsample2x_fwd_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ out, int64_t ldo,
                                                             int B, int H, int W, int C4) {
    const int64_t n = (int64_t)B * 2 * H * 2 * W * C4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C4) * 4;
    const int64_t pix = i / C4;
    const int ox = (int)(pix % (2 * W)), oy = (int)((pix / (2 * W)) % (2 * H)), b = (int)(pix / ((int64_t)4 * W * H));
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    up_axis(oy, H, y0, y1, hy0, hy1);
    up_axis(ox, W, x0, x1, wx0, wx1);
    const float* base = x + (int64_t)b * H * W * ldx + c;
    const float4 v00 = *(const float4*)(base + ((int64_t)y0 * W + x0) * ldx), v01 = *(const float4*)(base + ((int64_t)y0 * W + x1) * ldx);
    const float4 v10 = *(const float4*)(base + ((int64_t)y1 * W + x0) * ldx), v11 = *(const float4*)(base + ((int64_t)y1 * W + x1) * ldx);
    // torch's order: h0 * (w0 v00 + w1 v01) + h1 * (w0 v10 + w1 v11)
    const float4 top = f4_fma(wx1, v01, f4_mul(wx0, v00)), bot = f4_fma(wx1, v11, f4_mul(wx0, v10));
    *(float4*)(out + pix * ldo + c) = f4_fma(hy1, bot, f4_mul(hy0, top));
}

// the outputs that read input i along one axis: o = 2 i - 1 + j (j = 0..3) with weight a[j] (0: none)
__device__ __forceinline__ void up_axis_adjoint(int i, int n, float a[4]) {
    a[0] = i >= 1 ? 0.25f : 0.0f;
    a[1] = i == 0 ? 1.0f : 0.75f;
    a[2] = i == n - 1 ? 1.0f : 0.75f;
    a[3] = i <= n - 2 ? 0.25f : 0.0f;
}

// adjoint as a gather: one thread per (input pixel, 4 channels) sums its <= 16 outputs in a fixed order (no atomics)
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const float* __restrict__ dy, int64_t lddy, float* __restrict__ dx, int64_t lddx,
                                                             int B, int H, int W, int C4) {
    const int64_t n = (int64_t)B * H * W * C4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C4) * 4;
    const int64_t pix = i / C4;
    const int ix = (int)(pix % W), iy = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
    float ay[4], ax[4];
    up_axis_adjoint(iy, H, ay);
    up_axis_adjoint(ix, W, ax);
    const float* base = dy + (int64_t)b * 4 * H * W * lddy + c;
    float4 s = float4{0, 0, 0, 0};
#pragma unroll
    for (int jy = 0; jy < 4; ++jy) {
        if (ay[jy] == 0.0f) continue;
        const int oy = 2 * iy - 1 + jy;
        float4 r = float4{0, 0, 0, 0};
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            if (ax[jx] == 0.0f) continue;
            const int ox = 2 * ix - 1 + jx;
            r = f4_fma(ax[jx], *(const float4*)(base + ((int64_t)oy * 2 * W + ox) * lddy), r);
        }
        s = f4_fma(ay[jy], r, s);
    }
    *(float4*)(dx + pix * lddx + c) = s;
}

template <bool BWD>
int launch_conv4x4s2(const GrlConvArgs& p, hipStream_t st) {
    const int64_t M = (int64_t)p.B * (p.H / 2) * (p.W / 2);
    const int64_t mt = (M + DM - 1) / DM;
    if (mt > 0x7fffffffLL) return GRL_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)mt, (p.CoutP + DN - 1) / DN, BWD ? 4 : 1);
    if (p.CinP % 64 == 0) hipLaunchKernelGGL((conv4x4s2_kernel<64, BWD>), grid, dim3(DTHREADS), 0, st, p);
    else hipLaunchKernelGGL((conv4x4s2_kernel<32, BWD>), grid, dim3(DTHREADS), 0, st, p);
    GRL_CHECK_LAUNCH();
    return 0;
}

// what both directions ask of the argument block (H, W: the FULL-resolution grid -- x of the forward, dx of the data gradient)
int check_conv4x4s2(const GrlConvArgs& p) {
    if (p.x == nullptr || p.w == nullptr || p.out == nullptr) return GRL_ERR_BAD_ARG;
    if (p.B <= 0 || p.H <= 0 || p.W <= 0) return GRL_ERR_BAD_ARG;
    if ((p.H & 1) || (p.W & 1)) return GRL_ERR_UNSUPPORTED;
    if (p.CinP <= 0 || p.CoutP <= 0 || p.CinP % 32 || p.CoutP % 16 || p.CoutP > 65535 * DN) return GRL_ERR_BAD_ARG;
    if (p.x_dtype != GRL_DT_F32 || p.out_dtype != GRL_DT_F32) return GRL_ERR_UNSUPPORTED;
    if (p.x_split > 1 || p.resid != nullptr || p.pool_partial != nullptr || p.shuffle_r > 1 || p.bias != nullptr) return GRL_ERR_UNSUPPORTED;
    if (p.act != 0 && p.act != 2) return GRL_ERR_UNSUPPORTED;
    if (p.x_cols < 0 || p.n_store < 0 || (p.x_cols % 4) || (p.n_store % 4) || p.x_cols > p.CinP || p.n_store > p.CoutP) return GRL_ERR_BAD_ARG;
    const int xc = p.x_cols > 0 ? p.x_cols : p.CinP, nc = p.n_store > 0 ? p.n_store : p.CoutP;
    if ((p.ldx % 4) || (p.ldo % 4) || p.ldx < xc || p.ldo < nc) return GRL_ERR_BAD_ARG;          // 16-byte pieces of whole rows
    if (((uintptr_t)p.x % 16) || ((uintptr_t)p.out % 16) || ((uintptr_t)p.w % 16)) return GRL_ERR_BAD_ARG;
    if (p.w_tap_stride < (int64_t)p.CoutP * p.CinP) return GRL_ERR_BAD_ARG;
    return 0;
}

}  // namespace

extern "C" int grl_conv4x4s2_fwd(void* stream, const GrlConvArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const int e = check_conv4x4s2(*args);
    if (e != 0) return e;
    return launch_conv4x4s2<false>(*args, (hipStream_t)stream);
}

extern "C" int grl_conv4x4s2_bwd_data(void* stream, const GrlConvArgs* args) {
    if (args == nullptr) return GRL_ERR_BAD_ARG;
    const int e = check_conv4x4s2(*args);
    if (e != 0) return e;
    if (args->act != 0) return GRL_ERR_UNSUPPORTED;
    return launch_conv4x4s2<true>(*args, (hipStream_t)stream);
}

extern "C" int grl_pack_conv4x4(void* stream, const float* w, void* out_w, int32_t Cout, int32_t Cin, int32_t rows_pad, int32_t cols_pad,
                                int32_t transpose) {
    if (w == nullptr || out_w == nullptr || Cout <= 0 || Cin <= 0) return GRL_ERR_BAD_ARG;
    if (rows_pad < (transpose ? Cin : Cout) || cols_pad < (transpose ? Cout : Cin)) return GRL_ERR_BAD_ARG;
    const int64_t n = (int64_t)16 * rows_pad * cols_pad;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(pack_conv4x4_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, (gemm_t*)out_w, Cout, Cin, rows_pad, cols_pad,
                       transpose);
    GRL_CHECK_LAUNCH();
    return 0;
}

static int check_upsample(const float* a, int64_t lda, const float* b, int64_t ldb, int32_t B, int32_t H, int32_t W, int32_t C_) {
    if (a == nullptr || b == nullptr || B <= 0 || H <= 0 || W <= 0 || C_ <= 0) return GRL_ERR_BAD_ARG;
    if ((C_ % 4) || (lda % 4) || (ldb % 4) || lda < C_ || ldb < C_) return GRL_ERR_BAD_ARG;
    if (((uintptr_t)a % 16) || ((uintptr_t)b % 16)) return GRL_ERR_BAD_ARG;
    if (((int64_t)B * H * W * C_ + 255) / 256 > 0x7fffffffLL) return GRL_ERR_UNSUPPORTED;      // (the 2H x 2W grid in quarter-row threads)
    return 0;
}

extern "C" int grl_upsample2x_bilinear_fwd(void* stream, const float* x, int64_t ldx, float* out, int64_t ldo, int32_t B, int32_t H,
                                           int32_t W, int32_t C_) {
    const int e = check_upsample(x, ldx, out, ldo, B, H, W, C_);
    if (e != 0) return e;
    const int64_t n = (int64_t)B * 4 * H * W * (C_ / 4);
    hipLaunchKernelGGL(upsample2x_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, out, ldo, B, H, W,
                       C_ / 4);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_upsample2x_bilinear_bwd(void* stream, const float* dy, int64_t lddy, float* dx, int64_t lddx, int32_t B, int32_t H,
                                           int32_t W, int32_t C_) {
    const int e = check_upsample(dy, lddy, dx, lddx, B, H, W, C_);
    if (e != 0) return e;
    const int64_t n = (int64_t)B * H * W * (C_ / 4);
    hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, lddy, dx, lddx, B, H, W,
                       C_ / 4);
    GRL_CHECK_LAUNCH();
    return 0;
}
