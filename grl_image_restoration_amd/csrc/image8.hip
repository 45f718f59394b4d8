// 8-bit image pack (include/grl_hip.h, grl_image_pack8): the network's fp32 NCHW output as the HWC bytes a PNG encoder takes.  The
// reference rounds with tensor_round (utils/utils_image.py:30-33), hands the result to torchvision's to_pil_image, which for a float
// tensor is mul(255).byte() and a permute to HWC, and for super-resolution first enlarges the LQ with
// F.interpolate(input, scale_factor=scale) (engines/base.py:529-530, nearest).  All of it in one launch:
//
//   out[n][y][x][c] = uint8(rint(clamp(x[n][c][y / rep][x / rep], 0, 1) * 255.0f))
//
// rint rounds half to even (v_rndne_f32, as torch.round); the multiply is one fp32 multiply (__fmul_rn: nothing is contracted into
// it under -ffp-contract=fast); NaN and everything not above 0 give 0, everything above 1 gives 255.
//
// Shape: the output is one flat stream of N * H rep * W rep * C bytes.  A thread produces four consecutive bytes and stores them as
// one dword (a wave stores 256 contiguous bytes); the last thread stores its 1 .. 3 tail bytes singly.  Nothing assumes that an
// image or a row starts on a dword: the thread decomposes its first byte index into (n, y, x, c) once and steps from there.  For
// C = 3 the four bytes come from up to three planes at neighbouring columns, so across a wave every plane is read as one contiguous
// run of about 85 floats; with rep > 1 neighbouring outputs read the same source value, which the cache serves.  C and rep are
// template parameters (16 small kernels): the divisions by them are multiplications.  The input is read through its four element
// strides, so a crop is packed in place.  No LDS, no atomics, no scratch.
#include "common.h"

namespace {

constexpr int NT = 256;

struct Params {
    const float* x;
    uint8_t* out;
    int64_t sn, sc, sh, sw;       // element strides of x
    uint32_t Ho, Wo;              // output rows and columns (H rep, W rep)
    uint32_t total;               // bytes of the output, below 2^31
};

__device__ __forceinline__ uint32_t level8(float v) {
    if (!(v > 0.f)) v = 0.f;      // NaN, -inf, negatives, -0.0
    if (v > 1.f) v = 1.f;
    return (uint32_t)rintf(__fmul_rn(v, 255.0f));
}

template <int C, int REP>
__global__ __launch_bounds__(NT) void pack8_kernel(Params p) {
    const uint32_t b0 = (blockIdx.x * (uint32_t)NT + threadIdx.x) * 4u;
    if (b0 >= p.total) return;
    const uint32_t pix = b0 / C;
    uint32_t c = b0 - pix * C;
    const uint32_t row = pix / p.Wo;
    uint32_t x = pix - row * p.Wo;
    uint32_t n = row / p.Ho;
    uint32_t y = row - n * p.Ho;

    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = 0;
        if (b0 + j < p.total)
            v[j] = level8(p.x[n * p.sn + c * p.sc + (int64_t)(y / REP) * p.sh + (int64_t)(x / REP) * p.sw]);
        if (++c == C) {
            c = 0;
            if (++x == p.Wo) {
                x = 0;
                if (++y == p.Ho) { y = 0; ++n; }
            }
        }
    }
    if (b0 + 4 <= p.total) {
        *reinterpret_cast<uint32_t*>(p.out + b0) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (b0 + j < p.total) p.out[b0 + j] = (uint8_t)v[j];
    }
}

template <int C>
void launch(int rep, const Params& p, unsigned grid, hipStream_t st) {
    switch (rep) {
        case 1: hipLaunchKernelGGL((pack8_kernel<C, 1>), dim3(grid), dim3(NT), 0, st, p); break;
        case 2: hipLaunchKernelGGL((pack8_kernel<C, 2>), dim3(grid), dim3(NT), 0, st, p); break;
        case 3: hipLaunchKernelGGL((pack8_kernel<C, 3>), dim3(grid), dim3(NT), 0, st, p); break;
        case 4: hipLaunchKernelGGL((pack8_kernel<C, 4>), dim3(grid), dim3(NT), 0, st, p); break;
        case 5: hipLaunchKernelGGL((pack8_kernel<C, 5>), dim3(grid), dim3(NT), 0, st, p); break;
        case 6: hipLaunchKernelGGL((pack8_kernel<C, 6>), dim3(grid), dim3(NT), 0, st, p); break;
        case 7: hipLaunchKernelGGL((pack8_kernel<C, 7>), dim3(grid), dim3(NT), 0, st, p); break;
        default: hipLaunchKernelGGL((pack8_kernel<C, 8>), dim3(grid), dim3(NT), 0, st, p); break;
    }
}

}  // namespace

extern "C" int grl_image_pack8(void* stream, const GrlPack8Args* a) {
    if (!a || !a->x || !a->out) return GRL_ERR_BAD_ARG;
    if (a->C != 1 && a->C != 3) return GRL_ERR_BAD_ARG;
    if (a->N <= 0 || a->H <= 0 || a->W <= 0) return GRL_ERR_BAD_ARG;
    if (a->rep < 1 || a->rep > 8) return GRL_ERR_BAD_ARG;
    if ((uint64_t)a->x % 4 || (uint64_t)a->out % 4) return GRL_ERR_BAD_ARG;
    // every product below stays inside int64: Ho, Wo < 2^34; then each factor is checked before the next multiplication
    const int64_t lim = (int64_t)1 << 31;
    const int64_t Ho = (int64_t)a->H * a->rep, Wo = (int64_t)a->W * a->rep;
    if (Ho >= lim || Wo >= lim || Ho * Wo >= lim || Ho * Wo * a->C >= lim) return GRL_ERR_BAD_ARG;
    const int64_t total = Ho * Wo * a->C * a->N;
    if (total >= lim) return GRL_ERR_BAD_ARG;
    const int64_t grid = ((total + 3) / 4 + NT - 1) / NT;
    if (grid > 0x7fffffff) return GRL_ERR_BAD_ARG;

    Params p;
    p.x = a->x; p.out = a->out;
    p.sn = a->stride[0]; p.sc = a->stride[1]; p.sh = a->stride[2]; p.sw = a->stride[3];
    p.Ho = (uint32_t)Ho; p.Wo = (uint32_t)Wo; p.total = (uint32_t)total;

    const hipStream_t st = (hipStream_t)stream;
    if (a->C == 1) launch<1>(a->rep, p, (unsigned)grid, st);
    else launch<3>(a->rep, p, (unsigned)grid, st);
    GRL_CHECK_LAUNCH();
    return 0;
}
