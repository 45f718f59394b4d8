// Gradient-corrected linear demosaicking of an RGGB Bayer mosaic (include/grl_hip.h, grl_demosaic_matlab): the reference's
// ``dm_matlab`` (utils/utils_mosaic.py:36-111), which the engine applies to every demosaicking batch (engines/base.py:126-128).
//
// The mosaic comes as four packed planes (R at even rows / even columns, G at even / odd, G at odd / even, B at odd / odd), h x w
// each, that share one (batch, row, column) element-stride triple: the packed CFA4 tensor, or an RGB image read on that lattice.
// Full resolution is H = 2h, W = 2w.  The reference reflect-pads the full-resolution mosaic by 2 (torch "reflect": -1 -> 1, -2 -> 2,
// H -> H-2, H+1 -> H-3) and correlates it with four 5x5 filters, all scaled by 1/8 (utils_mosaic.py:44-86); with c(dy, dx) the
// mosaic around the pixel:
//   k0 (kgrb)   4 c + 2 (N1 + S1 + W1 + E1) - (N2 + S2 + W2 + E2)
//   k1 (krbg0)  5 c + 4 (W1 + E1) - (W2 + E2) - (the four diagonal neighbours) + (N2 + S2) / 2
//   k2 (krbg1)  k1 transposed: 5 c + 4 (N1 + S1) - (N2 + S2) - diagonals + (W2 + E2) / 2
//   k3 (krbbr)  6 c + 2 diagonals - 3/2 (N2 + S2 + W2 + E2)
// and fills the channels by the pixel's place in the 2x2 cell (utils_mosaic.py:97-109; native samples are copied):
//   (0, 0) R site: R = c,  G = k0, B = k3        (0, 1) G site: R = k1, G = c, B = k2
//   (1, 0) G site: R = k2, G = c,  B = k1        (1, 1) B site: R = k3, G = k0, B = c
//
// Arithmetic: every stencil is summed in fp64 and rounded once to fp32.  The weights are dyadic, so on 8-bit inputs (fp32 values of
// k / 255) every product and partial sum is exact in fp64: the result does not depend on the order of the sum and equals the
// reference's float64 run cast to fp32, bitwise.
//
// Shape: a workgroup of 256 threads owns TQY x TQX cells of one image.  It stages the four planes of those cells plus a one-cell halo
// in LDS (the reflection is resolved while loading: per plane, cell -1 and cell h / w map to fixed packed indices), then each thread
// forms whole cells -- 2 x 2 pixels x 3 channels -- and stores one float2 per channel and output row.  Partial edge tiles only load
// what exists and store only their own cells.
#include "common.h"

namespace {

constexpr int TQX = 64, TQY = 16, NT = 256;
constexpr int LX = TQX + 2, LY = TQY + 2;     // staged cells per plane, halo included
constexpr int ROWS_PER_THREAD = TQY / (NT / TQX);

struct Params {
    const float* plane[4];
    int64_t sb, sy, sx;
    int32_t h, w, ntx, nty;
    float* out;
};

// packed index of cell q (in -1 .. n) of a plane with parity `par` along that axis, after the full-resolution reflection by 2
__device__ __forceinline__ int reflect_cell(int q, int n, int par) {
    if (q < 0) return par ? 0 : 1;            // pixel -2 -> 2 (cell 1, even), pixel -1 -> 1 (cell 0, odd)
    if (q >= n) return par ? n - 2 : n - 1;   // pixel H -> H-2 (cell n-1, even), pixel H+1 -> H-3 (cell n-2, odd)
    return q;
}

__global__ __launch_bounds__(NT) void demosaic_matlab_kernel(Params p) {
    __shared__ float s[4][LY][LX];

    const int tiles = p.ntx * p.nty;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int qy0 = (t / p.ntx) * TQY, qx0 = (t % p.ntx) * TQX;

    for (int i = threadIdx.x; i < 4 * LY * LX; i += NT) {
        const int pl = i / (LY * LX), rem = i - pl * (LY * LX);
        const int r = rem / LX, c = rem - r * LX;
        const int gq = qy0 - 1 + r, gc = qx0 - 1 + c;
        float v = 0.f;
        if (gq <= p.h && gc <= p.w) {         // beyond the one-cell halo: no cell of this tile reads it
            const int yy = reflect_cell(gq, p.h, pl >> 1), xx = reflect_cell(gc, p.w, pl & 1);
            v = p.plane[pl][b * p.sb + yy * p.sy + xx * p.sx];
        }
        s[pl][r][c] = v;
    }
    __syncthreads();

    const int lx = threadIdx.x % TQX;
    const int qx = qx0 + lx;
    if (qx >= p.w) return;
    const int64_t W = 2 * (int64_t)p.w, plane_px = 2 * (int64_t)p.h * W;
    float* const out_b = p.out + (int64_t)b * 3 * plane_px;

    for (int k = 0; k < ROWS_PER_THREAD; ++k) {
        const int ly = threadIdx.x / TQX + k * (NT / TQX);
        const int qy = qy0 + ly;
        if (qy >= p.h) break;
        // c(u, v): the mosaic at full-resolution offset (u, v) from the cell's top-left pixel, u, v in -2 .. 3
        auto c = [&](int u, int v) -> double {
            const int uu = u + 2, vv = v + 2;
            return (double)s[((uu & 1) << 1) | (vv & 1)][ly + (uu >> 1)][lx + (vv >> 1)];
        };
        auto k0 = [&](int u, int v) {
            return 0.125 * (4.0 * c(u, v) + 2.0 * (c(u - 1, v) + c(u + 1, v) + c(u, v - 1) + c(u, v + 1))
                            - (c(u - 2, v) + c(u + 2, v) + c(u, v - 2) + c(u, v + 2)));
        };
        auto diag = [&](int u, int v) { return c(u - 1, v - 1) + c(u - 1, v + 1) + c(u + 1, v - 1) + c(u + 1, v + 1); };
        auto k1 = [&](int u, int v) {
            return 0.125 * (5.0 * c(u, v) + 4.0 * (c(u, v - 1) + c(u, v + 1)) - (c(u, v - 2) + c(u, v + 2)) - diag(u, v)
                            + 0.5 * (c(u - 2, v) + c(u + 2, v)));
        };
        auto k2 = [&](int u, int v) {
            return 0.125 * (5.0 * c(u, v) + 4.0 * (c(u - 1, v) + c(u + 1, v)) - (c(u - 2, v) + c(u + 2, v)) - diag(u, v)
                            + 0.5 * (c(u, v - 2) + c(u, v + 2)));
        };
        auto k3 = [&](int u, int v) {
            return 0.125 * (6.0 * c(u, v) + 2.0 * diag(u, v) - 1.5 * (c(u - 2, v) + c(u + 2, v) + c(u, v - 2) + c(u, v + 2)));
        };
        const float r00 = s[0][ly + 1][lx + 1], g01 = s[1][ly + 1][lx + 1], g10 = s[2][ly + 1][lx + 1], b11 = s[3][ly + 1][lx + 1];
        const float2 R0 = make_float2(r00, (float)k1(0, 1)), R1 = make_float2((float)k2(1, 0), (float)k3(1, 1));
        const float2 G0 = make_float2((float)k0(0, 0), g01), G1 = make_float2(g10, (float)k0(1, 1));
        const float2 B0 = make_float2((float)k3(0, 0), (float)k2(0, 1)), B1 = make_float2((float)k1(1, 0), b11);

        float* o = out_b + (2 * (int64_t)qy) * W + 2 * (int64_t)qx;
        *reinterpret_cast<float2*>(o) = R0;
        *reinterpret_cast<float2*>(o + W) = R1;
        o += plane_px;
        *reinterpret_cast<float2*>(o) = G0;
        *reinterpret_cast<float2*>(o + W) = G1;
        o += plane_px;
        *reinterpret_cast<float2*>(o) = B0;
        *reinterpret_cast<float2*>(o + W) = B1;
    }
}

}  // namespace

extern "C" int grl_demosaic_matlab(void* stream, const GrlDemosaicArgs* a) {
    if (!a || !a->out) return GRL_ERR_BAD_ARG;
    for (int i = 0; i < 4; ++i)
        if (!a->plane[i]) return GRL_ERR_BAD_ARG;
    const int32_t N = a->N, h = a->h, w = a->w;
    if (N <= 0 || h < 2 || w < 2) return GRL_ERR_BAD_ARG;     // the reflection by 2 needs at least 4 pixels per side
    if ((uint64_t)a->out % 8) return GRL_ERR_BAD_ARG;         // float2 stores
    const int32_t ntx = (w + TQX - 1) / TQX, nty = (h + TQY - 1) / TQY;
    const int64_t grid = (int64_t)N * ntx * nty;
    if (grid > 0x7fffffff) return GRL_ERR_BAD_ARG;

    Params p;
    for (int i = 0; i < 4; ++i) p.plane[i] = a->plane[i];
    p.sb = a->stride[0]; p.sy = a->stride[1]; p.sx = a->stride[2];
    p.h = h; p.w = w; p.ntx = ntx; p.nty = nty;
    p.out = a->out;
    hipLaunchKernelGGL(demosaic_matlab_kernel, dim3((unsigned)grid), dim3(NT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
