// K x K blur with scipy's ``mirror`` boundary on a list of images with per-item taps, sizes and stride (include/grl_hip.h,
// grl_blur_items): the ``ndimage.filters.convolve(img, np.expand_dims(k, axis=2), mode="mirror")`` calls of the reference's blind-SR
// degradation (utils/utils_bsr/utils_sisr.py:341-343, 359-362, 410-412) and the ``img[0::sf, 0::sf]`` that follows one of them, for
// every sample of a batch in one launch.
//
// Item list (device memory, read by the kernel): per item eight int64 -- src_off, dst_off, h, w, K, s, taps_off, 0.  The source is
// contiguous fp32 (C, h, w) at element src_off of the source arena, the taps K x K fp32 (row major, correlation order: the caller
// has flipped the kernel, as tasks.blur_taps does) at element taps_off of the taps buffer, the result contiguous
// (C, ceil(h / s), ceil(w / s)) at dst_off of the destination arena:
//   out[oy][ox] = sum over ky = 0 .. K-1 (outer), kx = 0 .. K-1 (inner) of taps[ky][kx] * x[m(oy s - K/2 + ky, h)][m(ox s - K/2 + kx, w)]
//   m(i, n)     = scipy's mirror (reflect-101) folded as often as needed: n == 1 -> 0; else j = i mod 2(n-1); j >= n ? 2(n-1) - j : j
// one fp32 fmaf chain from 0 per output in that order (the determinism csrc/blur.hip promises): the result does not depend on the
// tiling, on the path below or on which other items share the launch.  Only the strided outputs are computed.
//
// Shape: the grid is (16 x 16 output tiles of the largest output the host vouches for) x (items x channels); a workgroup of 256
// threads owns one tile of one plane, a thread one output.  For s <= 4 the workgroup stages the ((16 - 1) s + K)^2 inputs its tile
// reads in LDS, already mirrored (at most 91 x 91 floats; the row pitch is the odd side), and the K x K taps next to them: an fmaf
// then reads one broadcast tap and one pixel from LDS.  A larger stride reads the pixels from global memory (the tile would not
// fit; the pipeline's strides are 1, 2 and 4).  Every item is checked against the arena and taps lengths before anything is read or
// written, every pixel index is folded into the image, and an item whose K is even, below 1 or above the host's max_K is skipped:
// no list content can make the kernel touch memory outside the buffers.
#include "common.h"

namespace {

constexpr int TS = 16, NT = TS * TS, KMAX = 31, SMAX = 4, SIDE_MAX = (TS - 1) * SMAX + KMAX;

struct Params {
    const float* src;
    float* dst;
    const float* taps;
    const int64_t* items;
    int64_t src_elems, dst_elems, taps_elems;
    int32_t C, max_K, ntx, nty;
};

__device__ __forceinline__ int mirror(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int j = i % p;
    if (j < 0) j += p;
    return j >= n ? p - j : j;
}

__global__ __launch_bounds__(NT) void blur_items_kernel(Params p) {
    __shared__ float tile[SIDE_MAX * SIDE_MAX];
    __shared__ float tp[KMAX * KMAX];

    const int item = blockIdx.y / p.C, c = blockIdx.y - item * p.C;
    const int64_t* it = p.items + 8 * (int64_t)item;
    const int64_t src_off = it[0], dst_off = it[1], h64 = it[2], w64 = it[3], K64 = it[4], s64 = it[5], taps_off = it[6];
    // an item the buffers cannot hold, or with a size, K or stride out of range, is skipped whole (uniform over the workgroup)
    if (h64 < 1 || w64 < 1 || h64 > (1 << 20) || w64 > (1 << 20) || s64 < 1 || s64 > (1 << 20)) return;
    if (K64 < 1 || K64 > p.max_K || K64 > KMAX || !(K64 & 1)) return;
    const int h = (int)h64, w = (int)w64, K = (int)K64, s = (int)s64;
    const int ho = (h + s - 1) / s, wo = (w + s - 1) / s;
    if (src_off < 0 || dst_off < 0 || taps_off < 0 || src_off + p.C * h64 * w64 > p.src_elems ||
        dst_off + (int64_t)p.C * ho * wo > p.dst_elems || taps_off + K * K > p.taps_elems)
        return;

    const int tyb = blockIdx.x / p.ntx, txb = blockIdx.x - tyb * p.ntx;
    const int oy0 = tyb * TS, ox0 = txb * TS;
    if (oy0 >= ho || ox0 >= wo) return;                               // a surplus workgroup of a smaller item

    const float* const x = p.src + src_off + (int64_t)c * h * w;
    const float* const t = p.taps + taps_off;
    const int ly = threadIdx.x / TS, lx = threadIdx.x % TS;
    const int oy = oy0 + ly, ox = ox0 + lx;
    const int half = K / 2;
    const bool staged = s <= SMAX;                                    // uniform over the workgroup
    float acc = 0.f;

    if (staged) {
        const int side = (TS - 1) * s + K;
        for (int i = threadIdx.x; i < K * K; i += NT) tp[i] = t[i];
        for (int r = ly; r < side; r += TS) {
            const float* row = x + (int64_t)mirror(oy0 * s - half + r, h) * w;
            for (int q = lx; q < side; q += TS) tile[r * side + q] = row[mirror(ox0 * s - half + q, w)];
        }
        __syncthreads();
        if (oy >= ho || ox >= wo) return;
        const float* px = tile + ly * s * side + lx * s;
        const float* pt = tp;
        for (int ky = 0; ky < K; ++ky, px += side, pt += K)
            for (int kx = 0; kx < K; ++kx) acc = fmaf(pt[kx], px[kx], acc);
    } else {
        if (oy >= ho || ox >= wo) return;
        for (int ky = 0; ky < K; ++ky) {
            const float* row = x + (int64_t)mirror(oy * s - half + ky, h) * w;
            for (int kx = 0; kx < K; ++kx) acc = fmaf(t[ky * K + kx], row[mirror(ox * s - half + kx, w)], acc);
        }
    }
    p.dst[dst_off + ((int64_t)c * ho + oy) * wo + ox] = acc;
}

}  // namespace

extern "C" int grl_blur_items(void* stream, const GrlBlurItemsArgs* a) {
    if (!a || !a->src || !a->dst || !a->taps || !a->items) return GRL_ERR_BAD_ARG;
    if (a->C != 1 && a->C != 3) return GRL_ERR_BAD_ARG;
    if (a->max_K < 1 || a->max_K > KMAX || a->max_K % 2 == 0) return GRL_ERR_BAD_ARG;
    if (a->n_items <= 0 || a->max_ho <= 0 || a->max_wo <= 0 || a->src_elems <= 0 || a->dst_elems <= 0 || a->taps_elems <= 0)
        return GRL_ERR_BAD_ARG;
    if (a->max_ho > (1 << 20) || a->max_wo > (1 << 20) || (int64_t)a->n_items * a->C > 65535) return GRL_ERR_BAD_ARG;
    if ((uint64_t)a->src % 4 || (uint64_t)a->dst % 4 || (uint64_t)a->taps % 4 || (uint64_t)a->items % 8) return GRL_ERR_BAD_ARG;
    const int64_t ntx = (a->max_wo + TS - 1) / TS, nty = (a->max_ho + TS - 1) / TS;
    if (ntx * nty > 0x7fffffff) return GRL_ERR_BAD_ARG;

    Params p;
    p.src = a->src; p.dst = a->dst; p.taps = a->taps; p.items = a->items;
    p.src_elems = a->src_elems; p.dst_elems = a->dst_elems; p.taps_elems = a->taps_elems;
    p.C = a->C; p.max_K = a->max_K; p.ntx = (int32_t)ntx; p.nty = (int32_t)nty;
    hipLaunchKernelGGL(blur_items_kernel, dim3((unsigned)(ntx * nty), (unsigned)(a->n_items * a->C)), dim3(NT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
