// K x K blur with scipy's ``mirror`` boundary on a list of images with per-item taps, sizes and stride (include/grl_hip.h,
// grl_blur_items): the ``ndimage.filters.convolve(img, np.expand_dims(k, axis=2), mode="mirror")`` calls of the reference's blind-SR
// degradation (utils/utils_bsr/utils_sisr.py:341-343, 359-362, 410-412) and the ``img[0::sf, 0::sf]`` that follows one of them, for
// every sample of a batch in one launch.
//
// Item list (item_list.h states the shared contract): the entry's slots are K, s, taps_off, 0.  The taps are K x K fp32 (row major,
// correlation order: the caller has flipped the kernel, as tasks.blur_taps does) at element taps_off of the taps buffer, the result
// is (C, ceil(h / s), ceil(w / s)):
//   out[oy][ox] = sum over ky = 0 .. K-1 (outer), kx = 0 .. K-1 (inner) of taps[ky][kx] * x[m(oy s - K/2 + ky, h)][m(ox s - K/2 + kx, w)]
//   m(i, n)     = scipy's mirror (reflect-101) folded as often as needed: n == 1 -> 0; else j = i mod 2(n-1); j >= n ? 2(n-1) - j : j
// one fp32 fmaf chain from 0 per output in that order (the determinism csrc/blur.hip promises): the result does not depend on the
// tiling, on the path below or on which other items share the launch.  Only the strided outputs are computed.
//
// Shape: the grid's second axis is items x channels; a workgroup of 256 threads owns one 16 x 16 output tile of one plane, a thread
// one output.  For s <= 4 the workgroup stages the ((16 - 1) s + K)^2 inputs its tile
// reads in LDS, already mirrored (at most 91 x 91 floats; the row pitch is the odd side), and the K x K taps next to them: an fmaf
// then reads one broadcast tap and one pixel from LDS.  A larger stride reads the pixels from global memory (the tile would not
// fit; the pipeline's strides are 1, 2 and 4).  The taps are checked against taps_elems as the images against the arenas, every
// pixel index is folded into the image, and an item whose K is even, below 1 or above the host's max_K is skipped.
#include "common.h"
#include "item_list.h"

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
    namespace il = item_list;
    const int64_t* it = il::row(p.items, item);
    const int64_t src_off = it[il::SRC_OFF], dst_off = it[il::DST_OFF], h64 = it[il::H], w64 = it[il::W];
    const int64_t K64 = it[il::SLOT], s64 = it[il::SLOT + 1], taps_off = it[il::SLOT + 2];
    // an item the buffers cannot hold, or with a size, K or stride out of range, is skipped whole (uniform over the workgroup)
    if (!il::side_ok(h64) || !il::side_ok(w64) || !il::side_ok(s64)) return;
    if (K64 < 1 || K64 > p.max_K || K64 > KMAX || !(K64 & 1)) return;
    const int h = (int)h64, w = (int)w64, K = (int)K64, s = (int)s64;
    const int ho = (h + s - 1) / s, wo = (w + s - 1) / s;
    if (!il::fits(src_off, p.C * h64 * w64, p.src_elems) || !il::fits(dst_off, (int64_t)p.C * ho * wo, p.dst_elems) ||
        !il::fits(taps_off, K * K, p.taps_elems))
        return;

    const il::Tile tl = il::tile_of_block(p.ntx, TS, TS);
    if (tl.surplus(ho, wo)) return;
    const int oy0 = tl.y0, ox0 = tl.x0;

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
    if (!a || (a->C != 1 && a->C != 3)) return GRL_ERR_BAD_ARG;
    item_list::Grid g;
    if (int e = item_list::check_tiled(*a, a->max_ho, a->max_wo, TS, TS, g, 1, a->C)) return e;   // grid.y is items x channels
    if (a->max_K < 1 || a->max_K > KMAX || a->max_K % 2 == 0) return GRL_ERR_BAD_ARG;
    if (!a->taps || (uintptr_t)a->taps % 4 || a->taps_elems <= 0) return GRL_ERR_BAD_ARG;

    Params p;
    p.src = a->src; p.dst = a->dst; p.taps = a->taps; p.items = a->items;
    p.src_elems = a->src_elems; p.dst_elems = a->dst_elems; p.taps_elems = a->taps_elems;
    p.C = a->C; p.max_K = a->max_K; p.ntx = g.ntx; p.nty = g.nty;
    hipLaunchKernelGGL(blur_items_kernel, dim3(g.tiles(), (unsigned)(a->n_items * a->C)), dim3(NT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
