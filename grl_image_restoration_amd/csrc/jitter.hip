// The colour jitter of the blind-SR training branch on a list of images (include/grl_hip.h, grl_color_jitter): torchvision's
// ``ColorJitter.forward`` on float RGB in [0, 1] -- adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue in a drawn
// order -- as the reference applies it to every GT crop (data/datasets/restoration_bsr.py:66-68,100), for a whole batch in one call.
//
// Item list (item_list.h states the shared contract): the entry's slots are the four ops in the order they run (0 brightness,
// 1 contrast, 2 saturation, 3 hue), and every item has a record of four floats in `params`: b, c, s, h.  The arithmetic is
// stated in the header; all of it is fp32 but the sum behind the contrast mean, which is fp64 from the pixel on.
//
// Shape.  The three planes of an image are contiguous, so the image is walked as n = h * w pixels: rows follow each other in
// memory, and a wave reads 64 (or 256) consecutive pixels of each plane.  A workgroup of 256 threads owns SPAN = 4096 consecutive
// pixels (the grid's first axis counts such spans, not tiles), and the op order is uniform over a workgroup.  Where n, both
// offsets and both arena pointers are multiples of 4 elements a thread moves float4s (4 steps of 1024 pixels per workgroup, all
// twelve loads in flight before the first chain starts), else scalars (16 steps of 256).  The contrast mean needs the whole image as it stands
// when contrast runs, so the entry is two launches: pass 1 walks the ops that precede contrast and sums gray(x) -- per thread,
// over the wave by shuffles, over the four waves through LDS -- into one fp64 partial per (item, workgroup); pass 2 adds the
// item's partials in a fixed order (every workgroup the same way: a strided sum per thread, then the same wave / LDS tree),
// workgroup 0 writes the mean, and every thread walks the whole chain for its pixels, reading a pixel's three channels before it
// writes them.  No atomics: the result of an item is a function of its own record, its pixels and the alignment of its planes.
// An item with more pixels than the grid has workgroups for (and the partial buffer slots) is skipped like one that does not fit.
#include <math.h>

#include "common.h"
#include "item_list.h"

namespace {

constexpr int NT = 256, WAVES = NT / 64, SPAN = 4096;
constexpr int OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3;

struct Params {
    const float* src;
    float* dst;
    const int64_t* items;
    const float* params;
    double* partial;
    double* means;
    int64_t src_elems, dst_elems;
    int32_t nwg;
};

struct Item {
    int64_t src_off, dst_off, n;
    float b, c, s, h;
    int order;                                       // op k in bits 2k, 2k + 1
    bool vec_src, vec_dst;
};

// an item the buffers cannot hold, with a side out of range, with an order that is no permutation, or with more pixels than the
// grid has workgroups for, is skipped whole (uniform over the workgroup)
__device__ __forceinline__ bool load_item(const Params& p, int item, Item& it) {
    namespace il = item_list;
    const int64_t* t = il::row(p.items, item);
    const int64_t src_off = t[il::SRC_OFF], dst_off = t[il::DST_OFF], h = t[il::H], w = t[il::W];
    if (!il::side_ok(h) || !il::side_ok(w)) return false;
    const int64_t n = h * w;
    if (!il::fits(src_off, 3 * n, p.src_elems) || !il::fits(dst_off, 3 * n, p.dst_elems)) return false;
    if ((n + SPAN - 1) / SPAN > p.nwg) return false;
    int order = 0, seen = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t op = t[il::SLOT + k];
        if (op < 0 || op > 3) return false;
        order |= (int)op << (2 * k);
        seen |= 1 << (int)op;
    }
    if (seen != 15) return false;
    const float* rec = p.params + 4 * (int64_t)item;
    it.src_off = src_off; it.dst_off = dst_off; it.n = n; it.order = order;
    it.b = rec[0]; it.c = rec[1]; it.s = rec[2]; it.h = rec[3];
    it.vec_src = n % 4 == 0 && src_off % 4 == 0 && (uintptr_t)p.src % 16 == 0;
    it.vec_dst = it.vec_src && dst_off % 4 == 0 && (uintptr_t)p.dst % 16 == 0;
    return true;
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }   // NaN -> 0

__device__ __forceinline__ float gray(const float x[3]) { return (0.2989f * x[0] + 0.587f * x[1]) + 0.114f * x[2]; }

__device__ __forceinline__ float blend(float x, float y, float f) { return clamp01(f * x + (1.0f - f) * y); }

// fmod(x, 1) of a finite x: x - trunc(x) is exact and has the sign of x (libm's fmodf is a loop)
__device__ __forceinline__ float frac_part(float x) { return x - truncf(x); }

// adjust_hue: _rgb2hsv, the shift, _hsv2rgb
__device__ __forceinline__ void hue(float x[3], float shift) {
    const float r = x[0], g = x[1], b = x[2];
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float S = cr / (eq ? 1.0f : maxc), d = eq ? 1.0f : cr;
    const float rc = (maxc - r) / d, gc = (maxc - g) / d, bc = (maxc - b) / d;
    float H = maxc == r ? bc - gc : (maxc == g ? (2.0f + rc) - bc : (4.0f + gc) - rc);
    H = frac_part(H / 6.0f + 1.0f);
    H = frac_part(H + shift);                         // torch.remainder: fmod, then the sign of the divisor
    if (H < 0.0f) H += 1.0f;
    const float V = maxc, H6 = H * 6.0f, fl = floorf(H6), f = H6 - fl;
    const float pp = clamp01(V * (1.0f - S)), q = clamp01(V * (1.0f - S * f)), t = clamp01(V * (1.0f - S * (1.0f - f)));
    int i = (int)fl;                                  // 0 .. 6; 6 when the remainder rounded to 1
    i = i >= 6 ? i - 6 : i;
    x[0] = i == 0 || i == 5 ? V : (i == 1 ? q : (i == 4 ? t : pp));
    x[1] = i == 1 || i == 2 ? V : (i == 0 ? t : (i == 3 ? q : pp));
    x[2] = i == 3 || i == 4 ? V : (i == 2 ? t : (i == 5 ? q : pp));
}

// the chain on one pixel.  FIRST: only the ops that precede contrast (pass 1); else all of it with the mean `m`
template <bool FIRST>
__device__ __forceinline__ void chain(const Item& it, float x[3], float m) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = (it.order >> (2 * k)) & 3;     // uniform over the workgroup
        if (op == OP_BRIGHTNESS) {
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = blend(x[c], 0.0f, it.b);
        } else if (op == OP_CONTRAST) {
            if (FIRST) return;
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = blend(x[c], m, it.c);
        } else if (op == OP_SATURATION) {
            const float y = gray(x);
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = blend(x[c], y, it.s);
        } else {
            hue(x, it.h);
        }
    }
}

// the sum of `v` over the workgroup, in a fixed order, in every thread; a kernel calls it once (wave_sums is not reused)
__device__ __forceinline__ double block_sum(double v, double* wave_sums) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
    __syncthreads();
    double d = wave_sums[0];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) d += wave_sums[k];
    return d;
}

// PASS 1: returns the thread's sum of gray over its pixels after the ops that precede contrast.  PASS 2: the whole chain, stored.
template <bool FIRST>
__device__ __forceinline__ double walk(const Params& p, const Item& it, float m) {
    const float* s = p.src + it.src_off;
    float* d = p.dst + it.dst_off;
    const int64_t n = it.n, base = (int64_t)blockIdx.x * SPAN;
    double acc = 0.0;
    if (FIRST ? it.vec_src : it.vec_dst) {
        constexpr int Q = SPAN / (4 * NT);
        float4 rr[Q], gg[Q], bb[Q];                    // all of the thread's loads are in flight before the first chain starts
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int64_t i = base + 4 * (q * NT + (int64_t)threadIdx.x);
            if (i < n) {
                rr[q] = *(const float4*)(s + i); gg[q] = *(const float4*)(s + n + i); bb[q] = *(const float4*)(s + 2 * n + i);
            }
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int64_t i = base + 4 * (q * NT + (int64_t)threadIdx.x);
            if (i >= n) break;
            const float4 r = rr[q], g = gg[q], b = bb[q];
            float px[4][3] = {{r.x, g.x, b.x}, {r.y, g.y, b.y}, {r.z, g.z, b.z}, {r.w, g.w, b.w}};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                chain<FIRST>(it, px[j], m);
                if (FIRST) acc += (double)gray(px[j]);
            }
            if (!FIRST) {
                *(float4*)(d + i) = float4{px[0][0], px[1][0], px[2][0], px[3][0]};
                *(float4*)(d + n + i) = float4{px[0][1], px[1][1], px[2][1], px[3][1]};
                *(float4*)(d + 2 * n + i) = float4{px[0][2], px[1][2], px[2][2], px[3][2]};
            }
        }
    } else {
        for (int q = 0; q < SPAN / NT; ++q) {
            const int64_t i = base + q * NT + threadIdx.x;
            if (i >= n) break;
            float px[3] = {s[i], s[n + i], s[2 * n + i]};
            chain<FIRST>(it, px, m);
            if (FIRST) {
                acc += (double)gray(px);
            } else {
                d[i] = px[0]; d[n + i] = px[1]; d[2 * n + i] = px[2];
            }
        }
    }
    return acc;
}

__global__ __launch_bounds__(NT) void jitter_sum_kernel(Params p) {
    __shared__ double wave_sums[WAVES];
    Item it;
    if (!load_item(p, blockIdx.y, it)) return;
    if ((int64_t)blockIdx.x * SPAN >= it.n) return;  // a surplus workgroup of a smaller item
    const double d = block_sum(walk<true>(p, it, 0.0f), wave_sums);
    if (threadIdx.x == 0) p.partial[(int64_t)blockIdx.y * p.nwg + blockIdx.x] = d;
}

__global__ __launch_bounds__(NT) void jitter_apply_kernel(Params p) {
    __shared__ double wave_sums[WAVES];
    Item it;
    if (!load_item(p, blockIdx.y, it)) return;
    if ((int64_t)blockIdx.x * SPAN >= it.n) return;
    const int count = (int)((it.n + SPAN - 1) / SPAN);   // at most nwg: load_item
    const double* part = p.partial + (int64_t)blockIdx.y * p.nwg;
    double v = 0.0;
    for (int k = threadIdx.x; k < count; k += NT) v += part[k];
    const double mean = block_sum(v, wave_sums) / (double)it.n;
    if (blockIdx.x == 0 && threadIdx.x == 0) p.means[blockIdx.y] = mean;
    walk<false>(p, it, (float)mean);
}

int64_t workgroups(int64_t max_h, int64_t max_w) {
    if (!item_list::side_ok(max_h) || !item_list::side_ok(max_w)) return GRL_ERR_BAD_ARG;
    return (max_h * max_w + SPAN - 1) / SPAN;          // at most 2^28
}

}  // namespace

extern "C" int grl_color_jitter_num_workgroups(int32_t max_h, int32_t max_w) { return (int)workgroups(max_h, max_w); }

extern "C" int grl_color_jitter(void* stream, const GrlColorJitterArgs* a) {
    if (!a || a->C != 3) return GRL_ERR_BAD_ARG;
    if (int e = item_list::check_args(*a, a->max_h, a->max_w)) return e;
    if (!a->params || !a->partial || !a->means) return GRL_ERR_BAD_ARG;
    const int64_t nwg = workgroups(a->max_h, a->max_w);
    if (a->n_partial < nwg * a->n_items) return GRL_ERR_BAD_ARG;
    if ((uintptr_t)a->params % 4 || (uintptr_t)a->partial % 8 || (uintptr_t)a->means % 8) return GRL_ERR_BAD_ARG;
    Params p;
    p.src = a->src; p.dst = a->dst; p.items = a->items; p.params = a->params; p.partial = a->partial; p.means = a->means;
    p.src_elems = a->src_elems; p.dst_elems = a->dst_elems; p.nwg = (int32_t)nwg;
    const dim3 grid((unsigned)nwg, (unsigned)a->n_items);
    hipLaunchKernelGGL(jitter_sum_kernel, grid, dim3(NT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(jitter_apply_kernel, grid, dim3(NT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
