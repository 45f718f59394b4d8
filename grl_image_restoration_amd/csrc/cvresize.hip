// OpenCV's resize (INTER_LINEAR, INTER_CUBIC, INTER_AREA) on a list of images whose sizes differ (include/grl_hip.h,
// grl_cv_resize): the ``cv2.resize(img, (wo, ho), interpolation=random.choice([1, 2, 3]))`` calls of the reference's blind-SR
// degradation (utils/utils_bsr/utils_sisr.py:299-303, 350-354, 416-420), for every sample of a batch in one launch.
//
// Item list (item_list.h states the shared contract): the entry's slots are ho, wo, interp, 0; (C, h, w) -> (C, ho, wo).  Per axis, with scale = n / no, coordinates and weights in float64, every weight rounded once to fp32:
//   linear  f = (d + 0.5) scale - 0.5, i = floor(f), t = f - i; i < 0: i = 0, t = 0; i >= n - 1: i = n - 1, t = 0; taps i, i + 1
//           with 1 - t, t
//   cubic   the same f, i, t without the clamps of t; taps i - 1 .. i + 2 with OpenCV's A = -0.75 coefficients
//   area    scale_x >= 1 and scale_y >= 1: the coverage table of computeResizeAreaTab -- f1 = d scale, f2 = f1 + scale,
//           cell = min(scale, n - f1), s1 = ceil(f1), s2 = min(floor(f2), n - 1), s1 = min(s1, s2); (s1 - f1) / cell on s1 - 1 if
//           s1 - f1 > 1e-3, 1 / cell on s1 .. s2 - 1, min(min(f2 - s2, 1), cell) / cell on s2 if f2 - s2 > 1e-3
//           otherwise (an upscale on either axis): the linear taps with i = floor(d scale), t = (d + 1) - (i + 1) / scale,
//           t = 0 if t <= 0 else t - floor(t), on both axes
// Tap indices outside the image clamp to the edge.  An output is
//   out[oy][ox] = chain_ky wy[ky] * fl32(chain_kx wx[kx] * src[iy(ky)][ix(kx)])
// each chain one fp32 fmaf chain from 0 in ascending tap order: the horizontal pass first, then the vertical one, as OpenCV.  This
// is OpenCV's sampling rule with float64 coordinates; OpenCV rounds the coordinate to fp32 first, which moves a weight by up to
// n * 2^-24, so equality with OpenCV's bytes is not claimed.
//
// Shape: a workgroup of 256 threads owns a 16 x 16 output tile of one item, a thread one output position for all channels.  The taps
// of a thread are three numbers per axis (first index, count, and the weights: four explicit ones for linear / cubic, or the
// left / middle / right weight of the area table), computed once per thread.  The images are small (at most 3 x 400 x 400 in the
// pipeline) and stay in L2; the design point is many small items in one launch.  An item's result depends on nothing but the item.
#include "common.h"
#include "item_list.h"

namespace {

constexpr int TS = 16, NT = TS * TS;

struct Params {
    const float* src;
    float* dst;
    const int64_t* items;
    int64_t src_elems, dst_elems;
    int32_t C, ntx, nty;
};

// The taps of output index d on one axis: source indices first .. first + cnt - 1 (clamped by the caller).  cnt <= 4: weights w0 .. w3;
// area table (table = true): wl on the first tap if left, wr on the last if right, wm on every other one.
struct Taps {
    int first, cnt;
    bool table, left, right;
    float w0, w1, w2, w3;
    float wl, wm, wr;
};

enum { M_LINEAR = 0, M_CUBIC = 1, M_AREA_TABLE = 2, M_AREA_LINEAR = 3 };

__device__ __forceinline__ Taps make_taps(int mode, int n, int no, int d) {
#pragma clang fp contract(off)          // the float64 coordinates are the stated expressions, operation by operation
    Taps t;
    t.table = mode == M_AREA_TABLE;
    t.left = t.right = false;
    t.wl = t.wm = t.wr = 0.f;
    t.w0 = t.w1 = t.w2 = t.w3 = 0.f;
    const double scale = (double)n / (double)no;
    if (mode == M_AREA_TABLE) {
        const double f1 = d * scale, f2 = f1 + scale;
        const double cell = fmin(scale, (double)n - f1);
        int s1 = (int)ceil(f1), s2 = (int)floor(f2);
        s2 = min(s2, n - 1);
        s1 = min(s1, s2);
        t.left = (double)s1 - f1 > 1e-3;
        t.right = f2 - (double)s2 > 1e-3;
        t.wl = (float)(((double)s1 - f1) / cell);
        t.wm = (float)(1.0 / cell);
        t.wr = (float)(fmin(fmin(f2 - (double)s2, 1.0), cell) / cell);
        t.first = s1 - (t.left ? 1 : 0);
        t.cnt = (t.left ? 1 : 0) + (s2 - s1) + (t.right ? 1 : 0);
    } else {
        int i;
        double u;
        if (mode == M_AREA_LINEAR) {
            i = (int)floor(d * scale);
            u = (double)(d + 1) - (double)(i + 1) / scale;
            u = u <= 0.0 ? 0.0 : u - floor(u);
        } else {
            const double f = ((double)d + 0.5) * scale - 0.5;
            const double fl = floor(f);
            i = (int)fl;
            u = f - fl;
        }
        if (mode == M_CUBIC) {
            const double A = -0.75;
            const double c0 = ((A * (u + 1) - 5 * A) * (u + 1) + 8 * A) * (u + 1) - 4 * A;
            const double c1 = ((A + 2) * u - (A + 3)) * u * u + 1;
            const double v = 1 - u;
            const double c2 = ((A + 2) * v - (A + 3)) * v * v + 1;
            t.first = i - 1; t.cnt = 4;
            t.w0 = (float)c0; t.w1 = (float)c1; t.w2 = (float)c2; t.w3 = (float)(1.0 - c0 - c1 - c2);
        } else {
            if (i < 0) { i = 0; u = 0.0; }
            if (i >= n - 1) { i = n - 1; u = 0.0; }
            t.first = i; t.cnt = 2;
            t.w0 = (float)(1.0 - u); t.w1 = (float)u;
        }
    }
    return t;
}

// chain_k w[k] * f(first + k) over the taps of one axis: an fp32 fmaf chain from 0 in ascending tap order.  The two or four explicit
// weights are written out and the area table's left / middle / right runs are separate (a weight picked per tap turns the struct into an indexed array in memory).
template <class F>
__device__ __forceinline__ float tap_chain(const Taps& t, F f) {
    float r = 0.f;
    if (!t.table) {
        r = fmaf(t.w0, f(t.first), r);
        r = fmaf(t.w1, f(t.first + 1), r);
        if (t.cnt == 4) {
            r = fmaf(t.w2, f(t.first + 2), r);
            r = fmaf(t.w3, f(t.first + 3), r);
        }
        return r;
    }
    int k = 0;
    const int mid_end = t.cnt - (t.right ? 1 : 0);
    if (t.left) r = fmaf(t.wl, f(t.first + k++), r);
    for (; k < mid_end; ++k) r = fmaf(t.wm, f(t.first + k), r);
    if (t.right) r = fmaf(t.wr, f(t.first + k), r);
    return r;
}

__global__ __launch_bounds__(NT) void cv_resize_kernel(Params p) {
    namespace il = item_list;
    const int64_t* it = il::row(p.items, blockIdx.y);
    const int64_t src_off = it[il::SRC_OFF], dst_off = it[il::DST_OFF], h64 = it[il::H], w64 = it[il::W];
    const int64_t ho64 = it[il::SLOT], wo64 = it[il::SLOT + 1], interp = it[il::SLOT + 2];
    // an item the arenas cannot hold, or with sizes / a mode out of range, is skipped whole (wave-uniform: the item is per workgroup)
    if (!il::side_ok(h64) || !il::side_ok(w64) || !il::side_ok(ho64) || !il::side_ok(wo64)) return;
    if (interp < 1 || interp > 3) return;
    if (!il::fits(src_off, p.C * h64 * w64, p.src_elems) || !il::fits(dst_off, p.C * ho64 * wo64, p.dst_elems)) return;
    const int h = (int)h64, w = (int)w64, ho = (int)ho64, wo = (int)wo64;

    const il::Tile tile = il::tile_of_block(p.ntx, TS, TS);
    if (tile.surplus(ho, wo)) return;
    const int oy = tile.y0 + threadIdx.x / TS, ox = tile.x0 + threadIdx.x % TS;
    if (oy >= ho || ox >= wo) return;

    int my, mx;
    if (interp == 1) my = mx = M_LINEAR;
    else if (interp == 2) my = mx = M_CUBIC;
    else my = mx = (h >= ho && w >= wo) ? M_AREA_TABLE : M_AREA_LINEAR;
    const Taps ty_ = make_taps(my, h, ho, oy), tx_ = make_taps(mx, w, wo, ox);

    const float* s = p.src + src_off;
    float* d = p.dst + dst_off + (int64_t)oy * wo + ox;
    for (int c = 0; c < p.C; ++c, s += (int64_t)h * w, d += (int64_t)ho * wo) {
        *d = tap_chain(ty_, [&](int y) {
            const float* row = s + (int64_t)min(max(y, 0), h - 1) * w;
            return tap_chain(tx_, [&](int x) { return row[min(max(x, 0), w - 1)]; });
        });
    }
}

}  // namespace

extern "C" int grl_cv_resize(void* stream, const GrlCvResizeArgs* a) {
    if (!a || (a->C != 1 && a->C != 3)) return GRL_ERR_BAD_ARG;
    item_list::Grid g;
    if (int e = item_list::check_tiled(*a, a->max_ho, a->max_wo, TS, TS, g)) return e;

    Params p;
    p.src = a->src; p.dst = a->dst; p.items = a->items; p.src_elems = a->src_elems; p.dst_elems = a->dst_elems;
    p.C = a->C; p.ntx = g.ntx; p.nty = g.nty;
    hipLaunchKernelGGL(cv_resize_kernel, dim3(g.tiles(), (unsigned)a->n_items), dim3(NT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
