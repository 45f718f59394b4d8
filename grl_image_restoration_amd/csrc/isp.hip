// The camera-noise stage of the blind-SR degradation on a list of images (include/grl_hip.h, grl_isp_unprocess / grl_isp_process /
// grl_isp_roundtrip): stage 2 of the reference's ``degradation_sr2`` (utils/utils_bsr/utils_sisr.py:365-370), i.e.
// ``ISPModel.forward`` (utils/utils_bsr/utils_isp.py:539-543) -- ``ISPNet.reverse`` (445-454), the shot / read noise of
// utils_noise.py:95-103, ``ISPNet.forward`` (431-443) with the Malvar ``Demosaic`` (215-292) -- for every acting sample of a batch
// in one launch per entry.
//
// Item list (item_list.h states the shared contract): the entries' slots are yi_off, yi_inv_off, z_off, 0, and every item has
// a record of REC = 40 floats in `params`: W1i, W2i, W2, W1 (3 x 3 each, row major), 2^e, 2^-e, shot, read.  The arithmetic of every
// step is stated in the header.  All of it is fp32; clamp is to [0, 1] and sends NaN to 0, so every table index lies in the table.
//
// Shape.  The two per-pixel kernels (unprocess, roundtrip) give a thread one pixel of a 64 x 4 tile: it reads the three channels
// (row-contiguous over the wave), walks the colour chain once and writes one raw value (unprocess: only the row of W2i its lattice
// position keeps) or three.  The demosaic kernel (process) gives a workgroup of 256 threads a 32 x 32 pixel tile: the raw tile with
// its 2-pixel halo is staged in LDS already reflected (36 x 36 floats, pitch 37), a thread owns one 2 x 2 lattice quad -- so every
// lane runs the same four stencils and no wave diverges on pixel parity --, walks the colour chain for its four pixels and parks
// the twelve results in a second LDS image (3 x 32 x 33), from which the workgroup stores rows of 32 contiguous floats, leaving out
// the pixels an odd border does not have.  The tone tables and the normals are checked against tables_elems / normals_elems as
// the images against the arenas, and every pixel index is folded into the image.
#include <math.h>

#include "common.h"
#include "item_list.h"

namespace {

constexpr int NT = 256, PW = 64, PH = 4;                                   // per-pixel kernels: 64 x 4 pixels per workgroup
constexpr int QT = 16, TP = 2 * QT, SIDE = TP + 4, PITCH = SIDE + 1;       // demosaic: 16 x 16 quads, 36 x 36 staged
constexpr int OPITCH = TP + 1;
constexpr int REC = 40, TABLE_N = 1000001, MIN_SIDE = 3;                    // the demosaic reflects by 2
constexpr int W1I = 0, W2I = 9, W2 = 18, W1 = 27, P2E = 36, SHOT = 38, READ = 39;

struct Params {
    const float* src;
    float* dst;
    const int64_t* items;
    const float* params;
    const float* tables;
    const float* normals;
    int64_t src_elems, dst_elems, tables_elems, normals_elems;
    int32_t ntx, nty;
};

struct Item {
    int64_t src_off, dst_off, z_off;
    const float* yi;
    const float* yi_inv;
    const float* rec;
    int h, w;
};

// an item the buffers cannot hold, or with a side out of range, is skipped whole (uniform over the workgroup)
__device__ __forceinline__ bool load_item(const Params& p, int item, int src_planes, int dst_planes, bool noisy, Item& it) {
    namespace il = item_list;
    const int64_t* t = il::row(p.items, item);
    const int64_t src_off = t[il::SRC_OFF], dst_off = t[il::DST_OFF], h = t[il::H], w = t[il::W];
    const int64_t yi = t[il::SLOT], yi_inv = t[il::SLOT + 1], z = t[il::SLOT + 2];
    if (!il::side_ok(h, MIN_SIDE) || !il::side_ok(w, MIN_SIDE)) return false;
    if (!il::fits(src_off, src_planes * h * w, p.src_elems) || !il::fits(dst_off, dst_planes * h * w, p.dst_elems)) return false;
    if (!il::fits(yi, TABLE_N, p.tables_elems) || !il::fits(yi_inv, TABLE_N, p.tables_elems)) return false;
    if (noisy && !il::fits(z, h * w, p.normals_elems)) return false;
    it.src_off = src_off; it.dst_off = dst_off; it.z_off = z;
    it.yi = p.tables + yi; it.yi_inv = p.tables + yi_inv;
    it.rec = p.params + (int64_t)REC * item;
    it.h = (int)h; it.w = (int)w;
    return true;
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }   // NaN -> 0

__device__ __forceinline__ float lut(const float* table, float x) {                      // x in [0, 1]
    const int i = (int)rintf(x / 1e-6f);
    return table[i < TABLE_N - 1 ? i : TABLE_N - 1];
}

__device__ __forceinline__ float row3(const float* m, int r, const float x[3]) {
    return m[3 * r] * x[0] + m[3 * r + 1] * x[1] + m[3 * r + 2] * x[2];
}

// sRGB value -> XYZ(D50): the clamp, the inverse gamma, the inverse tone table and W1i (ISPNet.reverse up to xyz2linearrgb)
__device__ __forceinline__ void to_xyz(const Item& it, float x[3]) {
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = clamp01(x[c]);
        t = t > 0.04045f ? powf((200.f * t + 11.f) / 211.f, 2.4f) : fmaxf(t, 1e-8f) / 12.92f;
        v[c] = clamp01(lut(it.yi_inv, clamp01(t)));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = row3(it.rec + W1I, c, v);
}

// one camera channel of an XYZ pixel: the row of W2i and the exposure
__device__ __forceinline__ float to_camera(const Item& it, const float xyz[3], int c) {
    return clamp01(row3(it.rec + W2I, c, xyz) / it.rec[P2E]);
}

// camera pixel -> sRGB value (ISPNet.forward after the demosaic)
__device__ __forceinline__ void from_camera(const Item& it, float x[3]) {
    float v[3], u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = clamp01(x[c] * it.rec[P2E]);
#pragma unroll
    for (int c = 0; c < 3; ++c) u[c] = row3(it.rec + W2, c, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = clamp01(lut(it.yi, clamp01(row3(it.rec + W1, c, u))));
        t = t > 0.0031308f ? 1.055f * powf(t, (float)(1.0 / 2.4)) - 0.055f : 12.92f * t;
        x[c] = clamp01(t);
    }
}

__device__ __forceinline__ bool pixel_of_tile(const Params& p, const Item& it, int& y, int& x) {
    const item_list::Tile tile = item_list::tile_of_block(p.ntx, PH, PW);
    y = tile.y0 + threadIdx.x / PW;
    x = tile.x0 + threadIdx.x % PW;
    return y < it.h && x < it.w;
}

__global__ __launch_bounds__(NT) void isp_unprocess_kernel(Params p) {
    Item it;
    if (!load_item(p, blockIdx.y, 3, 1, true, it)) return;
    int y, x;
    if (!pixel_of_tile(p, it, y, x)) return;
    const int64_t plane = (int64_t)it.h * it.w, at = (int64_t)y * it.w + x;
    const float* s = p.src + it.src_off + at;
    float v[3] = {s[0], s[plane], s[2 * plane]};
    to_xyz(it, v);
    const float r = clamp01(to_camera(it, v, (y & 1) + (x & 1)));        // RGGB: the channel is the number of odd coordinates
    p.dst[it.dst_off + at] = clamp01(r + sqrtf(r * it.rec[SHOT] + it.rec[READ]) * p.normals[it.z_off + at]);
}

__global__ __launch_bounds__(NT) void isp_roundtrip_kernel(Params p) {
    Item it;
    if (!load_item(p, blockIdx.y, 3, 3, false, it)) return;
    int y, x;
    if (!pixel_of_tile(p, it, y, x)) return;
    const int64_t plane = (int64_t)it.h * it.w, at = (int64_t)y * it.w + x;
    const float* s = p.src + it.src_off + at;
    float v[3] = {s[0], s[plane], s[2 * plane]};
    to_xyz(it, v);
    float cam[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) cam[c] = to_camera(it, v, c);
    from_camera(it, cam);
    float* d = p.dst + it.dst_off + at;
    d[0] = cam[0]; d[plane] = cam[1]; d[2 * plane] = cam[2];
}

// torch's "reflect" (no repeated edge), folded as often as needed so that a tile reaching past a small image stays inside it
__device__ __forceinline__ int reflect(int i, int n) {
    const int q = 2 * (n - 1);
    int j = i % q;
    if (j < 0) j += q;
    return j >= n ? q - j : j;
}

__global__ __launch_bounds__(NT) void isp_process_kernel(Params p) {
    __shared__ float tile[SIDE * PITCH];
    __shared__ float outs[3 * TP * OPITCH];

    Item it;
    if (!load_item(p, blockIdx.y, 1, 3, false, it)) return;
    const item_list::Tile tl = item_list::tile_of_block(p.ntx, TP, TP);
    if (tl.surplus(it.h, it.w)) return;
    const int y0 = tl.y0, x0 = tl.x0;
    const int h = it.h, w = it.w;

    const float* raw = p.src + it.src_off;
    for (int i = threadIdx.x; i < SIDE * SIDE; i += NT) {
        const int r = i / SIDE, q = i - r * SIDE;
        tile[r * PITCH + q] = raw[(int64_t)reflect(y0 - 2 + r, h) * w + reflect(x0 - 2 + q, w)];
    }
    __syncthreads();

    const int qy = threadIdx.x / QT, qx = threadIdx.x % QT;
    if (y0 + 2 * qy < h && x0 + 2 * qx < w) {
        // the four 5 x 5 filters of Demosaic.__init__ (kgrb, krbg0, krbg1 = krbg0^T, krbbr), all weights exact in binary
        auto T = [&](int cy, int cx, int dy, int dx) { return tile[(cy + dy) * PITCH + cx + dx]; };
        auto cross = [&](int cy, int cx) {
            return 0.5f * T(cy, cx, 0, 0) + 0.25f * (T(cy, cx, -1, 0) + T(cy, cx, 1, 0) + T(cy, cx, 0, -1) + T(cy, cx, 0, 1)) -
                   0.125f * (T(cy, cx, -2, 0) + T(cy, cx, 2, 0) + T(cy, cx, 0, -2) + T(cy, cx, 0, 2));
        };
        auto diag = [&](int cy, int cx) {
            return 0.75f * T(cy, cx, 0, 0) + 0.25f * (T(cy, cx, -1, -1) + T(cy, cx, -1, 1) + T(cy, cx, 1, -1) + T(cy, cx, 1, 1)) -
                   0.1875f * (T(cy, cx, -2, 0) + T(cy, cx, 2, 0) + T(cy, cx, 0, -2) + T(cy, cx, 0, 2));
        };
        auto line = [&](int cy, int cx, int ay, int ax) {                 // krbg0: (ay, ax) = (0, 1); krbg1: (1, 0)
            return 0.625f * T(cy, cx, 0, 0) + 0.5f * (T(cy, cx, -ay, -ax) + T(cy, cx, ay, ax)) -
                   0.125f * (T(cy, cx, -2 * ay, -2 * ax) + T(cy, cx, 2 * ay, 2 * ax)) -
                   0.125f * (T(cy, cx, -1, -1) + T(cy, cx, -1, 1) + T(cy, cx, 1, -1) + T(cy, cx, 1, 1)) +
                   0.0625f * (T(cy, cx, -2 * ax, -2 * ay) + T(cy, cx, 2 * ax, 2 * ay));
        };
        const int cy = 2 * qy + 2, cx = 2 * qx + 2;
        float px[4][3];
        // (even, even) R site; (even, odd) G on a red row; (odd, even) G on a blue row; (odd, odd) B site -- Demosaic.forward
        px[0][0] = T(cy, cx, 0, 0);          px[0][1] = cross(cy, cx);            px[0][2] = diag(cy, cx);
        px[1][0] = line(cy, cx + 1, 0, 1);   px[1][1] = T(cy, cx + 1, 0, 0);      px[1][2] = line(cy, cx + 1, 1, 0);
        px[2][0] = line(cy + 1, cx, 1, 0);   px[2][1] = T(cy + 1, cx, 0, 0);      px[2][2] = line(cy + 1, cx, 0, 1);
        px[3][0] = diag(cy + 1, cx + 1);     px[3][1] = cross(cy + 1, cx + 1);    px[3][2] = T(cy + 1, cx + 1, 0, 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) px[k][c] = clamp01(px[k][c]);
            from_camera(it, px[k]);
            const int oy = 2 * qy + (k >> 1), ox = 2 * qx + (k & 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) outs[(c * TP + oy) * OPITCH + ox] = px[k][c];
        }
    }
    __syncthreads();

    const int64_t plane = (int64_t)h * w;
    float* dst = p.dst + it.dst_off;
    for (int i = threadIdx.x; i < 3 * TP * TP; i += NT) {
        const int c = i / (TP * TP), r = (i / TP) % TP, q = i % TP;
        if (y0 + r < h && x0 + q < w) dst[c * plane + (int64_t)(y0 + r) * w + x0 + q] = outs[(c * TP + r) * OPITCH + q];
    }
}

// what the host can see; 0 with the grid's tile counts, else the error
int check(const GrlIspArgs* a, bool noisy, int tw, int th, Params& p) {
    if (!a || a->C != 3) return GRL_ERR_BAD_ARG;
    item_list::Grid g;
    if (int e = item_list::check_tiled(*a, a->max_h, a->max_w, th, tw, g, MIN_SIDE)) return e;
    if (!a->params || !a->tables || (noisy && !a->normals)) return GRL_ERR_BAD_ARG;
    if (a->tables_elems < TABLE_N || (noisy && a->normals_elems <= 0)) return GRL_ERR_BAD_ARG;
    if ((uintptr_t)a->params % 4 || (uintptr_t)a->tables % 4 || (uintptr_t)a->normals % 4) return GRL_ERR_BAD_ARG;
    p.src = a->src; p.dst = a->dst; p.items = a->items; p.params = a->params; p.tables = a->tables; p.normals = a->normals;
    p.src_elems = a->src_elems; p.dst_elems = a->dst_elems; p.tables_elems = a->tables_elems;
    p.normals_elems = noisy ? a->normals_elems : 0;
    p.ntx = g.ntx; p.nty = g.nty;
    return 0;
}

}  // namespace

extern "C" int grl_isp_unprocess(void* stream, const GrlIspArgs* a) {
    Params p;
    if (int e = check(a, true, PW, PH, p)) return e;
    hipLaunchKernelGGL(isp_unprocess_kernel, dim3((unsigned)(p.ntx * p.nty), (unsigned)a->n_items), dim3(NT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_isp_process(void* stream, const GrlIspArgs* a) {
    Params p;
    if (int e = check(a, false, TP, TP, p)) return e;
    hipLaunchKernelGGL(isp_process_kernel, dim3((unsigned)(p.ntx * p.nty), (unsigned)a->n_items), dim3(NT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_isp_roundtrip(void* stream, const GrlIspArgs* a) {
    Params p;
    if (int e = check(a, false, PW, PH, p)) return e;
    hipLaunchKernelGGL(isp_roundtrip_kernel, dim3((unsigned)(p.ntx * p.nty), (unsigned)a->n_items), dim3(NT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
