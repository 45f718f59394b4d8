// Tiled inference, the stitch (include/grl_hip.h, grl_tile_stitch): the E / W accumulation of the reference's forward_tile
// (engines/base.py:100-116) for a contiguous range [lo, hi) of the row-major tile list, in ONE launch, with an optional 1-D blending
// window.  Every canvas pixel is owned by one thread, which walks the tiles that cover it in the reference's loop order:
//
//   acc  = first covering tile >= lo ? +0.0f : canvas            (an earlier chunk started the pixel)
//   acc  = __fadd_rn(acc, __fmul_rn(o, wgt))                     for the covering tiles inside [lo, hi)
//   wgt  = __fmul_rn(win[y - oy * scale], win[x - ox * scale])   (1.0f without a window)
//   acc  = __fdiv_rn(acc, wsum)                                  once the last covering tile is below hi; wsum over ALL covering tiles
//
// so the sums have torch's order and rounding, chunk after chunk gives the bits of one call, and a pixel is written once per call and
// read only when an earlier call began it.  This file is compiled with -ffp-contract=off (Makefile), as remix.hip is.
//
// Shape of the kernel: the grid covers the bounding box of the chunk's tiles only.  blockIdx.y is a group of four canvas rows of the
// box and blockIdx.z a (batch, channel) plane; the threads of blockIdx.x are laid over a row in 4-pixel slots that are 16-byte aligned IN
// THE CANVAS (a row of an odd-width canvas starts anywhere inside a 16-byte line: slot k covers the columns [4k - m, 4k - m + 4), m
// the row's misalignment).  The covering tile rows are the same for the whole workgroup; every thread finds its covering tile
// columns by a scan of the origin list (tens of entries, in the kernel arguments).
//   vector slot   whole inside the box and with ONE set of covering tiles for its four pixels: one 16-byte canvas store (and load,
//                 when an earlier chunk started the pixels), and per tile one 16-byte load where the tile's row is 16-byte aligned
//                 at that column, four 4-byte loads where it is not (an origin of 1100 output pixels at scale 3, a strided view).
//   scalar slot   a slot cut by the box or by a tile's edge: pixel by pixel.
// Nothing outside the tiles' (b, c, ts, ts) extents is read and nothing outside the box is written; a pixel that no tile of the
// chunk covers is not touched.  No LDS, no atomics, no workspace, no scratch.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int ROWS_PER_BLOCK = 4;       // canvas rows a workgroup walks: the scan of the tile columns serves all of them
constexpr int ROW = 8;                  // int64 per tile of the table: address, batch / channel / row stride, 4 reserved

struct StitchParams {
    float* canvas;
    const int64_t* tiles;               // row k: tile lo + k
    const float* win;
    int32_t C, H, W;                    // canvas planes per batch item, rows, columns
    int32_t ts, scale, ny, nx, lo, hi;
    int32_t by0, by1, bx0, bx1;         // the box: first row and column, one past the last row and column
    int32_t oy[GRL_STITCH_MAX_ORIGINS], ox[GRL_STITCH_MAX_ORIGINS];
};

// the covering range [i0, i1) of coordinate p on an axis: origins ascend, so the tiles with o * scale <= p < o * scale + ts are
// the ones after those that end at or before p and up to the last that starts at or before p
__device__ __forceinline__ void cover(const int32_t* o, int n, int scale, int ts, int p, int& i0, int& i1) {
    i0 = 0; i1 = 0;
    for (int i = 0; i < n; ++i) {
        const int s = o[i] * scale;
        i0 += s + ts <= p;
        i1 += s <= p;
    }
}

// N pixels (x .. x + N - 1 of row y) with the covering tiles [iy0, iy1) x [ix0, ix1); N == 4: one aligned 16-byte slot of the canvas
template <int N>
__device__ __forceinline__ void pixels(const StitchParams& q, float* crow, int64_t plane_b, int64_t plane_c, int y, int x,
                                       int iy0, int iy1, int ix0, int ix1) {
    if (ix0 >= ix1) return;                                                   // (a canvas the grid does not cover whole)
    bool any = false;
    for (int iy = iy0; iy < iy1; ++iy) any |= iy * q.nx + ix0 < q.hi && iy * q.nx + ix1 > q.lo;
    if (!any) return;

    float acc[N], wsum[N];
    const bool started = iy0 * q.nx + ix0 < q.lo;
    if constexpr (N == 4) {
        const float4 v = started ? *reinterpret_cast<const float4*>(crow + x) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        acc[0] = v.x; acc[1] = v.y; acc[2] = v.z; acc[3] = v.w;
    } else {
        acc[0] = started ? crow[x] : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < N; ++e) wsum[e] = 0.0f;

    for (int iy = iy0; iy < iy1; ++iy) {
        const int ty = y - q.oy[iy] * q.scale;
        const float wy = q.win ? q.win[ty] : 1.0f;
        for (int ix = ix0; ix < ix1; ++ix) {
            const int tx = x - q.ox[ix] * q.scale;
            float wgt[N];
#pragma unroll
            for (int e = 0; e < N; ++e) {
                wgt[e] = q.win ? __fmul_rn(wy, q.win[tx + e]) : 1.0f;
                wsum[e] = __fadd_rn(wsum[e], wgt[e]);
            }
            const int t = iy * q.nx + ix;
            if (t < q.lo || t >= q.hi) continue;
            const int64_t* r = q.tiles + (int64_t)(t - q.lo) * ROW;
            const float* o = reinterpret_cast<const float*>((uintptr_t)r[0]) + plane_b * r[1] + plane_c * r[2] + ty * r[3] + tx;
            float v[N];
            bool wide = false;
            if constexpr (N == 4) {
                wide = ((uintptr_t)o & 15) == 0;
                if (wide) {
                    const float4 f = *reinterpret_cast<const float4*>(o);
                    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                }
            }
            if (!wide) {
#pragma unroll
                for (int e = 0; e < N; ++e) v[e] = o[e];
            }
#pragma unroll
            for (int e = 0; e < N; ++e) acc[e] = __fadd_rn(acc[e], __fmul_rn(v[e], wgt[e]));
        }
    }
    if ((iy1 - 1) * q.nx + ix1 - 1 < q.hi) {
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = __fdiv_rn(acc[e], wsum[e]);
    }
    if constexpr (N == 4) *reinterpret_cast<float4*>(crow + x) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else crow[x] = acc[0];
}

__global__ __launch_bounds__(THREADS) void tile_stitch_kernel(StitchParams q) {
    const int plane = blockIdx.z;
    const int pb = plane / q.C, pc = plane - pb * q.C;
    const int slot = blockIdx.x * THREADS + threadIdx.x;
    int seen = -8, a0 = 0, a1 = 0, b0 = 0, b1 = 0;                            // the slot origin the column scans were made for
    for (int r = 0; r < ROWS_PER_BLOCK; ++r) {
        const int y = q.by0 + blockIdx.y * ROWS_PER_BLOCK + r;
        if (y >= q.by1) break;
        float* crow = q.canvas + ((int64_t)plane * q.H + y) * q.W;
        const int m = (int)(((uintptr_t)crow >> 2) & 3);                      // crow + j is 16-byte aligned where (j + m) % 4 == 0
        const int x0 = 4 * ((q.bx0 + m) / 4 + slot) - m;
        if (x0 >= q.bx1) continue;
        int iy0, iy1;
        cover(q.oy, q.ny, q.scale, q.ts, y, iy0, iy1);
        if (iy0 >= iy1) continue;
        if (x0 != seen) {                                                     // (every row, where the canvas width is no multiple of 4)
            cover(q.ox, q.nx, q.scale, q.ts, x0 < 0 ? 0 : x0, a0, a1);
            cover(q.ox, q.nx, q.scale, q.ts, x0 + 3, b0, b1);
            seen = x0;
        }
        if (x0 >= q.bx0 && x0 + 4 <= q.bx1 && a0 == b0 && a1 == b1) {
            pixels<4>(q, crow, pb, pc, y, x0, iy0, iy1, a0, a1);
        } else {
            for (int e = 0; e < 4; ++e) {
                const int x = x0 + e;
                if (x < q.bx0 || x >= q.bx1) continue;
                int c0, c1;
                cover(q.ox, q.nx, q.scale, q.ts, x, c0, c1);
                pixels<1>(q, crow, pb, pc, y, x, iy0, iy1, c0, c1);
            }
        }
    }
}

// strictly ascending origins of tiles that lie inside an axis of `dim` input pixels
bool origins_ok(const int32_t* o, int n, int tile, int dim) {
    for (int i = 0; i < n; ++i) {
        if (o[i] < 0 || o[i] > dim - tile) return false;
        if (i && o[i] <= o[i - 1]) return false;
    }
    return true;
}

}  // namespace

extern "C" int grl_tile_stitch(void* stream, const GrlTileStitchArgs* a) {
    if (!a || !a->canvas || !a->tiles) return GRL_ERR_BAD_ARG;
    if (a->b <= 0 || a->c <= 0 || a->h <= 0 || a->w <= 0 || a->tile <= 0 || a->scale <= 0 || a->ny <= 0 || a->nx <= 0) return GRL_ERR_BAD_ARG;
    if (a->tile > a->h || a->tile > a->w) return GRL_ERR_BAD_ARG;
    if (a->ny > GRL_STITCH_MAX_ORIGINS || a->nx > GRL_STITCH_MAX_ORIGINS) return GRL_ERR_UNSUPPORTED;
    if (a->lo < 0 || a->lo >= a->hi || a->hi > a->ny * a->nx) return GRL_ERR_BAD_ARG;
    if (!origins_ok(a->oy, a->ny, a->tile, a->h) || !origins_ok(a->ox, a->nx, a->tile, a->w)) return GRL_ERR_BAD_ARG;
    if ((uintptr_t)a->canvas % 4 || (uintptr_t)a->tiles % 8 || (uintptr_t)a->win % 4) return GRL_ERR_UNSUPPORTED;
    const int64_t H = (int64_t)a->h * a->scale, W = (int64_t)a->w * a->scale, ts = (int64_t)a->tile * a->scale;
    const int64_t planes = (int64_t)a->b * a->c;
    if (H > 0x7ffffff0 || W > 0x7ffffff0 || planes > 65535) return GRL_ERR_UNSUPPORTED;

    StitchParams q;
    q.canvas = a->canvas; q.tiles = a->tiles; q.win = a->win;
    q.C = a->c; q.H = (int32_t)H; q.W = (int32_t)W;
    q.ts = (int32_t)ts; q.scale = a->scale; q.ny = a->ny; q.nx = a->nx; q.lo = a->lo; q.hi = a->hi;
    for (int i = 0; i < GRL_STITCH_MAX_ORIGINS; ++i) {
        q.oy[i] = i < a->ny ? a->oy[i] : 0;
        q.ox[i] = i < a->nx ? a->ox[i] : 0;
    }
    // the box of the chunk: its band of tile rows; all columns unless the chunk lies inside one tile row
    const int r0 = a->lo / a->nx, r1 = (a->hi - 1) / a->nx;
    const int c0 = r0 == r1 ? a->lo % a->nx : 0, c1 = r0 == r1 ? (a->hi - 1) % a->nx : a->nx - 1;
    q.by0 = a->oy[r0] * a->scale;
    q.bx0 = a->ox[c0] * a->scale;
    q.bx1 = (int32_t)(a->ox[c1] * (int64_t)a->scale + ts);
    q.by1 = (int32_t)(a->oy[r1] * (int64_t)a->scale + ts);
    const int64_t rows = (q.by1 - q.by0 + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    if (rows > 65535) return GRL_ERR_UNSUPPORTED;
    const int64_t slots = (q.bx1 - q.bx0 + 3) / 4 + 1;                       // room for any misalignment of a row
    const dim3 grid((unsigned)((slots + THREADS - 1) / THREADS), (unsigned)rows, (unsigned)planes);
    hipLaunchKernelGGL(tile_stitch_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, q);
    GRL_CHECK_LAUNCH();
    return 0;
}
