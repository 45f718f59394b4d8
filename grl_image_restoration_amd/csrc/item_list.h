// What the item-list entries share (include/grl_hip.h, "ITEM LIST": grl_cv_resize, grl_blur_items, grl_isp_unprocess / process /
// roundtrip, grl_color_jitter).  An item list is a device table of ROW = 8 int64 per item: src_off, dst_off, h, w and four slots the
// entry names.  The images are contiguous fp32 at ELEMENT offsets into a source and a destination arena.  The grid is (work of the
// largest item the host vouches for) x (items); a workgroup reads its item's row, skips the item whole unless every buffer it names
// holds it (`fits`, for each of them, after `side_ok` has bounded the counts), and leaves if it is a surplus workgroup of a smaller
// item.  So no list content can make a kernel touch memory outside the buffers its arguments describe, whoever built the list.
// Nothing here needs a HIP header: the predicates and the host checks compile in a host-only C++ translation unit
// (tests/host/item_list_check.cpp); the device helpers exist under hipcc alone.
#pragma once
#include <stdint.h>

#include "../../include/grl_hip.h"

#ifdef __HIPCC__
#define GRL_ITEM_HD __host__ __device__ __forceinline__
#else
#define GRL_ITEM_HD inline
#endif

namespace item_list {

constexpr int ROW = 8;                                  // int64 per item
enum { SRC_OFF = 0, DST_OFF = 1, H = 2, W = 3, SLOT = 4 };   // SLOT .. SLOT + 3: the entry's own
constexpr int64_t MAX_SIDE = 1 << 20;                   // of an image (and of a stride)
constexpr int64_t MAX_GRID_Y = 65535;                   // items (x planes, where a workgroup owns one plane) of one launch

GRL_ITEM_HD bool side_ok(int64_t v, int64_t lo = 1) { return v >= lo && v <= MAX_SIDE; }

// `count` elements at element `off` lie inside a buffer of `elems` elements.  No sum is formed, so no offset, however large, wraps
// into range; `count` is a product of sides that side_ok has bounded (at most 3 * 2^40) or a constant.
GRL_ITEM_HD bool fits(int64_t off, int64_t count, int64_t elems) {
    return off >= 0 && count >= 0 && count <= elems && off <= elems - count;
}

#ifdef __HIPCC__
__device__ __forceinline__ const int64_t* row(const int64_t* items, int64_t item) { return items + ROW * item; }

// The tile of blockIdx.x in a grid of ntx tiles per row: its first row and column for tiles of th x tw.
struct Tile {
    int y0, x0;
    __device__ __forceinline__ bool surplus(int h, int w) const { return y0 >= h || x0 >= w; }   // of a smaller item: leave
};
__device__ __forceinline__ Tile tile_of_block(int ntx, int th, int tw) {
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    return {ty * th, tx * tw};
}
#endif

// What the host can see of any entry's arguments (a non-null struct with src, dst, items, src_elems, dst_elems, n_items): src, dst
// and items non-null, src / dst 4-byte and items 8-byte aligned, 1 .. MAX_GRID_Y / planes items, positive arena lengths, the vouched
// maxima within min_side .. MAX_SIDE.  0 or GRL_ERR_BAD_ARG.
template <class Args>
inline int check_args(const Args& a, int64_t max_h, int64_t max_w, int64_t min_side = 1, int64_t planes = 1) {
    if (!a.src || !a.dst || !a.items) return GRL_ERR_BAD_ARG;
    if ((uintptr_t)a.src % 4 || (uintptr_t)a.dst % 4 || (uintptr_t)a.items % 8) return GRL_ERR_BAD_ARG;
    if (a.n_items <= 0 || planes < 1 || a.n_items > MAX_GRID_Y / planes || a.src_elems <= 0 || a.dst_elems <= 0) return GRL_ERR_BAD_ARG;
    if (!side_ok(max_h, min_side) || !side_ok(max_w, min_side)) return GRL_ERR_BAD_ARG;
    return 0;
}

// check_args, then the tile counts of a max_h x max_w image in tiles of th x tw; more than 2^31 - 1 tiles are GRL_ERR_BAD_ARG.
struct Grid {
    int32_t ntx, nty;
    unsigned tiles() const { return (unsigned)ntx * (unsigned)nty; }
};
template <class Args>
inline int check_tiled(const Args& a, int64_t max_h, int64_t max_w, int th, int tw, Grid& g, int64_t min_side = 1, int64_t planes = 1) {
    if (int e = check_args(a, max_h, max_w, min_side, planes)) return e;
    const int64_t ntx = (max_w + tw - 1) / tw, nty = (max_h + th - 1) / th;
    if (ntx * nty > 0x7fffffff) return GRL_ERR_BAD_ARG;
    g.ntx = (int32_t)ntx; g.nty = (int32_t)nty;
    return 0;
}

}  // namespace item_list
