// Host check of csrc/item_list.h: the fit predicate and the host helpers at their boundaries.  A host-only C++ program (no HIP
// header), built with -fsanitize=undefined,address -fno-sanitize-recover=all by tests/test_item_list.py: a signed overflow in a
// check is then a failure of its own, not a wrong answer.  Exit status 0 and "ok" on success; the first failed line otherwise.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "../../grl_image_restoration_amd/csrc/item_list.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

namespace il = item_list;

struct Args {                                   // the fields every entry's argument struct has
    const float* src;
    float* dst;
    const int64_t* items;
    int64_t src_elems, dst_elems;
    int32_t n_items;
};

static void check_fits() {
    const int64_t count = 3 * il::MAX_SIDE * il::MAX_SIDE;                  // the largest the side limits allow: 3 * 2^40
    for (int64_t elems : {count, count + 5, INT64_MAX}) {
        CHECK(il::fits(0, count, elems));
        CHECK(il::fits(elems - count, count, elems));
        CHECK(!il::fits(elems - count + 1, count, elems));
        CHECK(!il::fits(-1, count, elems));
        CHECK(!il::fits(INT64_MAX, count, elems));
        CHECK(!il::fits(INT64_MAX - count + 1, count, elems));              // off + count would wrap to INT64_MIN
        CHECK(!il::fits(INT64_MIN, count, elems));
    }
    CHECK(!il::fits(INT64_MAX, count, INT64_MAX));
    CHECK(il::fits(INT64_MAX - count, count, INT64_MAX));
    // a small arena, as the kernels' tests use: 192 elements, items of 3 x 8 x 8
    CHECK(il::fits(0, 192, 192) && !il::fits(1, 192, 192) && !il::fits(64, 192, 192) && !il::fits(-1, 192, 192));
    CHECK(il::fits(0, 9, 9) && !il::fits(1, 9, 9));
    CHECK(!il::fits(0, 193, 192) && !il::fits(0, count, 192));              // more than the buffer holds
    CHECK(!il::fits(INT64_MAX, 192, 192) && !il::fits(INT64_MAX - 192 + 1, 192, 192) && !il::fits(INT64_MAX - 191, 1, 192));
    // count 0: any offset inside the buffer, its end included
    CHECK(il::fits(0, 0, 192) && il::fits(192, 0, 192) && !il::fits(193, 0, 192) && !il::fits(-1, 0, 192) && il::fits(0, 0, 0));
    CHECK(!il::fits(0, -1, 192) && !il::fits(0, 1, 0) && !il::fits(0, 1, -5) && !il::fits(0, 0, -1));
}

static void check_sides() {
    CHECK(il::side_ok(1) && il::side_ok(il::MAX_SIDE) && !il::side_ok(0) && !il::side_ok(-1) && !il::side_ok(il::MAX_SIDE + 1));
    CHECK(!il::side_ok(INT64_MAX) && !il::side_ok(INT64_MIN));
    CHECK(il::side_ok(3, 3) && !il::side_ok(2, 3));
    CHECK(il::MAX_SIDE == 1048576 && il::MAX_GRID_Y == 65535 && il::ROW == 8 && il::SLOT + 4 == il::ROW);
}

static void check_host_helpers() {
    alignas(8) static char mem[64];
    const Args good = {(const float*)mem, (float*)(mem + 16), (const int64_t*)(mem + 32), 192, 192, 1};
    il::Grid g = {-1, -1};
    const int T = 16;
    // tile counts for max = 1, tile, tile + 1 and 2^20, on each axis
    const int64_t maxima[] = {1, T, T + 1, il::MAX_SIDE};
    const int32_t tiles[] = {1, 1, 2, (int32_t)(il::MAX_SIDE / T)};
    for (int i = 0; i < 4; ++i) {
        CHECK(il::check_tiled(good, maxima[i], 1, T, T, g) == 0 && g.nty == tiles[i] && g.ntx == 1 && g.tiles() == (unsigned)tiles[i]);
        CHECK(il::check_tiled(good, 1, maxima[i], T, T, g) == 0 && g.ntx == tiles[i] && g.nty == 1);
    }
    CHECK(il::check_tiled(good, 5, 130, 4, 64, g) == 0 && g.nty == 2 && g.ntx == 3);          // th x tw = 4 x 64
    CHECK(il::check_tiled(good, il::MAX_SIDE, il::MAX_SIDE / 4, T, T, g) == 0 && g.tiles() == 1u << 30);
    CHECK(il::check_tiled(good, il::MAX_SIDE, il::MAX_SIDE / 2, T, T, g) == GRL_ERR_BAD_ARG);  // 2^31 tiles: one beyond 2^31 - 1
    CHECK(il::check_tiled(good, il::MAX_SIDE, il::MAX_SIDE, 4, 64, g) == GRL_ERR_BAD_ARG);    // 2^18 x 2^14 tiles: beyond 2^31 - 1
    CHECK(il::check_tiled(good, il::MAX_SIDE + 1, 1, T, T, g) == GRL_ERR_BAD_ARG);
    CHECK(il::check_tiled(good, 0, 1, T, T, g) == GRL_ERR_BAD_ARG && il::check_tiled(good, 1, -3, T, T, g) == GRL_ERR_BAD_ARG);
    CHECK(il::check_tiled(good, 2, 3, T, T, g, 3) == GRL_ERR_BAD_ARG && il::check_tiled(good, 3, 3, T, T, g, 3) == 0);

    CHECK(il::check_args(good, 8, 8) == 0);
    Args a = good; a.src = nullptr;                           CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.dst = nullptr;                                CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.items = nullptr;                              CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.src = (const float*)(mem + 2);                CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.dst = (float*)(mem + 17);                     CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.items = (const int64_t*)(mem + 36);           CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.src_elems = 0;                                CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.dst_elems = -1;                               CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.n_items = 0;                                  CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.n_items = -1;                                 CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.n_items = 65535;                              CHECK(il::check_args(a, 8, 8) == 0);
    a = good; a.n_items = 65536;                              CHECK(il::check_args(a, 8, 8) == GRL_ERR_BAD_ARG);
    a = good; a.n_items = 21845;                              CHECK(il::check_args(a, 8, 8, 1, 3) == 0);     // 3 planes per item
    a = good; a.n_items = 21846;                              CHECK(il::check_args(a, 8, 8, 1, 3) == GRL_ERR_BAD_ARG);
    a = good; a.n_items = INT32_MAX;                          CHECK(il::check_args(a, 8, 8, 1, 3) == GRL_ERR_BAD_ARG);
    CHECK(il::check_args(good, 8, 8, 1, 0) == GRL_ERR_BAD_ARG);
}

int main() {
    check_fits();
    check_sides();
    check_host_helpers();
    puts("ok");
    return 0;
}
