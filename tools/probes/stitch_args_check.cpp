// Host-side check of grl_tile_stitch's argument validation (csrc/stitch.hip) under AddressSanitizer and UBSan, without a GPU: every
// call below is refused before anything is launched, so the pointers -- addresses of host arrays, never dereferenced -- only have to
// be non-null and aligned.  A call that would launch is deliberately absent.
//
//   cd grl_image_restoration_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I../../include -Xarch_host -fsanitize=address,undefined \
//         stitch.hip ../../tools/probes/stitch_args_check.cpp -o /tmp/stitch_args_check && /tmp/stitch_args_check
#include <stdint.h>
#include <stdio.h>

#include "grl_hip.h"

static int failures = 0;

static void expect(const char* what, int got, int want) {
    if (got != want) {
        printf("FAIL %s: returned %d, expected %d\n", what, got, want);
        ++failures;
    }
}

int main() {
    alignas(16) static float canvas[16], win[16];
    alignas(16) static int64_t tiles[16];
    GrlTileStitchArgs ok = {};
    ok.canvas = canvas; ok.tiles = tiles; ok.win = win;
    ok.b = 1; ok.c = 3; ok.h = 9; ok.w = 11; ok.tile = 4; ok.scale = 2; ok.ny = 4; ok.nx = 5; ok.lo = 0; ok.hi = 20;
    const int32_t oy[4] = {0, 2, 4, 5}, ox[5] = {0, 2, 4, 6, 7};
    for (int i = 0; i < 4; ++i) ok.oy[i] = oy[i];
    for (int i = 0; i < 5; ++i) ok.ox[i] = ox[i];

    expect("null args", grl_tile_stitch(nullptr, nullptr), GRL_ERR_BAD_ARG);
    GrlTileStitchArgs a;
    a = ok; a.canvas = nullptr; expect("null canvas", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.tiles = nullptr; expect("null tiles", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    int32_t GrlTileStitchArgs::* const sizes[] = {&GrlTileStitchArgs::b, &GrlTileStitchArgs::c, &GrlTileStitchArgs::h, &GrlTileStitchArgs::w,
                                                  &GrlTileStitchArgs::tile, &GrlTileStitchArgs::scale, &GrlTileStitchArgs::ny,
                                                  &GrlTileStitchArgs::nx};
    for (auto m : sizes) {
        a = ok; a.*m = 0; expect("zero size", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
        a = ok; a.*m = INT32_MIN; expect("most negative size", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    }
    a = ok; a.tile = 10; expect("tile > h", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.hi = 21; expect("hi > n", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.lo = 7; a.hi = 7; expect("lo == hi", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.lo = -1; expect("lo < 0", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.lo = INT32_MIN; a.hi = INT32_MAX; expect("extreme range", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.ox[4] = 8; expect("tile outside the canvas (columns)", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.oy[3] = 6; expect("tile outside the canvas (rows)", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.oy[0] = -1; expect("negative origin", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.ox[2] = 2; expect("origins that do not ascend", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.ox[1] = INT32_MAX; expect("origin INT32_MAX", grl_tile_stitch(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.nx = GRL_STITCH_MAX_ORIGINS + 1; expect("too many origins", grl_tile_stitch(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.ny = INT32_MAX; a.nx = INT32_MAX; expect("origin counts INT32_MAX", grl_tile_stitch(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.canvas = (float*)((char*)canvas + 2); expect("misaligned canvas", grl_tile_stitch(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.tiles = (const int64_t*)((const char*)tiles + 4); expect("misaligned tiles", grl_tile_stitch(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.win = (const float*)((const char*)win + 1); expect("misaligned window", grl_tile_stitch(nullptr, &a), GRL_ERR_UNSUPPORTED);
    // sizes whose products pass 2^31: formed in 64 bits, refused
    a = ok; a.h = a.w = 1 << 20; a.scale = 1 << 12; expect("2^32 canvas rows", grl_tile_stitch(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.h = a.w = a.tile = a.scale = INT32_MAX; a.ny = a.nx = 1; a.hi = 1;
    expect("all sizes INT32_MAX", grl_tile_stitch(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.b = 256; a.c = 256; expect("planes above the grid", grl_tile_stitch(nullptr, &a), GRL_ERR_UNSUPPORTED);
    printf("%s: %d failure(s)\n", failures ? "FAILED" : "ok", failures);
    return failures != 0;
}
