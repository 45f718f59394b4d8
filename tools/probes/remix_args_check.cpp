// Host-side check of grl_batch_remix's argument validation (csrc/remix.hip) under AddressSanitizer and UBSan, without a GPU: every call
// below is refused before anything is launched, so the pointers -- addresses of host arrays, never dereferenced -- only have to be
// non-null and aligned.  A call that would launch is deliberately absent.
//
//   cd grl_image_restoration_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -I../../include -Xarch_host -fsanitize=address,undefined \
//         remix.hip ../../tools/probes/remix_args_check.cpp -o /tmp/remix_args_check && /tmp/remix_args_check
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
    alignas(16) static float lq[16], gt[16], lq_out[16], gt_out[16];
    alignas(16) static GrlRemixItem items[2];
    GrlBatchRemixArgs ok = {};
    ok.lq = lq; ok.gt = gt; ok.items = items; ok.lq_out = lq_out; ok.gt_out = gt_out;
    ok.B = 2; ok.P = 8; ok.Cl = 3; ok.Cg = 3; ok.b = 2; ok.p = 8; ok.s = 2; ok.mix = 1;
    const int64_t sl[4] = {192, 64, 8, 1}, sg[4] = {768, 256, 16, 1};
    for (int d = 0; d < 4; ++d) { ok.lq_stride[d] = sl[d]; ok.gt_stride[d] = sg[d]; }

    expect("null args", grl_batch_remix(nullptr, nullptr), GRL_ERR_BAD_ARG);
    GrlBatchRemixArgs a;
    a = ok; a.lq = nullptr; expect("null lq", grl_batch_remix(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.gt = nullptr; expect("null gt", grl_batch_remix(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.items = nullptr; expect("null items", grl_batch_remix(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.lq_out = nullptr; expect("null lq_out", grl_batch_remix(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.gt_out = nullptr; expect("null gt_out", grl_batch_remix(nullptr, &a), GRL_ERR_BAD_ARG);
    int32_t GrlBatchRemixArgs::* const sizes[] = {&GrlBatchRemixArgs::B, &GrlBatchRemixArgs::P, &GrlBatchRemixArgs::Cl, &GrlBatchRemixArgs::Cg,
                                                  &GrlBatchRemixArgs::b, &GrlBatchRemixArgs::p, &GrlBatchRemixArgs::s};
    for (auto m : sizes) {
        a = ok; a.*m = 0; expect("zero size", grl_batch_remix(nullptr, &a), GRL_ERR_BAD_ARG);
        a = ok; a.*m = INT32_MIN; expect("most negative size", grl_batch_remix(nullptr, &a), GRL_ERR_BAD_ARG);
    }
    a = ok; a.p = 9; expect("p > P", grl_batch_remix(nullptr, &a), GRL_ERR_BAD_ARG);
    a = ok; a.lq = (const float*)((const char*)lq + 2); expect("misaligned lq", grl_batch_remix(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.gt_out = (float*)((char*)gt_out + 1); expect("misaligned gt_out", grl_batch_remix(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.items = (const GrlRemixItem*)((const char*)items + 2); expect("misaligned items", grl_batch_remix(nullptr, &a), GRL_ERR_UNSUPPORTED);
    // sizes whose products pass 2^31 and 2^63: every product is checked before the next factor, so nothing overflows on the way
    a = ok; a.B = 1 << 15; a.P = 256; a.Cl = 1; expect("2^31 source elements", grl_batch_remix(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.B = a.P = a.p = a.Cl = a.Cg = a.b = a.s = INT32_MAX; expect("all sizes INT32_MAX", grl_batch_remix(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.P = a.p = 46340; a.Cl = a.Cg = 1; a.B = a.b = 1; a.s = INT32_MAX;
    expect("scale INT32_MAX", grl_batch_remix(nullptr, &a), GRL_ERR_UNSUPPORTED);
    a = ok; a.b = 65536; a.p = 1; expect("b above the grid", grl_batch_remix(nullptr, &a), GRL_ERR_UNSUPPORTED);
    printf("%s: %d failure(s)\n", failures ? "FAILED" : "ok", failures);
    return failures != 0;
}
