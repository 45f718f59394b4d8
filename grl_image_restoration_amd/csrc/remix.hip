// Progressive training and MixUp (include/grl_hip.h, grl_batch_remix): what the reference's engine does to a training batch between
// the loader and the model (engines/base.py:144-169: the stage's mini-batch and mini-patch; utils/dataset_utils.py:43-60: MixUp_AUG),
// for lq and gt in ONE launch.  Output sample i is the window (x0, y0) of input sample src_a -- blended, with mix, with the same
// window of input sample src_b:
//
//   out = __fadd_rn(__fmul_rn(lam, a), __fmul_rn(__fsub_rn(1.0f, lam), b))
//
// four IEEE operations, kept apart from the FMA contraction the rest of the library is built with, so that torch's
// lam * a + (1 - lam) * b on the CPU gives the same bits.  The items (src_a, src_b, x0, y0, lam) live in device memory.
//
// Shape of the kernel: blockIdx.y is the output sample; the threads of blockIdx.x are laid over that sample's rows, the Cl * p rows of
// lq_out first and the Cg * s p rows of gt_out after them, a fixed number of 4-element slots per row.  A row (c, r) is a contiguous
// run of w floats in the output and a run of w elements, a column stride apart, somewhere in each source.
//   vector row   the source's column stride is 1 and source A, source B (with mix) and the destination sit at the same offset m
//                (0 .. 3 elements) inside their 16-byte lines.  Slot k covers the columns [4k - m, 4k - m + 4) of the row: every
//                slot that lies whole inside [0, w) is one 16-byte load per source and one 16-byte store, aligned on all sides;
//                the row's first and last slot, when cut by its ends, go element by element.
//   scalar row   anything else (a crop at an odd offset against its output, a channels-last source).  Thread k takes the columns
//                k, k + n, k + 2n, k + 3n (n slots a row), so that the lanes of a wave stay side by side in every access.
// Nothing outside a window is read and nothing outside the outputs is written; slots past a row's end do nothing.  An item that
// points outside the batch or whose window leaves the patch is not followed: its output sample is left unwritten (the host
// validates every plan before it uploads it; this keeps a damaged table from becoming a wild read).
//
// Every source value is read once as an A and, with mix, once more as the B of the sample the permutation pairs it with; the second
// read of a training batch (a few MB) is served by the L2 / infinity cache.  No LDS, no atomics, no workspace, no scratch.
#include "common.h"

namespace {

constexpr int THREADS = 256;

struct RemixTensor {
    const float* src;
    float* dst;
    int64_t sn, sc, sh, sw;       // element strides of src
    int32_t C, w, k;              // channels, output side, window-origin multiplier (1 for lq, the scale for gt)
    int32_t slots;                // 4-element slots per row: ceil((w + 3) / 4), room for any misalignment m
};

struct RemixParams {
    RemixTensor t[2];             // lq, gt
    const GrlRemixItem* items;
    int32_t lq_work;              // slots of one lq_out sample; the gt slots follow
    int32_t B, P, p;
};

// this file is compiled with -ffp-contract=off (Makefile): under the library's contract=fast the backend fuses the last
// multiply and the add into an FMA whatever the intrinsics say
__device__ __forceinline__ float blend(float lam, float a, float b) {
    return __fadd_rn(__fmul_rn(lam, a), __fmul_rn(__fsub_rn(1.0f, lam), b));
}

template <bool MIX>
__global__ __launch_bounds__(THREADS) void batch_remix_kernel(RemixParams q) {
    const int i = blockIdx.y;
    const GrlRemixItem it = q.items[i];
    const int span = q.P - q.p;
    if ((unsigned)it.src_a >= (unsigned)q.B || (unsigned)it.x0 > (unsigned)span || (unsigned)it.y0 > (unsigned)span) return;
    if (MIX && (unsigned)it.src_b >= (unsigned)q.B) return;

    int g = blockIdx.x * THREADS + threadIdx.x;           // below 2^31 + THREADS: the launcher bounds a sample's slots
    const bool is_gt = g >= q.lq_work;
    if (is_gt) g -= q.lq_work;
    const RemixTensor& t = q.t[is_gt ? 1 : 0];
    const int w = t.w;
    const int row = g / t.slots, k = g % t.slots;
    if (row >= t.C * w) return;
    const int c = row / w, r = row % w;

    float* d = t.dst + (((int64_t)i * t.C + c) * w + r) * (int64_t)w;
    const int64_t win = c * t.sc + ((int64_t)it.x0 * t.k + r) * t.sh + (int64_t)it.y0 * t.k * t.sw;
    const float* a = t.src + it.src_a * t.sn + win;
    const float* b = MIX ? t.src + it.src_b * t.sn + win : a;
    const float lam = MIX ? it.lam : 0.0f;

    const int m = (int)(((uintptr_t)d >> 2) & 3);
    const bool vec = t.sw == 1 && (int)(((uintptr_t)a >> 2) & 3) == m && (int)(((uintptr_t)b >> 2) & 3) == m;
    if (vec) {
        // d + j is 16-byte aligned where (j + m) % 4 == 0, and so are a + j and b + j
        const int j0 = 4 * k - m;
        if (j0 >= 0 && j0 + 4 <= w) {
            const float4 va = *reinterpret_cast<const float4*>(a + j0);
            float4 o = va;
            if (MIX) {
                const float4 vb = *reinterpret_cast<const float4*>(b + j0);
                o.x = blend(lam, va.x, vb.x);
                o.y = blend(lam, va.y, vb.y);
                o.z = blend(lam, va.z, vb.z);
                o.w = blend(lam, va.w, vb.w);
            }
            *reinterpret_cast<float4*>(d + j0) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + e;
                if (j >= 0 && j < w) d[j] = MIX ? blend(lam, a[j], b[j]) : a[j];
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = k + e * t.slots;
            if (j < w) d[j] = MIX ? blend(lam, a[j * t.sw], b[j * t.sw]) : a[j * t.sw];
        }
    }
}

// n * C * side * side below 2^31 elements, every product checked before the next factor
bool fits(int32_t n, int32_t C, int64_t side) {
    const int64_t lim = (int64_t)1 << 31;
    if (side >= lim) return false;
    int64_t t = side * side;
    if (t >= lim) return false;
    t *= C;
    if (t >= lim) return false;
    return t * n < lim;
}

}  // namespace

extern "C" int grl_batch_remix(void* stream, const GrlBatchRemixArgs* a) {
    if (!a || !a->lq || !a->gt || !a->items || !a->lq_out || !a->gt_out) return GRL_ERR_BAD_ARG;
    if (a->B <= 0 || a->P <= 0 || a->Cl <= 0 || a->Cg <= 0 || a->b <= 0 || a->p <= 0 || a->s <= 0) return GRL_ERR_BAD_ARG;
    if (a->p > a->P) return GRL_ERR_BAD_ARG;
    if ((uint64_t)a->lq % 4 || (uint64_t)a->gt % 4 || (uint64_t)a->items % 4 || (uint64_t)a->lq_out % 4 || (uint64_t)a->gt_out % 4)
        return GRL_ERR_UNSUPPORTED;
    const int64_t Ps = (int64_t)a->P * a->s, ps = (int64_t)a->p * a->s;
    if (!fits(a->B, a->Cl, a->P) || !fits(a->B, a->Cg, Ps) || !fits(a->b, a->Cl, a->p) || !fits(a->b, a->Cg, ps))
        return GRL_ERR_UNSUPPORTED;
    if (a->b > 65535) return GRL_ERR_UNSUPPORTED;

    RemixParams q;
    q.t[0].src = a->lq; q.t[0].dst = a->lq_out; q.t[0].C = a->Cl; q.t[0].w = a->p; q.t[0].k = 1;
    q.t[0].sn = a->lq_stride[0]; q.t[0].sc = a->lq_stride[1]; q.t[0].sh = a->lq_stride[2]; q.t[0].sw = a->lq_stride[3];
    q.t[1].src = a->gt; q.t[1].dst = a->gt_out; q.t[1].C = a->Cg; q.t[1].w = (int32_t)ps; q.t[1].k = a->s;
    q.t[1].sn = a->gt_stride[0]; q.t[1].sc = a->gt_stride[1]; q.t[1].sh = a->gt_stride[2]; q.t[1].sw = a->gt_stride[3];
    int64_t work[2];
    for (int n = 0; n < 2; ++n) {
        q.t[n].slots = (q.t[n].w + 3 + 3) / 4;
        work[n] = (int64_t)q.t[n].C * q.t[n].w * q.t[n].slots;        // C w w below 2^31 and slots <= w / 4 + 2
    }
    q.items = a->items;
    if (work[0] + work[1] >= ((int64_t)1 << 31) - THREADS) return GRL_ERR_UNSUPPORTED;
    q.lq_work = (int32_t)work[0];
    q.B = a->B; q.P = a->P; q.p = a->p;
    const int64_t gx = (work[0] + work[1] + THREADS - 1) / THREADS;
    const dim3 grid((unsigned)gx, (unsigned)a->b);
    const hipStream_t st = (hipStream_t)stream;
    if (a->mix) hipLaunchKernelGGL(batch_remix_kernel<true>, grid, dim3(THREADS), 0, st, q);
    else hipLaunchKernelGGL(batch_remix_kernel<false>, grid, dim3(THREADS), 0, st, q);
    GRL_CHECK_LAUNCH();
    return 0;
}
