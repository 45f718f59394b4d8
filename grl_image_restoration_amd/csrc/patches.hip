// Training patches cut out of a device-resident store of 8-bit images (include/grl_hip.h, grl_sample_patches): the reference's
// per-sample host path -- _pad_images / _sample_patches (data/datasets/base_image.py:276-293), _augment (base_image.py:356-372),
// np.ascontiguousarray and to_tensor (restoration_sr.py:111-115) -- for a whole batch in one launch.
//
// Store: images back to back in one uint8 buffer, each H x W x C interleaved; offsets[n] is the first byte of image n, dims[n] its
// (H, W).  Work list (device memory, read by the kernel: a captured launch follows the list's contents): per sample
// (image, x, y, flags).  With S = P * scale the sample is
//     crop[r][c]  = image[x * scale + r][y * scale + c], 0 <= r, c < S, zero outside the image (the reference's bottom / right padding)
//     a[u][v]     = crop[flags & 1 ? S - 1 - u : u][flags & 2 ? S - 1 - v : v]         (x[::-1], then x[:, ::-1])
//     out[i][j]   = flags & 4 ? a[j][i] : a[i][j]                                       (np.swapaxes(x, 0, 1))
// written planar, fp32, as float(v) / 255 with IEEE division (to_tensor's ``.to(float32).div(255)``), never a reciprocal multiply.
//
// Shape: a workgroup of 256 threads owns one T x T tile (T = 32) of one sample's output, all channels.  It reads the source tile
// the output tile comes from -- rows of T * C contiguous bytes, consecutive lanes on consecutive bytes -- converts, and stages it
// de-interleaved in LDS in SOURCE orientation; the two flips and the axis swap are then only a choice of the LDS element each
// output element reads, so the transposed case never touches global memory with a stride.  Each thread stores four consecutive
// output columns per channel: one float4 when S is a multiple of 4 (rows are then 16-byte aligned), four guarded scalars otherwise.
// LDS rows are padded to T + 1 floats: a 32-lane half reads 4 rows x 8 quads (straight) or 8 quads x 4 rows (transposed) on 32
// distinct banks; the channel planes are offset by 11 banks so that the de-interleaving writes of C = 3 spread over the banks.
// Every global read is bounds-checked against the image, and a work-list entry whose image index is outside the store reads as
// zeros, so no list content can make the kernel read outside the store.
//
// grl_sample_patch_views (ABI 39) cuts up to four VIEWS of one work list in one launch: every view has its own store, scale and
// channel window (c0 .. c0 + C - 1 of Ctot) of an output batch, so the dual-pixel batch -- left view into lq[:, 0:3], right view
// into lq[:, 3:6], GT into gt -- is one launch with no torch.cat behind it.  The tile body below is the one both entries run; a
// workgroup of the view launch finds its view in a prefix table of first workgroups that travels in the by-value parameter struct,
// and takes the float4 store or not by its own view's S.
#include "common.h"

namespace {

constexpr int T = 32, NT = 256, LROW = T + 1, LPLANE = T * LROW + 11, CMAX = 3, VMAX = 4;

// one view of one launch: a store and the window of output channels it fills
struct View {
    const uint8_t* store;
    const int64_t* offsets;
    const int32_t* dims;
    float* out;
    int32_t N, C, S, scale, nt, Ctot, c0;
    int32_t first;                      // the view's first workgroup (grl_sample_patch_views; 0 in grl_sample_patches)
};

struct Params {
    View v;
    const int32_t* work;
};

struct ViewsParams {
    View v[VMAX];
    const int32_t* work;
    int32_t V;
};

// One T x T output tile of one sample of view `p`; `blk` counts the view's workgroups, `s` is the workgroup's CMAX * LPLANE floats.
template <int C, bool VEC>
__device__ __forceinline__ void sample_tile(const View& p, const int32_t* work, int blk, float* s) {
    const int tiles = p.nt * p.nt;
    const int b = blk / tiles, t = blk - b * tiles;
    const int I0 = (t / p.nt) * T, J0 = (t - (t / p.nt) * p.nt) * T;      // output tile origin
    const int S = p.S;

    const int4 w = *reinterpret_cast<const int4*>(work + 4 * (int64_t)b);
    const int img = w.x, flags = w.w;
    const bool fr = flags & 1, fc = flags & 2, sw = flags & 4;
    const bool have = (uint32_t)img < (uint32_t)p.N;
    const int H = have ? p.dims[2 * img] : 0, W = have ? p.dims[2 * img + 1] : 0;
    const uint8_t* const src = p.store + (have ? p.offsets[img] : 0);
    const int64_t r0 = (int64_t)w.y * p.scale, c0 = (int64_t)w.z * p.scale;   // crop origin in the image

    // origin of the source tile in crop coordinates; with a flip the tile is anchored at its far end, so that local index
    // T - 1 - d holds what output offset d reads (ragged tiles then start before the crop: those elements are never read)
    const int U0 = sw ? J0 : I0, V0 = sw ? I0 : J0;
    const int R0 = fr ? S - U0 - T : U0, C0 = fc ? S - V0 - T : V0;

    for (int i = threadIdx.x; i < T * T * C; i += NT) {
        const int lr = i / (T * C), k = i - lr * (T * C);
        const int lc = k / C, ch = k - lc * C;
        const int r = R0 + lr, c = C0 + lc;                                   // crop coordinates
        float v = 0.f;
        if ((uint32_t)r < (uint32_t)S && (uint32_t)c < (uint32_t)S) {
            const int64_t y = r0 + r, x = c0 + c;
            if (y >= 0 && y < H && x >= 0 && x < W) v = __fdiv_rn((float)src[(y * W + x) * C + ch], 255.f);
        }
        s[ch * LPLANE + lr * LROW + lc] = v;
    }
    __syncthreads();

    const int a = threadIdx.x / (T / 4), b4 = (threadIdx.x % (T / 4)) * 4;
    const int i = I0 + a, j = J0 + b4;
    if (i >= S || j >= S) return;
    float* o = p.out + (((int64_t)b * p.Ctot + p.c0) * S + i) * S + j;
    const int64_t plane = (int64_t)S * S;
#pragma unroll
    for (int ch = 0; ch < C; ++ch, o += plane) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int du = sw ? b4 + e : a, dv = sw ? a : b4 + e;
            v[e] = s[ch * LPLANE + (fr ? T - 1 - du : du) * LROW + (fc ? T - 1 - dv : dv)];
        }
        if (VEC) {                                   // S % 4 == 0: j + 3 < S and the row is 16-byte aligned
            *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (j + e < S) o[e] = v[e];
        }
    }
}

template <int C, bool VEC>
__global__ __launch_bounds__(NT) void sample_patches_kernel(Params p) {
    __shared__ float s[CMAX * LPLANE];
    sample_tile<C, VEC>(p.v, p.work, blockIdx.x, s);
}

// Every workgroup of the launch belongs to one view: the last one whose first workgroup is not after it.  The choice and the two
// branches below are uniform over the workgroup.
__global__ __launch_bounds__(NT) void sample_patch_views_kernel(ViewsParams p) {
    __shared__ float s[CMAX * LPLANE];
    View v = p.v[0];                    // constant indices only: the table stays in scalar registers, never in scratch
#pragma unroll
    for (int q = 1; q < VMAX; ++q)
        if (q < p.V && (int)blockIdx.x >= p.v[q].first) v = p.v[q];
    const int blk = blockIdx.x - v.first;
    const bool vec = v.S % 4 == 0;
    if (v.C == 3) {
        if (vec) sample_tile<3, true>(v, p.work, blk, s);
        else sample_tile<3, false>(v, p.work, blk, s);
    } else {
        if (vec) sample_tile<1, true>(v, p.work, blk, s);
        else sample_tile<1, false>(v, p.work, blk, s);
    }
}

// The checks of one view that both entries share (GRL_ERR_BAD_ARG as 0); fills `v` but for `first`.
bool fill_view(View& v, const uint8_t* store, const int64_t* offsets, const int32_t* dims, float* out, int32_t N, int32_t C,
               int32_t scale, int32_t Ctot, int32_t c0, int32_t P) {
    if (!store || !offsets || !dims || !out) return false;
    if (C != 1 && C != 3) return false;
    if (N <= 0 || P <= 0 || scale < 1) return false;
    if (c0 < 0 || (int64_t)c0 + C > Ctot) return false;
    if ((uint64_t)out % 16 || (uint64_t)offsets % 8 || (uint64_t)dims % 4) return false;
    const int64_t S = (int64_t)P * scale;
    if (S > (1 << 20)) return false;
    v.store = store; v.offsets = offsets; v.dims = dims; v.out = out;
    v.N = N; v.C = C; v.S = (int32_t)S; v.scale = scale; v.nt = (int32_t)((S + T - 1) / T); v.Ctot = Ctot; v.c0 = c0; v.first = 0;
    return true;
}

}  // namespace

extern "C" int grl_sample_patches(void* stream, const GrlPatchArgs* a) {
    if (!a || !a->work || a->B <= 0 || (uint64_t)a->work % 16) return GRL_ERR_BAD_ARG;
    Params p;
    if (!fill_view(p.v, a->store, a->offsets, a->dims, a->out, a->N, a->C, a->scale, a->C, 0, a->P)) return GRL_ERR_BAD_ARG;
    p.work = a->work;
    const int64_t grid = (int64_t)a->B * p.v.nt * p.v.nt;
    if (grid > 0x7fffffff) return GRL_ERR_BAD_ARG;

    const dim3 g((unsigned)grid), blk(NT);
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = p.v.S % 4 == 0;
    if (a->C == 3 && vec) hipLaunchKernelGGL((sample_patches_kernel<3, true>), g, blk, 0, st, p);
    else if (a->C == 3) hipLaunchKernelGGL((sample_patches_kernel<3, false>), g, blk, 0, st, p);
    else if (vec) hipLaunchKernelGGL((sample_patches_kernel<1, true>), g, blk, 0, st, p);
    else hipLaunchKernelGGL((sample_patches_kernel<1, false>), g, blk, 0, st, p);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_sample_patch_views(void* stream, const GrlPatchViewsArgs* a) {
    if (!a || !a->work || a->B <= 0 || (uint64_t)a->work % 16) return GRL_ERR_BAD_ARG;
    if (a->V < 1 || a->V > VMAX) return GRL_ERR_BAD_ARG;
    ViewsParams p = {};
    int64_t grid = 0;
    for (int k = 0; k < a->V; ++k) {
        const GrlPatchView& w = a->view[k];
        if (!fill_view(p.v[k], w.store, w.offsets, w.dims, w.out, w.N, w.C, w.scale, w.Ctot, w.c0, a->P)) return GRL_ERR_BAD_ARG;
        if (grid > 0x7fffffff) return GRL_ERR_BAD_ARG;
        p.v[k].first = (int32_t)grid;
        grid += (int64_t)a->B * p.v[k].nt * p.v[k].nt;
    }
    if (grid > 0x7fffffff) return GRL_ERR_BAD_ARG;
    p.work = a->work; p.V = a->V;
    hipLaunchKernelGGL(sample_patch_views_kernel, dim3((unsigned)grid), dim3(NT), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
