// Unsharp-mask sharpening of an image batch (include/grl_hip.h, grl_usm_sharp): the reference's ``usm_sharp``
// (utils/utils_bsr/utils_usm.py:34-60; its torch twin ``USMSharp`` at :63-82), which turns the GT of the real-world-SR PSNR stage into
// its sharpened target (data/datasets/restoration_sr.py:105-109 for validation, restoration_bsr.py:56-59 for training).
//
//   idx(i, n)  = reflect-101, reflected as often as needed: n == 1 -> 0; else j = i mod 2(n-1); j >= n ? 2(n-1) - j : j
//   G(a)[y][x] = column pass(row pass(a)); a pass is one fp32 fmaf chain from 0 over the taps t = 0 .. K-1 on a[idx(. + t - K/2)]
//   blur = G(x);  res = x - blur;  m = fabsf(res) * 255.0f > threshold ? 1 : 0
//   soft = G(m);  sharp = clamp(x + weight * res, 0, 1);  out = soft * sharp + (1 - soft) * x     (every operation rounded on its own)
//   quantise: out = float(rint(clamp(out, 0, 1) * 255.0f)) / 255 by IEEE division (single2uint, then to_tensor)
//
// Shape: two launches of one tiled separable blur.  A workgroup of 256 threads owns a TH x TW = 64 x 32 output tile of one (n, c)
// plane.  It first writes the reflected source row of every tile row and the reflected source column of every tile column into LDS
// (one integer modulo per thread instead of one per pixel), then stages the (TH+K-1) x (TW+K-1) source tile through these tables
// (three loads per thread and row in flight before the first LDS write).  Row pass: a lane owns four adjacent outputs of one tile row
// and walks the taps four at a time: one ds_read_b128 brings the next four source values, 16 fmaf consume a seven-value register
// window, so the pass costs 1/16 LDS read per fmaf.  The LDS row stride is 96 dwords.  The LDS serves a wave64 ds_read_b128 in four
// groups of 16 lanes that are NOT consecutive: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same plus 32.  With lane = 8 * row
// + column group, the first group reads 16-dword pieces of four tile rows -- columns 0-15 of row r, 16-31 of r + 1, 16-31 of r + 2,
// 0-15 of r + 3 -- and the second the complementary pieces; at a stride of 96 = 32 (mod 64) dwords they start at banks 0, 48, 16, 32
// (and 16, 32, 0, 48), four different quarters of the 64 banks.  Derived from the bank rule, not measured with the conflict counter.
// 96 >= TW + 64 also covers the last read-ahead at K = 63.  The row-blurred tile goes back to LDS as one float4 per lane; the column pass reads it with lanes along the
// row (32 consecutive dwords: conflict free), a lane owning two runs of four outputs down a column with the same window walk.
// Every tap is a wave-uniform read of device memory (scalar cache): nothing is uploaded and the host never synchronises, so the call
// can be captured and the taps rewritten between replays.  Kernel 1 ends by storing blur and the 0 / 1 mask into the workspace;
// kernel 2 blurs the mask the same way and blends.  Every output is the same fmaf chain in the same order wherever its tile lies,
// so the result does not depend on the tiling or on the position in the batch.  K is a run-time value (1 .. 63): the dynamic LDS
// is (TH+K-1) * (96 + 32) + TH + TW + 2K - 2 dwords, 58.8 KB at K = 51 and 65392 bytes at K = 63, under the 64 KB that need no opt-in.
#include "common.h"

namespace {

constexpr int TW = 32, TH = 64, NT = 256, LW = 96, KMAX = 63;
typedef float f4 __attribute__((ext_vector_type(4)));
static_assert(LW % 64 == 32 && LW >= TW + (KMAX + 3) / 4 * 4, "bank spread of the row pass and room for its read-ahead");
static_assert(3 * 32 >= TW + KMAX - 1, "the staging loop covers a tile row in three steps of 32 lanes");

struct Params {
    const float* x;
    const float* taps;
    float* blur;
    float* mask;
    float* out;
    float weight, threshold;
    int32_t K, H, W, ntx, nty, quantise;
};

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int j = i % p;
    if (j < 0) j += p;
    return j >= n ? p - j : j;
}

// Four adjacent outputs of one pass: acc[j] = fmaf(taps[t], a[j + t], acc[j]) for t = 0 .. K-1 in this order.  load(i) returns
// a[4 i .. 4 i + 3]; it is called for i = 0 .. ceil(K / 4), the last call only feeds taps that exist.
template <class Load>
__device__ __forceinline__ void chain4(const float* __restrict__ taps, int K, Load load, float (&acc)[4]) {
    f4 cur = load(0);
    int t0 = 0, i = 1;
    for (; t0 + 4 <= K; t0 += 4, ++i) {
        const f4 nxt = load(i);
        const float w[7] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z};
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const float tap = taps[t0 + tt];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(tap, w[tt + j], acc[j]);
        }
        cur = nxt;
    }
    if (t0 < K) {                                          // the last one to three taps
        const f4 nxt = load(i);
        const float w[7] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z};
#pragma unroll
        for (int tt = 0; tt < 3; ++tt) {
            if (t0 + tt < K) {
                const float tap = taps[t0 + tt];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(tap, w[tt + j], acc[j]);
            }
        }
    }
}

// G(src) on the tile at (oy0, ox0) of one H x W plane.  Thread tid ends with its eight outputs acc[g][j] at tile row
// (tid >> 5) * 8 + 4 g + j, tile column tid & 31; s_in keeps the staged source tile (row stride LW, the tile's origin at [K/2][K/2]).
__device__ __forceinline__ void blur_tile(const float* __restrict__ src, const float* __restrict__ taps, int K, int H, int W, int oy0,
                                          int ox0, float* smem, float (&acc)[2][4]) {
    const int LH = TH + K - 1, CW = TW + K - 1, half = K / 2;
    float* const s_in = smem;                             // [LH][LW]
    float* const s_row = smem + LH * LW;                  // [LH][TW]
    int* const s_idx = (int*)(s_row + LH * TW);           // [LH] source rows, then [CW] source columns
    const int tid = threadIdx.x;

    for (int i = tid; i < LH + CW; i += NT) s_idx[i] = i < LH ? reflect101(oy0 - half + i, H) : reflect101(ox0 - half + i - LH, W);
    __syncthreads();

    {
        const int lane = tid & 31;
        int ix[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) ix[k] = lane + 32 * k < CW ? s_idx[LH + lane + 32 * k] : -1;
        for (int r = tid >> 5; r < LH; r += NT / 32) {
            const float* const row = src + (int64_t)s_idx[r] * W;
            float v[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = ix[k] >= 0 ? row[ix[k]] : 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) s_in[r * LW + lane + 32 * k] = v[k];      // columns CW .. LW-1 hold zeros
        }
    }
    __syncthreads();

    for (int r = tid >> 3; r < LH; r += NT / 8) {
        const float* const p = s_in + r * LW + 4 * (tid & 7);
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        chain4(taps, K, [&](int i) { return *reinterpret_cast<const f4*>(p + 4 * i); }, a);
        *reinterpret_cast<f4*>(s_row + r * TW + 4 * (tid & 7)) = f4{a[0], a[1], a[2], a[3]};
    }
    __syncthreads();

    const float* const col = s_row + (tid & 31);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int yb = (tid >> 5) * 8 + 4 * g;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[g][j] = 0.f;
        chain4(taps, K, [&](int i) {
            f4 v;                                          // the read-ahead past the last row is clamped; those values feed no tap
            v.x = col[min(yb + 4 * i + 0, LH - 1) * TW];
            v.y = col[min(yb + 4 * i + 1, LH - 1) * TW];
            v.z = col[min(yb + 4 * i + 2, LH - 1) * TW];
            v.w = col[min(yb + 4 * i + 3, LH - 1) * TW];
            return v;
        }, acc[g]);
    }
}

struct Tile {
    int64_t plane_off;      // first element of the (n, c) plane
    int oy0, ox0;
};

__device__ __forceinline__ Tile tile_of_block(const Params& p) {
    const int tiles = p.ntx * p.nty;
    const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
    Tile r;
    r.plane_off = (int64_t)plane * p.H * p.W;
    r.oy0 = (t / p.ntx) * TH;
    r.ox0 = (t % p.ntx) * TW;
    return r;
}

// x -> blur, mask
__global__ __launch_bounds__(NT) void usm_blur_mask_kernel(Params p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Tile t = tile_of_block(p);
    float acc[2][4];
    blur_tile(p.x + t.plane_off, p.taps, p.K, p.H, p.W, t.oy0, t.ox0, smem, acc);
    const int half = p.K / 2, lx = threadIdx.x & 31, ox = t.ox0 + lx;
    if (ox >= p.W) return;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ly = (threadIdx.x >> 5) * 8 + 4 * g + j, oy = t.oy0 + ly;
            if (oy >= p.H) continue;
            const float xv = smem[(ly + half) * LW + lx + half];
            const float res = __fsub_rn(xv, acc[g][j]);
            const int64_t o = t.plane_off + (int64_t)oy * p.W + ox;
            p.blur[o] = acc[g][j];
            p.mask[o] = __fmul_rn(fabsf(res), 255.0f) > p.threshold ? 1.0f : 0.0f;
        }
}

// mask -> soft; x, blur, soft -> out.  The intrinsics keep every operation of the blend a rounding of its own under
// -ffp-contract=fast, so the plain and the quantised call see the same value.
__global__ __launch_bounds__(NT) void usm_blend_kernel(Params p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const Tile t = tile_of_block(p);
    float acc[2][4];
    blur_tile(p.mask + t.plane_off, p.taps, p.K, p.H, p.W, t.oy0, t.ox0, smem, acc);
    const int ox = t.ox0 + (threadIdx.x & 31);
    if (ox >= p.W) return;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int oy = t.oy0 + (threadIdx.x >> 5) * 8 + 4 * g + j;
            if (oy >= p.H) continue;
            const int64_t o = t.plane_off + (int64_t)oy * p.W + ox;
            const float xv = p.x[o], soft = acc[g][j];
            const float res = __fsub_rn(xv, p.blur[o]);
            const float sharp = fminf(fmaxf(__fadd_rn(xv, __fmul_rn(p.weight, res)), 0.f), 1.f);
            float v = __fadd_rn(__fmul_rn(soft, sharp), __fmul_rn(__fsub_rn(1.0f, soft), xv));
            if (p.quantise) {                             // grl_image_pack8's level, then to_tensor's division
                if (!(v > 0.f)) v = 0.f;
                if (v > 1.f) v = 1.f;
                v = __fdiv_rn(rintf(__fmul_rn(v, 255.0f)), 255.0f);
            }
            p.out[o] = v;
        }
}

// false: sizes the entry refuses
bool geometry(int32_t N, int32_t C, int32_t H, int32_t W, int64_t* elems, int64_t* grid, int32_t* ntx, int32_t* nty) {
    if (N <= 0 || (C != 1 && C != 3) || H <= 0 || W <= 0 || H > (1 << 30) || W > (1 << 30)) return false;
    const int64_t tx = ((int64_t)W + TW - 1) / TW, ty = ((int64_t)H + TH - 1) / TH, planes = (int64_t)N * C;
    if (tx * ty > 0x7fffffff || planes * tx * ty > 0x7fffffff) return false;
    *elems = planes * H * W;
    *grid = planes * tx * ty;
    *ntx = (int32_t)tx;
    *nty = (int32_t)ty;
    return true;
}

}  // namespace

extern "C" int64_t grl_usm_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
    int64_t elems, grid;
    int32_t ntx, nty;
    if (!geometry(N, C, H, W, &elems, &grid, &ntx, &nty)) return GRL_ERR_BAD_ARG;
    return 2 * elems * (int64_t)sizeof(float);
}

extern "C" int grl_usm_sharp(void* stream, const GrlUsmArgs* a) {
    if (!a || !a->x || !a->taps || !a->workspace || !a->out) return GRL_ERR_BAD_ARG;
    if (a->K < 1 || a->K > KMAX || a->K % 2 == 0) return GRL_ERR_BAD_ARG;
    int64_t elems, grid;
    Params p;
    if (!geometry(a->N, a->C, a->H, a->W, &elems, &grid, &p.ntx, &p.nty)) return GRL_ERR_BAD_ARG;
    if ((uint64_t)a->x % 4 || (uint64_t)a->taps % 4 || (uint64_t)a->workspace % 4 || (uint64_t)a->out % 4) return GRL_ERR_BAD_ARG;

    p.x = a->x; p.taps = a->taps; p.out = a->out;
    p.blur = (float*)a->workspace;
    p.mask = p.blur + elems;
    p.weight = a->weight; p.threshold = a->threshold;
    p.K = a->K; p.H = a->H; p.W = a->W; p.quantise = a->quantise != 0;
    const int LH = TH + a->K - 1, CW = TW + a->K - 1;
    const size_t lds = (size_t)(LH * (LW + TW) + LH + CW) * sizeof(float);

    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(usm_blur_mask_kernel, dim3((unsigned)grid), dim3(NT), lds, st, p);
    GRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(usm_blend_kernel, dim3((unsigned)grid), dim3(NT), lds, st, p);
    GRL_CHECK_LAUNCH();
    return 0;
}
