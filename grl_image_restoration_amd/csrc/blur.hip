// Depthwise blur of the non-blind deblurring task (include/grl_hip.h, grl_blur_depthwise): the reference's
// ``input_ += F.conv2d(target, blur_kernel, groups=3, padding=(bkh, bkw))`` (engines/base.py:131-142), with the training branch's
// crop ``[bkh:-bkh, bkw:-bkw]`` of input and target folded in.
//
//   acc(oy, ox) = sum over ky = 0 .. K-1 (outer), kx = 0 .. K-1 (inner) of taps[ky][kx] * x[oy - pad + ky][ox - pad + kx]
//   out(oy, ox) = fl32(acc) + add(oy, ox)
// x reads as 0 outside the image.  pad = K / 2: output H x W (zero padding, validation); pad = 0: output (H-K+1) x (W-K+1) (the valid
// region, training), and `center` receives x[oy + K/2][ox + K/2].  One K x K tap table serves every plane (the reference repeats its
// kernel over the three channels).  The sum is one fp32 fmaf chain per output, started at 0, in the order above: the result does not
// depend on the tiling, the launch or the run, and a `valid` output equals the `same` output at the same place bitwise.
//
// Shape: a workgroup of 256 threads owns a TH x TW = 32 x 64 output tile of one (n, c) plane and stages the (TH+K-1) x (TW+K-1)
// input tile it reads in LDS (strided global reads, all issued before the first LDS write; zeros outside the image).  A lane
// produces R = 8 adjacent outputs of one row: per tap row it reads its R+K-1 input values, rounded up to whole float4, with
// ds_read_b128 only into a register window and issues K x R fmaf on it as K x R / 2 v_pk_fma_f32, every tap a wave-uniform value
// read from device memory through the scalar cache.  At K = 25 that is 8 LDS reads of 16 B and 23 register moves (the 15 odd pairs) per 100 packed
// fmaf (0.16 LDS dwords per fmaf).  The reads are volatile so that the compiler keeps them whole: left alone it re-reads the
// odd-aligned pairs with ds_read2_b32, which at a lane stride of 8 dwords is an 8-way bank conflict and made the LDS, not the
// VALU, the limit (104 us instead of 48 us at 720p).  K is a template parameter (the 16 odd sizes 1 .. 31), so the window is
// indexed at compile time and stays in registers.  The taps are never copied to __constant__ memory and the host does not
// synchronise: the launch can be captured.  Ragged tiles stage zeros (or in-range neighbours) beyond the image and store only
// their own outputs.
#include "common.h"

namespace {

constexpr int TW = 64, TH = 32, R = 8, NT = 256;
constexpr int LANES_X = TW / R;
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef const volatile __attribute__((address_space(3))) f4* lds_f4;      // an LDS pointer that stays one (a volatile generic one would load flat)
static_assert(LANES_X * TH == NT, "one lane per R outputs of the tile");

struct Params {
    const float* x;
    const float* taps;
    const float* add;
    float* out;
    float* center;
    int64_t sn, sc, sh, sw;       // element strides of x
    int64_t an, ac, ah;           // element strides of add (unit column stride)
    int32_t C, H, W, Ho, Wo, pad, ntx, nty;
    int32_t vec;                  // Wo % 4 == 0 and out / center 16-byte aligned: whole rows of 8 go out as two float4
};

template <int K>
__global__ __launch_bounds__(NT) void blur_depthwise_kernel(Params p) {
    constexpr int WIN = (R + K - 1 + 3) / 4 * 4;      // register window of a lane, whole float4
    constexpr int LW = TW - R + WIN;                  // LDS row: the last lane's window ends at the row's end
    constexpr int LH = TH + K - 1;
    __shared__ __attribute__((aligned(16))) float s[LH * LW];

    const int tiles = p.ntx * p.nty;
    const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
    const int n = plane / p.C, c = plane - n * p.C;
    const int oy0 = (t / p.ntx) * TH, ox0 = (t % p.ntx) * TW;
    const float* const xp = p.x + n * p.sn + c * p.sc;

    // every global read of the tile is issued before the first LDS write, so that their latencies overlap (the trip count is a
    // compile-time constant: 20 values per thread at K = 25)
    constexpr int NLOAD = (LH * LW + NT - 1) / NT;
    float stage[NLOAD];
#pragma unroll
    for (int j = 0; j < NLOAD; ++j) {
        const int i = threadIdx.x + j * NT;
        const int r = i / LW, q = i - r * LW;
        const int y = oy0 - p.pad + r, xx = ox0 - p.pad + q;
        float v = 0.f;
        if (i < LH * LW && (uint32_t)y < (uint32_t)p.H && (uint32_t)xx < (uint32_t)p.W) v = xp[y * p.sh + xx * p.sw];
        stage[j] = v;
    }
#pragma unroll
    for (int j = 0; j < NLOAD; ++j) {
        const int i = threadIdx.x + j * NT;
        if (i < LH * LW) s[i] = stage[j];
    }
    __syncthreads();

    const int ly = threadIdx.x / LANES_X, lx = (threadIdx.x % LANES_X) * R;
    const int oy = oy0 + ly, ox = ox0 + lx;
    if (oy >= p.Ho || ox >= p.Wo) return;

    // Packed arithmetic: outputs (2h, 2h+1) share one v_pk_fma_f32.  Tap kx of them reads the window pair that starts at kx + 2h:
    // an even start is a register pair of the float4 reads as they are (ev), an odd one is made once per row by a register move
    // (od).  Every output still gets the same fmaf chain, tap by tap.
    f2 acc[R / 2];
#pragma unroll
    for (int h = 0; h < R / 2; ++h) acc[h] = f2{0.f, 0.f};
    const float* row = s + ly * LW + lx;
    const float* __restrict__ w = p.taps;
#pragma unroll 1
    for (int ky = 0; ky < K; ++ky, row += LW, w += K) {
        f2 ev[WIN / 2], od[WIN / 2 - 1];
#pragma unroll
        for (int j = 0; j < WIN / 4; ++j) {
            const f4 v = *(lds_f4)(row + 4 * j);                  // volatile: one ds_read_b128, not re-read piecewise
            ev[2 * j] = f2{v.x, v.y};
            ev[2 * j + 1] = f2{v.z, v.w};
        }
#pragma unroll
        for (int j = 0; j < WIN / 2 - 1; ++j) od[j] = f2{ev[j].y, ev[j + 1].x};
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const float wk = w[kx];
            const f2 w2 = f2{wk, wk};
#pragma unroll
            for (int h = 0; h < R / 2; ++h) {
                const int o = kx + 2 * h;
                acc[h] = __builtin_elementwise_fma(w2, (o & 1) ? od[o / 2] : ev[o / 2], acc[h]);
            }
        }
    }
    float out8[R];
#pragma unroll
    for (int h = 0; h < R / 2; ++h) { out8[2 * h] = acc[h].x; out8[2 * h + 1] = acc[h].y; }

    const int64_t o = (((int64_t)plane * p.Ho) + oy) * p.Wo + ox;
    const bool whole = ox + R <= p.Wo;
    if (p.add) {
        const float* a = p.add + n * p.an + c * p.ac + oy * p.ah + ox;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (whole || ox + r < p.Wo) out8[r] += a[r];
    }
    if (p.vec && whole) {
        float4* d = reinterpret_cast<float4*>(p.out + o);
        d[0] = make_float4(out8[0], out8[1], out8[2], out8[3]);
        d[1] = make_float4(out8[4], out8[5], out8[6], out8[7]);
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (ox + r < p.Wo) p.out[o + r] = out8[r];
    }
    if (p.center) {                                   // pad = 0: the centre of the staged tile is the cropped input
        const float* m = s + (ly + K / 2) * LW + lx + K / 2;
        if (p.vec && whole) {
            float4* d = reinterpret_cast<float4*>(p.center + o);
            d[0] = make_float4(m[0], m[1], m[2], m[3]);
            d[1] = make_float4(m[4], m[5], m[6], m[7]);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (ox + r < p.Wo) p.center[o + r] = m[r];
        }
    }
}

template <int K>
void launch(const Params& p, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((blur_depthwise_kernel<K>), dim3(grid), dim3(NT), 0, st, p);
}

}  // namespace

extern "C" int grl_blur_depthwise(void* stream, const GrlBlurArgs* a) {
    if (!a || !a->x || !a->taps || !a->out) return GRL_ERR_BAD_ARG;
    const int32_t K = a->K, pad = a->pad;
    if (K < 1 || K > 31 || K % 2 == 0) return GRL_ERR_BAD_ARG;
    if (pad != 0 && pad != K / 2) return GRL_ERR_BAD_ARG;
    if (a->N <= 0 || a->C <= 0 || a->H <= 0 || a->W <= 0) return GRL_ERR_BAD_ARG;
    if (pad == 0 && (a->H < K || a->W < K)) return GRL_ERR_BAD_ARG;
    if (a->center && pad != 0) return GRL_ERR_BAD_ARG;
    if ((uint64_t)a->x % 4 || (uint64_t)a->taps % 4 || (uint64_t)a->out % 4 || (uint64_t)a->add % 4 || (uint64_t)a->center % 4)
        return GRL_ERR_BAD_ARG;
    const int32_t Ho = a->H + 2 * pad - K + 1, Wo = a->W + 2 * pad - K + 1;
    const int64_t ntx = (Wo + TW - 1) / TW, nty = (Ho + TH - 1) / TH;
    const int64_t planes = (int64_t)a->N * a->C;
    if (planes > 0x7fffffff || planes * ntx * nty > 0x7fffffff) return GRL_ERR_BAD_ARG;
    const int64_t grid = planes * ntx * nty;

    Params p;
    p.x = a->x; p.taps = a->taps; p.add = a->add; p.out = a->out; p.center = a->center;
    p.sn = a->stride[0]; p.sc = a->stride[1]; p.sh = a->stride[2]; p.sw = a->stride[3];
    p.an = a->add_stride[0]; p.ac = a->add_stride[1]; p.ah = a->add_stride[2];
    p.C = a->C; p.H = a->H; p.W = a->W; p.Ho = Ho; p.Wo = Wo; p.pad = pad; p.ntx = (int32_t)ntx; p.nty = (int32_t)nty;
    p.vec = Wo % 4 == 0 && (uint64_t)a->out % 16 == 0 && (uint64_t)a->center % 16 == 0;

    const hipStream_t st = (hipStream_t)stream;
    const unsigned g = (unsigned)grid;
    switch (K) {
        case 1: launch<1>(p, g, st); break;
        case 3: launch<3>(p, g, st); break;
        case 5: launch<5>(p, g, st); break;
        case 7: launch<7>(p, g, st); break;
        case 9: launch<9>(p, g, st); break;
        case 11: launch<11>(p, g, st); break;
        case 13: launch<13>(p, g, st); break;
        case 15: launch<15>(p, g, st); break;
        case 17: launch<17>(p, g, st); break;
        case 19: launch<19>(p, g, st); break;
        case 21: launch<21>(p, g, st); break;
        case 23: launch<23>(p, g, st); break;
        case 25: launch<25>(p, g, st); break;
        case 27: launch<27>(p, g, st); break;
        case 29: launch<29>(p, g, st); break;
        default: launch<31>(p, g, st); break;
    }
    GRL_CHECK_LAUNCH();
    return 0;
}
