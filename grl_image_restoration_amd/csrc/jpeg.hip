// JPEG compression and decompression of an image batch (include/grl_hip.h, grl_jpeg_roundtrip): the LQ synthesis of the JPEG
// artifact-removal task, the reference's ``cv2.imencode(".jpg", img, [IMWRITE_JPEG_QUALITY, q])`` + ``cv2.imdecode``
// (data/datasets/restoration_jpeg.py:62-79).  The entropy coding of JPEG is lossless, so the decoded image depends only on the
// colour conversion, the 2 x 2 chroma down- and up-sampling and the 8 x 8 DCT / quantisation / inverse DCT.  All of that is
// libjpeg's block-local integer arithmetic (jccolor.c, jcsample.c h2v2_downsample, jfdctint.c, jcdctmgr.c, jidctint.c,
// jdsample.c h2v2_fancy_upsample, jdcolor.c) and is restated here operation for operation in int32, which libjpeg's fixed-point
// design never leaves: the result equals libjpeg-turbo's with its defaults (4:2:0, JDCT_ISLOW, baseline tables, fancy
// upsampling) in every byte.
//
// Kernel 1, the block pass.  Work item = one 8 x 8 block of one component of one sample, handled by EIGHT lanes (eight blocks per
// wave64, 32 per workgroup of 256).  Lane l loads row l of the block: the loader converts fp32 k / 255 to the 8-bit level,
// replicates the image edge, and for the chroma planes converts four pixels to Cb (or Cr) and averages them (bias 1 / 2 by the
// parity of the output column).  A 1-D DCT pass runs on the eight values of a lane in registers; the transposition between the row
// pass and the column pass goes through LDS with a row stride of 9 dwords and a block stride of 72: ds_write_b32 / ds_read_b32 bank
// by (address / 4) % 32 within 32-lane halves, and (8 b + 9 l + j) % 32 (writes) and (8 b + l + 9 j) % 32 (reads) are distinct
// over b = 0 .. 3, l = 0 .. 7, so neither side conflicts.  The lane that holds column l quantises and dequantises its eight
// coefficients with the sample's table, built in LDS from its quality once per workgroup (a workgroup never spans two samples),
// runs the inverse column pass, transposes back and runs the inverse row pass, then stores its eight decoded samples as one
// 8-byte word into the component plane of the workspace.
//
// Kernel 2, the merge pass.  One thread per output pixel: the triangle-filter upsampling of Cb and Cr from the decoded planes
// (each output reads a 2 x 2 neighbourhood: weights 9, 3, 3, 1 over 16), YCbCr -> RGB, clamp, and float(v) / 255 by IEEE
// division for the three channels.  Planes of at most two chroma columns (images of at most four) are replicated instead, as
// libjpeg picks its plain upsampler there (jdsample.c: ``do_fancy && downsampled_width > 2``).  Gray copies and scales only.
#include "common.h"

namespace {

constexpr int NT = 256, BPG = NT / 8;       // threads and 8 x 8 blocks per workgroup
constexpr int LS = 9, BS = 8 * LS;          // LDS dwords per block row and per block

// JPEG Annex K, tables K.1 (luminance) and K.2 (chrominance), natural order
__device__ const uint8_t kStd[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

struct Geom {
    int32_t C, H, W;
    int32_t Hp, Wp;             // the Y (or gray) plane, multiples of 8
    int32_t h2, w2, Hc, Wc;     // the chroma planes: real size and size in whole blocks
    int32_t nY, nC;             // 8 x 8 blocks of the Y plane and of one chroma plane
    int32_t total, wgs;         // blocks and workgroups of one sample
    int64_t ws_stride;          // workspace bytes of one sample
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int level(float x) { return min(max(__float2int_rn(x * 255.f), 0), 255); }

// jfdctint.c, one 1-D pass.  FIRST: the row pass (outputs scaled up by 2 bits), else the column pass.
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
    constexpr int n = FIRST ? 11 : 15;
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2] = descale(z1 + t13 * 6270, n);
    d[6] = descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = descale(t4 + z1 + z3, n);
    d[5] = descale(t5 + z2 + z4, n);
    d[3] = descale(t6 + z2 + z3, n);
    d[1] = descale(t7 + z1 + z4, n);
}

// jidctint.c, one 1-D pass.  FIRST: the column pass (descale 11), else the row pass (descale 18).
template <bool FIRST>
__device__ __forceinline__ void idct8(int (&d)[8]) {
    constexpr int n = FIRST ? 11 : 18;
    int z1 = (d[2] + d[6]) * 4433;
    int t2 = z1 - d[6] * 15137, t3 = z1 + d[2] * 6270;
    int t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7]; t1 = d[5]; t2 = d[3]; t3 = d[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    d[0] = descale(t10 + t3, n); d[7] = descale(t10 - t3, n);
    d[1] = descale(t11 + t2, n); d[6] = descale(t11 - t2, n);
    d[2] = descale(t12 + t1, n); d[5] = descale(t12 - t1, n);
    d[3] = descale(t13 + t0, n); d[4] = descale(t13 - t0, n);
}

__device__ __forceinline__ int rgb_to(int comp, int r, int g, int b) {
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__global__ __launch_bounds__(NT) void jpeg_block_kernel(const float* __restrict__ x, const int32_t* __restrict__ quality,
                                                        uint8_t* __restrict__ ws, Geom g) {
    __shared__ int tile[BPG * BS];
    __shared__ int qt[2][64];

    const int n = blockIdx.x / g.wgs, w = blockIdx.x - n * g.wgs;
    if (threadIdx.x < 128) {
        const int q = min(max(quality[n], 1), 100);
        const int s = q < 50 ? 5000 / q : 200 - 2 * q;
        const int c = threadIdx.x >> 6, i = threadIdx.x & 63;
        qt[c][i] = min(max((kStd[c][i] * s + 50) / 100, 1), 255);
    }

    const int blk = threadIdx.x >> 3, l = threadIdx.x & 7;
    const int t = w * BPG + blk;
    const bool valid = t < g.total;                   // the last workgroup of a sample may hold fewer than 32 blocks
    int comp = 0, bi = t;
    if (t >= g.nY) { comp = t - g.nY >= g.nC ? 2 : 1; bi = t - g.nY - (comp - 1) * g.nC; }
    const int pw = comp ? g.Wc : g.Wp;                // plane width in samples
    const int by = valid ? bi / (pw >> 3) : 0, bx = valid ? bi - by * (pw >> 3) : 0;

    int d[8];
    if (valid) {
        const int64_t hw = (int64_t)g.H * g.W;
        const float* xn = x + (int64_t)n * g.C * hw;
        if (comp == 0) {
            const float* row = xn + (int64_t)min(by * 8 + l, g.H - 1) * g.W;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int xx = min(bx * 8 + j, g.W - 1);
                d[j] = g.C == 1 ? level(row[xx]) : rgb_to(0, level(row[xx]), level(row[hw + xx]), level(row[2 * hw + xx]));
            }
        } else {
            // rows of the small plane beyond h2 repeat row h2 - 1; the full-resolution plane is replicated to 2 h2 rows, 2 Wc columns
            const int r = min(by * 8 + l, g.h2 - 1);
            const float* row0 = xn + (int64_t)min(2 * r, g.H - 1) * g.W;
            const float* row1 = xn + (int64_t)min(2 * r + 1, g.H - 1) * g.W;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = bx * 8 + j;
                const int x0 = min(2 * c, g.W - 1), x1 = min(2 * c + 1, g.W - 1);
                const int a = rgb_to(comp, level(row0[x0]), level(row0[hw + x0]), level(row0[2 * hw + x0]));
                const int b = rgb_to(comp, level(row0[x1]), level(row0[hw + x1]), level(row0[2 * hw + x1]));
                const int e = rgb_to(comp, level(row1[x0]), level(row1[hw + x0]), level(row1[2 * hw + x0]));
                const int f = rgb_to(comp, level(row1[x1]), level(row1[hw + x1]), level(row1[2 * hw + x1]));
                d[j] = (a + b + e + f + 1 + (c & 1)) >> 2;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] -= 128;
        fdct8<true>(d);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) d[j] = 0;
    }

    // every thread takes part in the transpositions, so that the barriers are uniform; invalid lanes carry zeros
    int* const tb = tile + blk * BS;
#pragma unroll
    for (int j = 0; j < 8; ++j) tb[l * LS + j] = d[j];          // row l
    __syncthreads();                                            // also publishes qt
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = tb[j * LS + l];          // column l
    fdct8<false>(d);

    const int* const q = qt[comp ? 1 : 0];
#pragma unroll
    for (int j = 0; j < 8; ++j) {                               // coefficient (vertical j, horizontal l)
        const int qv = q[j * 8 + l], v = qv << 3;
        const int c = d[j];
        const unsigned m = (unsigned)(abs(c) + (v >> 1));
        const int k = m >= (unsigned)v ? (int)(m / (unsigned)v) : 0;
        d[j] = (c < 0 ? -k : k) * qv;
    }
    idct8<true>(d);
    __syncthreads();                                            // every lane has read its column
#pragma unroll
    for (int j = 0; j < 8; ++j) tb[j * LS + l] = d[j];          // column l
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = tb[l * LS + j];          // row l
    idct8<false>(d);

    if (valid) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo |= (uint32_t)min(max(d[j] + 128, 0), 255) << (8 * j);
            hi |= (uint32_t)min(max(d[j + 4] + 128, 0), 255) << (8 * j);
        }
        uint8_t* plane = ws + n * g.ws_stride;
        if (comp) plane += (int64_t)g.Hp * g.Wp + (int64_t)(comp - 1) * g.Hc * g.Wc;
        *reinterpret_cast<uint2*>(plane + (int64_t)(by * 8 + l) * pw + bx * 8) = make_uint2(lo, hi);
    }
}

constexpr int MW = 64, MH = NT / MW;        // the merge pass: a workgroup owns MH rows of MW pixels, one wave per row

__global__ __launch_bounds__(NT) void jpeg_merge_kernel(const uint8_t* __restrict__ ws, float* __restrict__ out, Geom g, int32_t tx,
                                                        int32_t ty) {
    const uint32_t per = (uint32_t)tx * (uint32_t)ty;
    const int n = (int)(blockIdx.x / per);
    const uint32_t t = blockIdx.x - (uint32_t)n * per;
    const int y = (int)(t / (uint32_t)tx) * MH + (int)(threadIdx.x / MW);
    const int xx = (int)(t % (uint32_t)tx) * MW + (int)(threadIdx.x % MW);
    if (y >= g.H || xx >= g.W) return;
    const int64_t hw = (int64_t)g.H * g.W, rem = (int64_t)y * g.W + xx;
    const uint8_t* py = ws + n * g.ws_stride;
    const int Y = py[(int64_t)y * g.Wp + xx];
    if (g.C == 1) {
        out[n * hw + rem] = __fdiv_rn((float)Y, 255.f);
        return;
    }
    const uint8_t* pb = py + (int64_t)g.Hp * g.Wp;
    const uint8_t* pr = pb + (int64_t)g.Hc * g.Wc;
    const int r = y >> 1, c = xx >> 1;
    const int64_t o0 = (int64_t)r * g.Wc;
    int cb, cr;
    if (g.w2 <= 2) {                                                // libjpeg's plain 2 x 2 replication
        cb = pb[o0 + c];
        cr = pr[o0 + c];
    } else {
        const int r2 = min(max((y & 1) ? r + 1 : r - 1, 0), g.h2 - 1);
        const int c2 = min(max((xx & 1) ? c + 1 : c - 1, 0), g.w2 - 1);
        const int64_t o2 = (int64_t)r2 * g.Wc;
        const int bias = (xx & 1) ? 7 : 8;
        cb = (3 * (3 * pb[o0 + c] + pb[o2 + c]) + 3 * pb[o0 + c2] + pb[o2 + c2] + bias) >> 4;
        cr = (3 * (3 * pr[o0 + c] + pr[o2 + c]) + 3 * pr[o0 + c2] + pr[o2 + c2] + bias) >> 4;
    }
    cb -= 128;
    cr -= 128;
    const int R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
    const int G = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
    const int B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
    float* o = out + n * 3 * hw + rem;
    o[0] = __fdiv_rn((float)R, 255.f);
    o[hw] = __fdiv_rn((float)G, 255.f);
    o[2 * hw] = __fdiv_rn((float)B, 255.f);
}

// false: sizes that the entry points reject
bool geometry(int32_t N, int32_t C, int32_t H, int32_t W, Geom* g) {
    if (N <= 0 || (C != 1 && C != 3) || H <= 0 || W <= 0 || H > 0x7ffffff0 || W > 0x7ffffff0) return false;
    g->C = C; g->H = H; g->W = W;
    g->Hp = (H + 7) / 8 * 8; g->Wp = (W + 7) / 8 * 8;
    g->h2 = (H + 1) / 2; g->w2 = (W + 1) / 2;
    g->Hc = (g->h2 + 7) / 8 * 8; g->Wc = (g->w2 + 7) / 8 * 8;
    const int64_t nY = (int64_t)(g->Hp / 8) * (g->Wp / 8), nC = C == 3 ? (int64_t)(g->Hc / 8) * (g->Wc / 8) : 0;
    const int64_t total = nY + 2 * nC;
    if (total > 0x7fffffff) return false;
    g->nY = (int32_t)nY; g->nC = (int32_t)nC; g->total = (int32_t)total;
    g->wgs = (int32_t)((total + BPG - 1) / BPG);
    g->ws_stride = total * 64;
    return true;
}

}  // namespace

extern "C" int64_t grl_jpeg_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
    Geom g;
    if (!geometry(N, C, H, W, &g)) return GRL_ERR_BAD_ARG;
    return g.ws_stride * N;
}

extern "C" int grl_jpeg_roundtrip(void* stream, const GrlJpegArgs* a) {
    if (!a || !a->x || !a->quality || !a->workspace || !a->out) return GRL_ERR_BAD_ARG;
    Geom g;
    if (!geometry(a->N, a->C, a->H, a->W, &g)) return GRL_ERR_BAD_ARG;
    if ((uint64_t)a->x % 4 || (uint64_t)a->out % 4 || (uint64_t)a->quality % 4 || (uint64_t)a->workspace % 8) return GRL_ERR_BAD_ARG;
    const int64_t tx = (a->W + MW - 1) / MW, ty = (a->H + MH - 1) / MH;
    const int64_t grid1 = (int64_t)a->N * g.wgs;
    if (grid1 > 0x7fffffff || tx * ty > 0x7fffffff || tx * ty * a->N > 0x7fffffff) return GRL_ERR_BAD_ARG;
    const int64_t grid2 = tx * ty * a->N;

    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_block_kernel, dim3((unsigned)grid1), dim3(NT), 0, st, a->x, a->quality, (uint8_t*)a->workspace, g);
    GRL_CHECK_LAUNCH();
    hipLaunchKernelGGL(jpeg_merge_kernel, dim3((unsigned)grid2), dim3(NT), 0, st, (const uint8_t*)a->workspace, a->out, g, (int32_t)tx,
                       (int32_t)ty);
    GRL_CHECK_LAUNCH();
    return 0;
}
