// Backward of the cosine window / anchored-stripe attention (gfx950), flash-style: nothing of size Nq x Nk is stored.
//
// Replaces autograd through Attention.attn + AffineTransform (models/common/mixed_attn_block_efficient.py:36-58,77-94)
// inside WindowAttention / AnchorStripeAttention (:128-165, :215-270) in the reference's training step
// (engines/base.py:221-236).  Closed form (the tests check it against autograd), in the kernel's own operands
//   S_ij = q~_i . k^_j + table[idx(i,j)] (+ mask)        (log2 domain; q~ carries scale*log2e)
//   P_ij = exp2(S_ij - lse_i)                             (lse from the forward kernel)
//   D_i  = sum_c dO_ic O_ic          dP_ij = dO_i . v_j          dS_ij = ln2 * P_ij (dP_ij - D_i)
//   dv_j = sum_i P_ij dO_i     dq~_i = sum_j dS_ij k^_j     dk^_j = sum_i dS_ij q~_i     dtable[idx(i,j)] += dS_ij
// The gradients of the L2 normalisation, the logit scale and the CPB-MLP (table) are taken by the caller.
//
// Two kernels, both built like the generic forward kernel (any window shape, index arithmetic instead of partition / roll /
// mask / index tensors):
//   dq_kernel  : workgroup = (window, head, 256 queries); S^T = K.Q orientation (lane = query) exactly as the forward, keys
//                stream through LDS; 6 MFMAs per (32 keys x 32 queries) tile; dtable as an LDS histogram (ds_add_f32)
//                flushed with global atomics.  When both windows are whole multiples of 32 wide a (32 x 32) tile is one key-row
//                segment against one query-row segment, its table entries depend on (key - query) only, and the tile is
//                summed along its diagonals in registers first (rotating the wave one lane per key row, see diag_ring):
//                one conflict-free ds_add per tile instead of 16 two-way-conflicting ones.
//   dkv_kernel : workgroup = (window, head, 256 keys); S = Q.K^T orientation (lane = key), queries stream through LDS;
//                8 MFMAs per tile.
// dO is multiplied by g_scale on its way to fp16 (gradients of an L1 loss are ~1e-6: below the fp16 normal range); all
// outputs are un-scaled on store.
#include "common.h"
#include <stdlib.h>
#include <type_traits>
#include "grl_hip_internal.h"
#include "attn_common.h"

namespace {

// kernel argument block: GrlAttnBwdArgs + what the host derives per launch
struct GrlAttnBwdLaunch : GrlAttnBwdArgs {
    int32_t tab_window;      // floats of a table window in attn_dq_kernel's LDS (table and histogram)
    int32_t tab_window_kv;   // ... in attn_dkv_kernel's
};

constexpr int QT = 2;            // tiles (32 queries resp. keys) per wave
constexpr int KC = 128;          // streamed rows per LDS chunk
constexpr int TROW = KC * 2 + 8; // transposed staging: row stride in bytes
constexpr float LN2_F = 0.69314718055994531f;

// a [32-row][32 half] A-operand fragment pair from row-major swizzled LDS rows (64 B per row): rows = kb + l31,
// k-slots = columns 8*half (+16)
__device__ __forceinline__ void frag_rows(const char* base, int kb, int l31, int half, f16x8 (&f)[2]) {
    const int kk = kb + l31;
    const int sw = (kk >> 2) & 3;
    f[0] = *(const f16x8*)(base + kk * 64 + (((0 + half) ^ sw) << 4));
    f[1] = *(const f16x8*)(base + kk * 64 + (((2 + half) ^ sw) << 4));
}

// a [32 x 32-row] A-operand fragment pair from the TRANSPOSED staging [32 cols][TROW]: rows = column l31 of the source,
// k-slot e <-> source row kb + 16*s + 8*(e>>2) + 4*half + (e&3)  (the order the packed accumulator registers imply)
__device__ __forceinline__ void frag_cols(const char* base, int kb, int l31, int half, f16x8 (&f)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const char* vp = base + l31 * TROW + (kb + 16 * s + 4 * half) * 2;
        const f16x4 lo = *(const f16x4*)(vp);
        const f16x4 hi = *(const f16x4*)(vp + 16);
        f[s] = f16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
}

__device__ __forceinline__ void pack_acc(const f32x16& a, f16x8 (&o)[2]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r >> 3][r & 7] = to_f16(a[r]);
}

__device__ __forceinline__ f16x8 load_f16x8(const GrlTokenGrid& g, int64_t row, int head, int seg) {
    return *(const f16x8*)((const f16*)g.ptr + row * g.ld + g.col0 + head * g.hstride + seg * 8);
}

// dO lies on o's grid except, optionally, for its row stride (GrlAttnBwdArgs.d_o_ld: a column block of a wider gradient matrix)
__device__ __forceinline__ f16x8 load_do_as_f16(const GrlAttnBwdArgs& a, int64_t row, int head, int seg) {
    const GrlTokenGrid& g = a.fwd.o;
    const int64_t ld = a.d_o_ld > 0 ? a.d_o_ld : g.ld;
    const float4* q = (const float4*)(a.d_o + row * ld + g.col0 + head * g.hstride + seg * 8);
    const float4 a0 = q[0], a1 = q[1];
    const float scale = a.g_scale;
    f16x8 v;
    v[0] = to_f16(a0.x * scale); v[1] = to_f16(a0.y * scale); v[2] = to_f16(a0.z * scale); v[3] = to_f16(a0.w * scale);
    v[4] = to_f16(a1.x * scale); v[5] = to_f16(a1.y * scale); v[6] = to_f16(a1.z * scale); v[7] = to_f16(a1.w * scale);
    return v;
}

// store an accumulator in the (rows = head dim, cols = token) orientation to a [token][32] fp32 slot
__device__ __forceinline__ void store_cols(float* base, const GrlTokenGrid& g, int64_t row, int head, int half, const f32x16& a, float scale) {
    float* dst = base + row * g.ld + g.col0 + head * g.hstride + 4 * half;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *(float4*)(dst + 8 * q) = float4{a[4 * q + 0] * scale, a[4 * q + 1] * scale, a[4 * q + 2] * scale, a[4 * q + 3] * scale};
}

// Accumulation instead of a store (split launches: several workgroups hold partial sums of one token's row; the destination was
// zeroed) through a wave-private LDS tile, so that one atomic instruction covers two 128-byte rows instead of 64 different cache lines
// (with lane = token, rows 128 bytes apart, splitting the 384-workgroup launches in two cost +30 ms per training step).  ``off``: element offset of this lane's token row in the destination, -1 = no such token; ``w``: XWAVE bytes of LDS.
constexpr int XROW = 36;                               // floats per staged row: 16-byte aligned, rows 4 banks apart
constexpr int XWAVE = 32 * XROW * 4 + 32 * 8;          // tile + row offsets
__device__ __forceinline__ void add_cols_lds(float* base, int64_t off, int lane, const f32x16& a, float scale, char* w) {
    const int half = lane >> 5, l31 = lane & 31;
    float* tile = (float*)w;
    int64_t* rows = (int64_t*)(w + 32 * XROW * 4);
    if (half == 0) rows[l31] = off;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *(float4*)(tile + l31 * XROW + 8 * q + 4 * half) = float4{a[4 * q + 0] * scale, a[4 * q + 1] * scale, a[4 * q + 2] * scale, a[4 * q + 3] * scale};
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // (a wave's LDS operations execute in order; this keeps the compiler from moving them)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int tok = 2 * i + half;
        const float v = tile[tok * XROW + l31];
        const int64_t o = rows[tok];
        if (o >= 0) unsafeAtomicAdd(base + o + l31, v);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// wave_rol:1 -- lane i takes the value of lane (i + 1) mod 64
__device__ __forceinline__ float wave_rol1(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x134, 0xf, 0xf, true));
}

// Diagonal sums of a (32 keys x 32 queries) dS tile whose table entry is  ebase + key - query.
// The accumulator holds key row 8g + 4*half + m in register 4g + m, query = lane & 31.  v_permlane32_swap against zero
// (vdst lanes 32-63 <-> src lanes 0-31) splits a register into its two key rows, each in lanes 0-31 over zeros.  Then Horner from key row 31 down to 0 on one
// 64-lane ring: rotate the running sums one lane towards lane 0 (the entry of a value does not change, it now sits with
// the query one to the left; what leaves lane 0 re-enters at lane 63, and after 31 steps the spill has reached lane 33)
// and add the next row.  Lane p ends with the whole diagonal  key - query = -p  (p < 32)  or  64 - p  (p > 32): one
// conflict-free ds_add per tile instead of 16 two-way conflicting ones.
// First (4-aligned) reversed table entry the queries n0..n1 of a window can touch (attn_dq_kernel), and the same for the keys
// n0..n1 in attn_dkv_kernel; window_floats: an upper bound of the entries from there, for rows_spanned query (key) rows.
__host__ __device__ inline int dq_window_lo(const GrlAttnArgs& p, int n0, int n1, int D) {
    const int hqb = n1 / p.q.ww;
    (void)n0;
    const int lo = p.trows - 1 - ((hqb + p.k.wh - 1) * D + (p.q.ww - 1) + (p.k.ww - 1));
    return lo < 0 ? 0 : lo & ~3;
}
__host__ __device__ inline int dkv_window_lo(const GrlAttnArgs& p, int n0, int n1, int D) {
    const int hka = n0 / p.k.ww;
    (void)n1;
    const int lo = p.trows - 1 - ((p.k.wh - 1 - hka) * D + (p.k.ww - 1)) - ((p.q.wh - 1) * D + (p.q.ww - 1));
    return lo < 0 ? 0 : lo & ~3;
}
// floats of LDS that hold any workgroup's window: `blk` consecutive tokens of a window `ww` wide span at most
// (blk - 1) / ww + 2 rows (one less when rows divide the block), against `other_h` rows of the other side
inline int window_floats(int blk, int n, int ww, int wh, int other_h, int D, int trows) {
    int rows = (blk % ww == 0) ? blk / ww : (blk - 1) / ww + 2;
    if (rows > wh) rows = wh;
    (void)n;
    const int w = ((rows + other_h - 1) * D + D + 3 + 3) & ~3;
    const int full = (trows + 3) & ~3;
    return w < full ? w : full;
}

// deterministic mode: a value of the g_scale-d domain added as 64-bit fixed point (integer atomics commute)
__device__ __forceinline__ void fix_add(int64_t* dst, float v) {
    atomicAdd((unsigned long long*)dst, (unsigned long long)(long long)__float2ll_rn(v * 4294967296.0f));
}

template <bool GHIST>
__device__ __forceinline__ void diag_ring(const f32x16& dS, int lane, float* dtab, float* gtab, int64_t* ftab, int ebase, float inv_g) {
    float z = 0.f;
#pragma unroll
    for (int g = 3; g >= 0; --g) {
        // (inline asm: this toolchain's __builtin_amdgcn_permlane32_swap returns its first result twice; the s_nops are the
        // VALU-write -> swap and swap -> DPP-read wait states the compiler would otherwise place)
        float row_lo[4] = {dS[4 * g], dS[4 * g + 1], dS[4 * g + 2], dS[4 * g + 3]};   // -> key rows 8g + m     in lanes 0-31
        float row_hi[4] = {0.f, 0.f, 0.f, 0.f};                                        // -> key rows 8g + 4 + m in lanes 0-31
        asm("s_nop 1\n\t"
            "v_permlane32_swap_b32 %0, %4\n\t"
            "v_permlane32_swap_b32 %1, %5\n\t"
            "v_permlane32_swap_b32 %2, %6\n\t"
            "v_permlane32_swap_b32 %3, %7\n\t"
            "s_nop 1"
            : "+v"(row_lo[0]), "+v"(row_lo[1]), "+v"(row_lo[2]), "+v"(row_lo[3]),
              "+v"(row_hi[0]), "+v"(row_hi[1]), "+v"(row_hi[2]), "+v"(row_hi[3]));
#pragma unroll
        for (int m = 3; m >= 0; --m) z = wave_rol1(z) + row_hi[m];
#pragma unroll
        for (int m = 3; m >= 0; --m) z = wave_rol1(z) + row_lo[m];
    }
    const int e = ebase - (lane < 32 ? lane : lane - 64);
    if (lane != 32) {
        if constexpr (GHIST) {
            if (ftab) fix_add(ftab + e, z);
            else unsafeAtomicAdd(gtab + e, z * inv_g);
        } else atomicAdd(&dtab[e], z);
    }
}

// ------------------------------------------------------------------------------------------------
// dq + dtable
// ------------------------------------------------------------------------------------------------
// GHIST: the bias-table gradient goes straight to global memory with atomics (tables whose two LDS copies would not fit:
// 64x128 stripes with /2 anchors = 73 KB per copy); otherwise an LDS histogram flushed once per workgroup.
template <bool GHIST>
// ``splits`` > 1: the key loop is cut into that many parts, one workgroup each, and dQ is accumulated with atomics into a zeroed
// destination -- for launches with fewer workgroups than CUs (anchors -> stripe tokens at training batch sizes: 96 workgroups
// streaming 4096 keys each).
__global__ __launch_bounds__(256) void attn_dq_kernel(GrlAttnBwdLaunch a, int splits) {
    const GrlAttnArgs& p = a.fwd;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
    const int half = lane >> 5, l31 = lane & 31;
    const int Nq = p.q.wh * p.q.ww, Nk = p.k.wh * p.k.ww;
    const int qblk = (nthreads >> 6) * (QT * 32);
    const int nqs = (Nq + qblk - 1) / qblk;
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int sp = bid % splits; bid /= splits;
    const int qs = bid % nqs; bid /= nqs;
    const int head = bid % p.nh; bid /= p.nh;
    const int wx = bid % p.nwx; bid /= p.nwx;
    const int wy = bid % p.nwy;
    const int b = bid / p.nwy;
    const int D = p.q.ww + p.k.ww - 1;
    // Table WINDOW of this workgroup (round 6): its queries span the rows hqa..hqb of the query window, so the (reversed) entries it
    // can touch -- trows-1 - [(hq - hk + KH-1) * D + (wq - wk + KW-1)] over all keys -- are the contiguous range
    // [trows-1 - (hqb + KH-1) * D - (QW + KW - 2), trows-1 - hqa * D]: (hqb - hqa + KH) * D entries instead of the whole table
    // (stripe tokens -> anchors at 64x64 / 32x32: 3 325 of 9 025).  Table and histogram in LDS shrink from 2 x 36 KB to 2 x 13 KB:
    // three workgroups per CU instead of one.
    const int wlo = dq_window_lo(p, qs * qblk, min(Nq, (qs + 1) * qblk) - 1, D);
    const int tpad = a.tab_window;                     // floats per LDS copy (host: the largest window of the launch, multiple of 4)

    float* tab = (float*)smem;                         // tpad
    float* dtab = tab + tpad;                          // tpad (histogram; absent with GHIST)
    char* Ks = (char*)(dtab + (GHIST ? 0 : tpad));     // KC x 64 B   (rows = keys)
    char* Vs = Ks + KC * 64;                           // KC x 64 B
    char* Kt = Vs + KC * 64;                           // 32 x TROW   (rows = head dim)
    int* koff = (int*)(Kt + 32 * TROW);                // KC
    unsigned char* kreg = (unsigned char*)(koff + KC); // KC

    const int wn = min(tpad, ((p.trows + 3) & ~3) - wlo);              // entries of the window that exist (wlo is a multiple of 4)
    load_table(tab, p.table + (int64_t)head * p.tstride + wlo, wn, tid, nthreads);
    if constexpr (!GHIST)
        for (int i = tid; i < tpad; i += nthreads) dtab[i] = 0.f;
    float* gtab = a.d_table + (int64_t)head * p.tstride + wlo;         // (window-relative like tab / dtab)
    int64_t* ftab = a.d_table_fix ? a.d_table_fix + (int64_t)head * p.tstride + wlo : nullptr;
    const float inv_g = 1.0f / a.g_scale;

    const bool border = p.masked && ((p.q.shy > 0 && wy == p.nwy - 1) || (p.q.shx > 0 && wx == p.nwx - 1));
    // every (32 x 32) tile is a key-row segment against a query-row segment: table entry = U(query 0) + koff(key 0) + key - query
    const bool toeplitz = (p.q.ww & 31) == 0 && (p.k.ww & 31) == 0;
    const bool band16 = (p.k.shx & 15) == 0;

    int U[QT], idq[QT];
    int64_t qrow[QT];
    bool qvalid[QT];
    f16x8 qf[QT][2], dof[QT][2];
    f32x16 dQ[QT];
    float lse[QT], Dq[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        int n = qs * qblk + wave * (QT * 32) + t * 32 + l31;
        qvalid[t] = n < Nq;
        if (!qvalid[t]) n = Nq - 1;
        locate(p.q, b, wy, wx, n, qrow[t], idq[t]);
        const int hq = n / p.q.ww, wq = n - hq * p.q.ww;
        U[t] = p.trows - 1 - (hq * D + wq + (p.k.wh - 1) * D + (p.k.ww - 1)) - wlo;     // window-relative
        qf[t][0] = load_f16x8(p.q, qrow[t], head, half);
        qf[t][1] = load_f16x8(p.q, qrow[t], head, 2 + half);
        // slot 31 of q carries the forward kernel's running offset in registers only: in memory it is a pad column (0)
        dof[t][0] = load_do_as_f16(a, qrow[t], head, half);
        dof[t][1] = load_do_as_f16(a, qrow[t], head, 2 + half);
        // D_i = sum_c dO_ic O_ic (scaled like dO): this lane holds 16 of the 32 columns.  Taken from the SAME fp16-rounded dO the
        // MFMA contracts with v: dS = P (dO.v_j - D_i) is a small difference of two nearly equal numbers wherever the values of a
        // window resemble each other (stripe tokens -> anchors: v is the anchors' aggregate), and with D from the unrounded dO the
        // rounding error of dO -- the same for every key j of the row -- did not cancel: round 5 measured 13-32 % run-to-run
        // noise in dQ of those launches (an upstream 1e-7 flips fp16 roundings) and the bias-table gradient error above the bar.
        float d = 0.f;
        {
            const float* op = (const float*)p.o.ptr + qrow[t] * p.o.ld + p.o.col0 + head * p.o.hstride;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int c = 16 * s + 8 * half + e;
                    if (c < p.head_dim) d += op[c] * (float)dof[t][s][e];
                }
        }
        d += xhalf(d);
        Dq[t] = d;
        lse[t] = p.lse[(int64_t)head * p.lse_stride + qrow[t]];
#pragma unroll
        for (int r = 0; r < 16; ++r) dQ[t][r] = 0.f;
    }

    const int nchunks = (Nk + KC - 1) / KC;
    // Round 6: with the full 256 threads a chunk is two (key, 16-byte segment) items per thread, and their K / V loads for chunk ch + 1
    // are ISSUED before the tiles of chunk ch are computed (16 registers); the LDS stores follow behind the next barrier.  Before, every
    // chunk began with the full global-load latency in front of its first tile -- with one wave per SIMD nothing else covers it.
    const bool pre = nthreads == 256;
    const int ch_end = (sp + 1) * nchunks / splits;
    f16x8 pk[2], pv[2];
    int prid[2];
    auto chunk_load = [&](int ch) {
        const int k0 = ch * KC;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + j * 256;
            const int kk = i >> 2, seg = i & 3;
            const int n = k0 + kk;
            const bool valid = n < Nk;
            int64_t row;
            locate(p.k, b, wy, wx, valid ? n : 0, row, prid[j]);
            pk[j] = f16x8{0, 0, 0, 0, 0, 0, 0, 0}; pv[j] = pk[j];
            if (valid) {
                pk[j] = load_f16x8(p.k, row, head, seg);
                pv[j] = load_f16x8(p.v, row, head, seg);
            }
        }
    };
    auto stage_item = [&](int k0, int i, const f16x8& kv, const f16x8& vv, int rid) {
        const int kk = i >> 2, seg = i & 3;
        const int n = k0 + kk;
        const bool valid = n < Nk;
        *(f16x8*)(Ks + kk * 64 + ((seg ^ ((kk >> 2) & 3)) << 4)) = kv;
        *(f16x8*)(Vs + kk * 64 + ((seg ^ ((kk >> 2) & 3)) << 4)) = vv;
#pragma unroll
        for (int e = 0; e < 8; ++e) *(f16*)(Kt + (seg * 8 + e) * TROW + kk * 2) = kv[e];
        if (seg == 0) {
            const int nn = valid ? n : 0;
            const int hk = nn / p.k.ww, wk = nn - hk * p.k.ww;
            koff[kk] = hk * D + wk;
            kreg[kk] = valid ? (unsigned char)rid : (unsigned char)255;
        }
    };
    if (pre && sp * nchunks / splits < ch_end) chunk_load(sp * nchunks / splits);
    for (int ch = sp * nchunks / splits; ch < ch_end; ++ch) {
        const int k0 = ch * KC;
        const int klen = min(KC, Nk - k0);
        const int ntiles = (klen + 31) >> 5;
        __syncthreads();
        if (pre) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (tid + j * 256 < ntiles * 32 * 4) stage_item(k0, tid + j * 256, pk[j], pv[j], prid[j]);
            if (ch + 1 < ch_end) chunk_load(ch + 1);       // in flight while this chunk's tiles are computed
        } else {
            for (int i = tid; i < ntiles * 32 * 4; i += nthreads) {
                const int kk = i >> 2, seg = i & 3;
                const int n = k0 + kk;
                const bool valid = n < Nk;
                int64_t row; int rid;
                locate(p.k, b, wy, wx, valid ? n : 0, row, rid);
                f16x8 kv = {0, 0, 0, 0, 0, 0, 0, 0}, vv = kv;
                if (valid) {
                    kv = load_f16x8(p.k, row, head, seg);
                    vv = load_f16x8(p.v, row, head, seg);
                }
                stage_item(k0, i, kv, vv, rid);
            }
        }
        __syncthreads();

        for (int kt = 0; kt < ntiles; ++kt) {
            const int kb = kt * 32;
            f16x8 kf[2], vf[2], ktf[2];
            frag_rows(Ks, kb, l31, half, kf);
            frag_rows(Vs, kb, l31, half, vf);
            frag_cols(Kt, kb, l31, half, ktf);
            // PLAIN (compile-time tag): Toeplitz geometry and no shift mask -- every key of the tile is valid and unmasked, and the
            // bias of (query lane, key row i) is tab[U + koff(key 0) + i]: ascending LDS reads at constant offsets instead of
            // 16 key-offset + 16 region-id look-ups per tile.  (A run-time `if` inside the element loop would merge the two
            // versions of dS in 16 register copies per tile.)
            // MODE 2: the same geometry with a shift mask whose key-column bands are 16 wide (shift % 16 == 0): keys 0..15 of the
            // tile (accumulator registers 0..7) share one region label, keys 16..31 another -- two look-ups and two selects.
            auto tile = [&](auto mode_tag) {
                constexpr int MODE = decltype(mode_tag)::value;
                constexpr bool PLAIN = MODE != 0;
                int kofs[16];
                if constexpr (!PLAIN) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) kofs[r] = koff[kb + mfma32_row(r, half)];
                }
                const int kbase = koff[kb];
                int id_lo = 0, id_hi = 0;
                if constexpr (MODE == 2) { id_lo = kreg[kb]; id_hi = kreg[kb + 16]; }
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    f32x16 S, dP;
                    if constexpr (PLAIN) {
                        const float* tp = tab + (U[t] + kbase + 4 * half);
#pragma unroll
                        for (int r = 0; r < 16; ++r) { S[r] = tp[(r & 3) + 8 * (r >> 2)]; dP[r] = 0.f; }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) { S[r] = tab[U[t] + kofs[r]]; dP[r] = 0.f; }
                    }
                    S = mfma32_f16(kf[0], qf[t][0], S);
                    S = mfma32_f16(kf[1], qf[t][1], S);
                    dP = mfma32_f16(vf[0], dof[t][0], dP);
                    dP = mfma32_f16(vf[1], dof[t][1], dP);
                    f32x16 dS;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float s = S[r];
                        if constexpr (!PLAIN) {
                            const int idk = kreg[kb + mfma32_row(r, half)];
                            if (idk == 255) s = NEG_BIG;
                            else if (border && idk != idq[t]) s += MASK_L2;
                            const float pr = __builtin_amdgcn_exp2f(s - lse[t]);
                            dS[r] = LN2_F * pr * (dP[r] - Dq[t]);
                            if (!toeplitz && qvalid[t] && idk != 255) {
                                if constexpr (GHIST) {
                                    if (ftab) fix_add(ftab + U[t] + kofs[r], dS[r]);
                                    else unsafeAtomicAdd(gtab + U[t] + kofs[r], dS[r] * inv_g);
                                } else atomicAdd(&dtab[U[t] + kofs[r]], dS[r]);
                            }
                        } else {
                            if constexpr (MODE == 2) s += (r < 8 ? id_lo : id_hi) != idq[t] ? MASK_L2 : 0.f;
                            const float pr = __builtin_amdgcn_exp2f(s - lse[t]);
                            dS[r] = LN2_F * pr * (dP[r] - Dq[t]);
                        }
                    }
                    f16x8 dsp[2];
                    pack_acc(dS, dsp);
                    dQ[t] = mfma32_f16(ktf[0], dsp[0], dQ[t]);
                    dQ[t] = mfma32_f16(ktf[1], dsp[1], dQ[t]);
                    // masked pairs carry dS = 0 exactly; there are no pad rows in this geometry.  A clamped (invalid) query tile --
                    // Nq % 64 == 32: the last wave's second tile repeats query Nq - 1 -- must not reach the table gradient
                    // (qvalid is wave-uniform per tile here: query tiles are whole 32-wide row segments)
                    if (toeplitz && __builtin_amdgcn_readfirstlane((int)qvalid[t]))
                        diag_ring<GHIST>(dS, lane, dtab, gtab, ftab, __builtin_amdgcn_readfirstlane(U[t]) + kbase, inv_g);
                }
            };
            if (toeplitz && !border) tile(std::integral_constant<int, 1>{});
            else if (toeplitz && band16) tile(std::integral_constant<int, 2>{});
            else tile(std::integral_constant<int, 0>{});
        }
    }

    const float inv = 1.0f / a.g_scale;
    // slot 31 of k holds 1.0 for the forward kernel's offset (see attn_dkv_kernel): against it dQ's column 31 collects sum_j dS_ij,
    // zero only up to the fp16 rounding of dS.  It is a pad column: it carries no gradient (register 15 of the upper half-wave)
    if (half && p.head_dim <= 30) {
#pragma unroll
        for (int t = 0; t < QT; ++t) dQ[t][15] = 0.f;
    }
#pragma unroll
    for (int t = 0; t < QT; ++t)
        if (splits == 1 && qvalid[t]) store_cols(a.d_q, p.q, qrow[t], head, half, dQ[t], inv);
    if (splits > 1) {          // (uniform) partial sums of a split launch: the K / V chunk buffers are free now
        __syncthreads();
#pragma unroll
        for (int t = 0; t < QT; ++t)
            add_cols_lds(a.d_q, qvalid[t] ? qrow[t] * p.q.ld + p.q.col0 + (int64_t)head * p.q.hstride : -1, lane, dQ[t], inv, Ks + wave * XWAVE);
    }
    if constexpr (!GHIST) {
        __syncthreads();
        for (int i = tid; i < wn; i += nthreads) {
            const float v = dtab[i];
            if (v != 0.f) {
                if (ftab) fix_add(ftab + i, v);
                else unsafeAtomicAdd(gtab + i, v * inv);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// dk + dv
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void attn_dkv_kernel(GrlAttnBwdLaunch a, int splits) {
    const GrlAttnArgs& p = a.fwd;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
    const int half = lane >> 5, l31 = lane & 31;
    const int Nq = p.q.wh * p.q.ww, Nk = p.k.wh * p.k.ww;
    const int kblk = (nthreads >> 6) * (QT * 32);
    const int nks = (Nk + kblk - 1) / kblk;
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int sp = bid % splits; bid /= splits;
    const int ks = bid % nks; bid /= nks;
    const int head = bid % p.nh; bid /= p.nh;
    const int wx = bid % p.nwx; bid /= p.nwx;
    const int wy = bid % p.nwy;
    const int b = bid / p.nwy;
    const int D = p.q.ww + p.k.ww - 1;
    // table window of this workgroup's keys (see attn_dq_kernel): entries Uk - (hq * D + wq) over all queries
    const int wlo = dkv_window_lo(p, ks * kblk, min(Nk, (ks + 1) * kblk) - 1, D);
    const int tpad = a.tab_window_kv;

    float* tab = (float*)smem;                         // tpad
    char* Qs = (char*)(tab + tpad);                    // KC x 64 B   (rows = queries)
    char* Gs = Qs + KC * 64;                           // KC x 64 B   dO rows (scaled fp16)
    char* Qt = Gs + KC * 64;                           // 32 x TROW   (rows = head dim)
    char* Gt = Qt + 32 * TROW;                         // 32 x TROW
    float* qlse = (float*)(Gt + 32 * TROW);            // KC
    float* qD = qlse + KC;                             // KC
    int* qoff = (int*)(qD + KC);                       // KC
    unsigned char* qreg = (unsigned char*)(qoff + KC); // KC

    load_table(tab, p.table + (int64_t)head * p.tstride + wlo, min(tpad, ((p.trows + 3) & ~3) - wlo), tid, nthreads);

    const bool border = p.masked && ((p.q.shy > 0 && wy == p.nwy - 1) || (p.q.shx > 0 && wx == p.nwx - 1));

    // Toeplitz geometry (both windows whole multiples of 32 wide: no pad rows, a tile is one row segment) and no shift mask
    const bool toeplitz = (p.q.ww & 31) == 0 && (p.k.ww & 31) == 0;
    const bool plain = toeplitz && !border;
    const bool band16 = (p.q.shx & 15) == 0;

    int Uk[QT], idk[QT];
    int64_t krow[QT];
    bool kvalid[QT];
    f16x8 kfb[QT][2], vfb[QT][2];
    f32x16 dK[QT], dV[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        int n = ks * kblk + wave * (QT * 32) + t * 32 + l31;
        kvalid[t] = n < Nk;
        if (!kvalid[t]) n = Nk - 1;
        locate(p.k, b, wy, wx, n, krow[t], idk[t]);
        const int hk = n / p.k.ww, wk = n - hk * p.k.ww;
        // reversed table entry of (query (hq, wq), key (hk, wk)) = trows-1 - [(hq-hk+KH-1)*D + (wq-wk+KW-1)] = Uk - (hq*D + wq)
        Uk[t] = p.trows - 1 - ((p.k.wh - 1 - hk) * D + (p.k.ww - 1 - wk)) - wlo;       // window-relative
        kfb[t][0] = load_f16x8(p.k, krow[t], head, half);
        kfb[t][1] = load_f16x8(p.k, krow[t], head, 2 + half);
        if (half && p.head_dim <= 30) kfb[t][1][7] = (f16)0.f;   // slot 31 of k holds 1.0 for the forward kernel's offset: not part of the logit
        vfb[t][0] = load_f16x8(p.v, krow[t], head, half);
        vfb[t][1] = load_f16x8(p.v, krow[t], head, 2 + half);
#pragma unroll
        for (int r = 0; r < 16; ++r) { dK[t][r] = 0.f; dV[t][r] = 0.f; }
    }

    const int nchunks = (Nq + KC - 1) / KC;
    for (int ch = sp * nchunks / splits; ch < (sp + 1) * nchunks / splits; ++ch) {
        const int q0 = ch * KC;
        const int qlen = min(KC, Nq - q0);
        const int ntiles = (qlen + 31) >> 5;
        __syncthreads();
        for (int i = tid; i < ntiles * 32 * 4; i += nthreads) {
            const int qq = i >> 2, seg = i & 3;
            const int n = q0 + qq;
            const bool valid = n < Nq;
            int64_t row; int rid;
            locate(p.q, b, wy, wx, valid ? n : 0, row, rid);
            f16x8 qv = {0, 0, 0, 0, 0, 0, 0, 0}, gv = qv;
            float dpart = 0.f;
            if (valid) {
                qv = load_f16x8(p.q, row, head, seg);
                gv = load_do_as_f16(a, row, head, seg);
                const float* op = (const float*)p.o.ptr + row * p.o.ld + p.o.col0 + head * p.o.hstride + seg * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e)                              // (from the rounded dO: see attn_dq_kernel)
                    if (seg * 8 + e < p.head_dim) dpart += op[e] * (float)gv[e];
            }
            // D_i: the four segment owners of a query are four consecutive lanes
            dpart += dpp_move<DPP_QUAD_XOR1>(dpart);
            dpart += dpp_move<DPP_QUAD_XOR2>(dpart);
            *(f16x8*)(Qs + qq * 64 + ((seg ^ ((qq >> 2) & 3)) << 4)) = qv;
            *(f16x8*)(Gs + qq * 64 + ((seg ^ ((qq >> 2) & 3)) << 4)) = gv;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                *(f16*)(Qt + (seg * 8 + e) * TROW + qq * 2) = qv[e];
                *(f16*)(Gt + (seg * 8 + e) * TROW + qq * 2) = gv[e];
            }
            if (seg == 0) {
                const int nn = valid ? n : 0;
                const int hq = nn / p.q.ww, wq = nn - hq * p.q.ww;
                qoff[qq] = hq * D + wq;
                qreg[qq] = valid ? (unsigned char)rid : (unsigned char)255;
                qlse[qq] = valid ? p.lse[(int64_t)head * p.lse_stride + row] : 1.0e30f;   // invalid query: weight 0
                qD[qq] = dpart;
            }
        }
        __syncthreads();

        for (int qt = 0; qt < ntiles; ++qt) {
            const int qb = qt * 32;
            f16x8 qfr[2], gfr[2], qtf[2], gtf[2];
            frag_rows(Qs, qb, l31, half, qfr);     // A operand: rows = queries, k-slots = head dim
            frag_rows(Gs, qb, l31, half, gfr);
            frag_cols(Qt, qb, l31, half, qtf);     // A operand: rows = head dim, k-slots = queries
            frag_cols(Gt, qb, l31, half, gtf);
            // per-query scalars of the tile's 16 rows of this lane: rows 8g + 4*half + [0..3] are four consecutive queries
            float ql[16], qd[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 l4 = *(const float4*)(qlse + qb + 8 * g + 4 * half);
                const float4 d4 = *(const float4*)(qD + qb + 8 * g + 4 * half);
                ql[4 * g] = l4.x; ql[4 * g + 1] = l4.y; ql[4 * g + 2] = l4.z; ql[4 * g + 3] = l4.w;
                qd[4 * g] = d4.x; qd[4 * g + 1] = d4.y; qd[4 * g + 2] = d4.z; qd[4 * g + 3] = d4.w;
            }
            // PLAIN: see attn_dq_kernel -- the bias of (key lane, query row i) is tab[Uk - qoff(query 0) - i]
            // MODE 2: shift mask with 16-wide query-column bands (queries 0..15 of the tile share a label, 16..31 another)
            auto tile = [&](auto mode_tag) {
                constexpr int MODE = decltype(mode_tag)::value;
                constexpr bool PLAIN = MODE != 0;
                int qofs[16], qids[16];
                if constexpr (!PLAIN) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int qq = qb + mfma32_row(r, half);
                        qofs[r] = qoff[qq]; qids[r] = qreg[qq];
                    }
                }
                const int qbase = qoff[qb];
                int id_lo = 0, id_hi = 0;
                if constexpr (MODE == 2) { id_lo = qreg[qb]; id_hi = qreg[qb + 16]; }
#pragma unroll
                for (int t = 0; t < QT; ++t) {
                    f32x16 S, dP;
                    if constexpr (PLAIN) {
                        const float* tp = tab + (Uk[t] - qbase - 4 * half);
#pragma unroll
                        for (int r = 0; r < 16; ++r) { S[r] = tp[-((r & 3) + 8 * (r >> 2))]; dP[r] = 0.f; }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) { S[r] = tab[Uk[t] - qofs[r]]; dP[r] = 0.f; }
                    }
                    S = mfma32_f16(qfr[0], kfb[t][0], S);
                    S = mfma32_f16(qfr[1], kfb[t][1], S);
                    dP = mfma32_f16(gfr[0], vfb[t][0], dP);
                    dP = mfma32_f16(gfr[1], vfb[t][1], dP);
                    f32x16 P, dS;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float s = S[r];
                        if constexpr (!PLAIN) {
                            if (border && qids[r] != idk[t]) s += MASK_L2;
                            const float pr = kvalid[t] ? __builtin_amdgcn_exp2f(s - ql[r]) : 0.f;
                            P[r] = pr;
                            dS[r] = LN2_F * pr * (dP[r] - qd[r]);
                        } else {
                            if constexpr (MODE == 2) s += (r < 8 ? id_lo : id_hi) != idk[t] ? MASK_L2 : 0.f;
                            const float pr = __builtin_amdgcn_exp2f(s - ql[r]);
                            P[r] = pr;
                            dS[r] = LN2_F * pr * (dP[r] - qd[r]);
                        }
                    }
                    f16x8 pp[2], dsp[2];
                    pack_acc(P, pp);
                    pack_acc(dS, dsp);
                    dV[t] = mfma32_f16(gtf[0], pp[0], dV[t]);
                    dV[t] = mfma32_f16(gtf[1], pp[1], dV[t]);
                    dK[t] = mfma32_f16(qtf[0], dsp[0], dK[t]);
                    dK[t] = mfma32_f16(qtf[1], dsp[1], dK[t]);
                }
            };
            if (plain) tile(std::integral_constant<int, 1>{});
            else if (toeplitz && band16) tile(std::integral_constant<int, 2>{});
            else tile(std::integral_constant<int, 0>{});
        }
    }
    const float inv = 1.0f / a.g_scale;
#pragma unroll
    for (int t = 0; t < QT; ++t)
        if (kvalid[t]) {
            if (splits == 1) {
                store_cols(a.d_k, p.k, krow[t], head, half, dK[t], inv);
                store_cols(a.d_v, p.v, krow[t], head, half, dV[t], inv);
            }
        }
    if (splits > 1) {          // (uniform) see attn_dq_kernel
        __syncthreads();
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            add_cols_lds(a.d_k, kvalid[t] ? krow[t] * p.k.ld + p.k.col0 + (int64_t)head * p.k.hstride : -1, lane, dK[t], inv, Qs + wave * XWAVE);
            add_cols_lds(a.d_v, kvalid[t] ? krow[t] * p.v.ld + p.v.col0 + (int64_t)head * p.v.hstride : -1, lane, dV[t], inv, Qs + wave * XWAVE);
        }
    }
}

// Zero fill of a split launch's destination -- a KERNEL, not hipMemsetAsync: on this ROCm (7.0.2 runtime) a hipMemsetAsync captured
// into a HIP graph is wrong from the second replay on (every 4th float keeps its old value: tools/probes/graph_memset_probe3.py,
// profiles/r06_graph_memset_probe.txt; the kernel-only control is always right).  Round 5's split launches zeroed with the
// memset, so a CAPTURED training step accumulated dQ / dK / dV onto stale values in a quarter of the entries -- finite most of
// the time, NaN when the graph's private pool had received another process's leftovers: the order-dependent failure of
// test_graphed_train_step_follows_lr_schedule_and_resume.
__global__ __launch_bounds__(256) void zero_f32x4_kernel(float4* dst, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = float4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace

extern "C" int grl_attention_bwd(void* stream, const GrlAttnBwdArgs* args) {
    const GrlAttnBwdArgs& a = *args;
    const GrlAttnArgs& p = a.fwd;
    const int Nq = p.q.wh * p.q.ww, Nk = p.k.wh * p.k.ww;
    if (Nq <= 0 || Nk <= 0 || p.B <= 0 || p.nh <= 0) return GRL_ERR_BAD_ARG;
    if (p.q.Himg != p.nwy * p.q.wh || p.q.Wimg != p.nwx * p.q.ww || p.k.Himg != p.nwy * p.k.wh || p.k.Wimg != p.nwx * p.k.ww) return GRL_ERR_BAD_ARG;
    if (p.q.transposed || p.k.transposed || p.v.transposed || p.o.transposed) return GRL_ERR_UNSUPPORTED;   // (GrlTokenGrid.transposed: forward only)
    if (p.trows != (p.q.wh + p.k.wh - 1) * (p.q.ww + p.k.ww - 1) || p.tstride < p.trows || (p.tstride & 3)) return GRL_ERR_BAD_ARG;
    if (p.head_dim > 32 || p.out_dtype != GRL_DT_F32 || p.lse == nullptr || p.lse_stride <= 0) return GRL_ERR_BAD_ARG;
    if (!a.d_o || !a.d_q || !a.d_k || !a.d_v || !a.d_table || !(a.g_scale > 0.f)) return GRL_ERR_BAD_ARG;
    if (a.d_o_ld < 0 || (a.d_o_ld % 4) || ((uintptr_t)a.d_o & 15)) return GRL_ERR_BAD_ARG;
    if ((p.q.ld % 8) || (p.k.ld % 8) || (p.v.ld % 8) || (p.o.ld % 8) || (p.q.col0 % 8) || (p.k.col0 % 8) || (p.v.col0 % 8) ||
        (p.o.col0 % 8) || (p.q.hstride % 8) || (p.k.hstride % 8) || (p.v.hstride % 8) || (p.o.hstride % 8))
        return GRL_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    GrlAttnBwdLaunch a_l;                               // the caller's arguments + the table-window sizes of the two launches
    a_l.fwd = a.fwd; a_l.d_o = a.d_o; a_l.d_q = a.d_q; a_l.d_k = a.d_k; a_l.d_v = a.d_v; a_l.d_table = a.d_table; a_l.g_scale = a.g_scale;
    a_l.d_table_fix = a.d_table_fix; a_l.d_o_ld = a.d_o_ld; a_l.tab_window = 0; a_l.tab_window_kv = 0;
    const int Dw = p.q.ww + p.k.ww - 1;
    // Split launches (see attn_dq_kernel): when a launch has fewer workgroups than the chip has CUs and a long streamed dimension,
    // cut that dimension over several workgroups that accumulate with atomics.  Needs a destination this function can zero: dense
    // head planes [nh][tokens][32] (what the training path passes).  GRL_ATTN_BWD_SPLITS=1 disables, =n forces n parts on every launch, =-n caps the automatic choice at n (timing experiments).
    const int force_splits = grl_env_int("GRL_ATTN_BWD_SPLITS", 0);       // (read per call: the tests switch it)
    auto dense = [&](const GrlTokenGrid& g) {
        return g.ld == 32 && g.col0 == 0 && g.hstride == (int64_t)p.B * g.Himg * g.Wimg * 32;
    };
    auto pick_splits = [&](int64_t grid, int streamed, bool ok) {
        const int nchunks = (streamed + KC - 1) / KC;
        if (!ok || force_splits == 1 || a.d_table_fix != nullptr) return 1;
        int s = 1;
        if (force_splits > 1) s = force_splits;
        else {
            // measured (GRL-Base training step, batch 8 x 64x64, same box): no split 156.5 ms; the 96-workgroup launches in 2 parts
            // 152.9, in 4 parts 151.5, in 8 parts 151.5; ALSO splitting the 384-workgroup launches 154.5 (they are bound by their
            // VALU work, not by parallelism).  With per-lane atomics (lane = token, 64 cache lines per instruction) instead of
            // add_cols_lds the same experiments read 162.1 / 165.0 / 164.9 / 187.4 against 169.1.
            const int cap = force_splits < 0 ? -force_splits : 4;
            while (grid * s < 256 && nchunks / (2 * s) >= 4 && 2 * s <= cap) s *= 2;      // >= 4 chunks per workgroup stay
        }
        return s < nchunks ? (s < 1 ? 1 : s) : (nchunks > 0 ? nchunks : 1);
    };
    auto zero = [&](float* ptr, const GrlTokenGrid& g) {          // (dense planes: 32 floats per token, 16-byte aligned rows)
        const int64_t n4 = (int64_t)p.nh * p.B * g.Himg * g.Wimg * 8;
        if (((uintptr_t)ptr & 15) != 0) return hipErrorInvalidValue;
        hipLaunchKernelGGL(zero_f32x4_kernel, dim3((unsigned)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048)), dim3(256), 0, st, (float4*)ptr, n4);
        return hipGetLastError();
    };
    {
        // (deterministic mode: one wave per workgroup -- the LDS histogram of the table gradient is then filled in program order)
        const int waves = a.d_table_fix ? 1 : min(4, (Nq + QT * 32 - 1) / (QT * 32));
        const int blk = waves * QT * 32;
        int64_t grid = (int64_t)((Nq + blk - 1) / blk) * p.nh * p.nwx * p.nwy * p.B;
        const int splits = pick_splits(grid, Nk, dense(p.q));
        if (splits > 1) {
            hipError_t e = zero(a.d_q, p.q);
            if (e != hipSuccess) return (int)e;
            grid *= splits;
        }
        a_l.tab_window = window_floats(blk, Nq, p.q.ww, p.q.wh, p.k.wh, Dw, p.trows);
        const size_t tpad = (size_t)a_l.tab_window * 4;
        const size_t rest = 2 * (size_t)KC * 64 + 32 * (size_t)TROW + KC * 4 + KC;
        const bool ghist = 2 * tpad + rest > 160 * 1024;
        const size_t lds = (ghist ? 1 : 2) * tpad + rest;
        if (grid > 0x7fffffff || lds > 160 * 1024) return GRL_ERR_UNSUPPORTED;
        auto kfn = ghist ? attn_dq_kernel<true> : attn_dq_kernel<false>;
        hipError_t e = hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(kfn, dim3((int)grid), dim3(waves * 64), lds, st, a_l, splits);
        GRL_CHECK_LAUNCH();
    }
    {
        const int waves = min(4, (Nk + QT * 32 - 1) / (QT * 32));
        const int blk = waves * QT * 32;
        int64_t grid = (int64_t)((Nk + blk - 1) / blk) * p.nh * p.nwx * p.nwy * p.B;
        const int splits = pick_splits(grid, Nq, dense(p.k) && dense(p.v));
        if (splits > 1) {
            hipError_t e = zero(a.d_k, p.k);
            if (e == hipSuccess) e = zero(a.d_v, p.v);
            if (e != hipSuccess) return (int)e;
            grid *= splits;
        }
        a_l.tab_window_kv = window_floats(blk, Nk, p.k.ww, p.k.wh, p.q.wh, Dw, p.trows);
        const size_t tpad = (size_t)a_l.tab_window_kv * 4;
        const size_t lds = tpad + 2 * (size_t)KC * 64 + 2 * 32 * (size_t)TROW + KC * 4 * 3 + KC;
        if (grid > 0x7fffffff || lds > 160 * 1024) return GRL_ERR_UNSUPPORTED;
        hipError_t e = hipFuncSetAttribute((const void*)attn_dkv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(attn_dkv_kernel, dim3((int)grid), dim3(waves * 64), lds, st, a_l, splits);
        GRL_CHECK_LAUNCH();
    }
    return 0;
}
