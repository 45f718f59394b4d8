// x8 geometric self-ensemble at test time (include/grl_hip.h, grl_dihedral_pack / grl_dihedral_merge): the eight flips and rotations
// of the square that the reference's Augment_RGB_torch lists (utils/dataset_utils.py:6-39, transform0 .. transform7:
// torch.rot90(t, k, dims=[-1, -2]), with .flip(-2) after it for k >= 4).  As index maps, y = T_k(x), x of H rows and W columns:
//
//   k   y[i][j] =               shape of y   inverse
//   0   x[i][j]                 H x W        T0
//   1   x[H-1-j][i]             W x H        T3
//   2   x[H-1-i][W-1-j]         H x W        T2
//   3   x[j][W-1-i]             W x H        T1
//   4   x[H-1-i][j]             H x W        T4
//   5   x[H-1-j][W-1-i]         W x H        T5
//   6   x[i][W-1-j]             H x W        T6
//   7   x[j][i]                 W x H        T7
//
// Group A (0, 2, 4, 6) keeps the shape, group B (1, 3, 5, 7) transposes it.
//
// Shape of both kernels: a workgroup of 256 threads (32 x 8) owns one 32 x 32 tile of the untransformed image -- of the source for
// pack, of the output for merge -- for one batch index, and walks the channels three at a time.  Threads of a wave run along a row
// of whatever they touch in global memory: a flipped row is the same contiguous segment met from its other end, and the
// transposing half goes through [32][33] fp32 LDS tiles (written along their rows, read along their columns; the odd pitch puts the
// 32 lanes of either access on 32 banks).  For a channels-last source the lanes of a row are a pixel apart and the unit moved is
// the pixel: a thread reads the (up to three) channels of its pixel back to back, so the line a pixel lies in is fetched once and
// met again at once, not a whole pass over the tile later.
//
//   pack    one tile read (every source value leaves HBM once), eight tiles written: four straight from the LDS rows, four from
//           its columns.  LDS 3 x 4224 bytes.
//   merge   the four group-B tiles of a pass go through LDS (16896 bytes a channel), the group-A values are read in place; a pass is
//           three channels when a member is channels-last and one channel otherwise (planar members gain nothing from the wider
//           pass and keep the smaller kernel); then
//           out = (((m0 + m1) + (m2 + m3)) + ((m4 + m5) + (m6 + m7))) * 0.125f in fp32: seven IEEE adds in that order and an exact
//           scaling, nothing for the compiler to contract, so the result is the same bits on every run and equals the same
//           expression in torch on the CPU.  fp16 members are widened first (exact).  NaN and Inf propagate.
//
// No atomics, no workspace, no scratch; every global access is guarded by the image's bounds.
#include "common.h"

namespace {

constexpr int TS = 32;            // tile side
constexpr int TY = 8;             // thread rows; a thread owns TS / TY = 4 tile rows
constexpr int PITCH = TS + 1;
constexpr int PACK_CG = 3;        // pack: channels per pass, a thread reads them from its pixel back to back

struct PackParams {
    const float* x;
    float* a;                     // [4][B][C][H][W]
    float* b;                     // [4][B][C][W][H]
    int64_t sn, sc, sh, sw;       // element strides of x
    int32_t B, C, H, W;
};

__global__ __launch_bounds__(TS * TY) void dihedral_pack_kernel(PackParams p) {
    __shared__ float tile[PACK_CG][TS][PITCH];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i0 = blockIdx.y * TS, j0 = blockIdx.x * TS;      // tile origin in the source
    const int n = blockIdx.z;
    const int H = p.H, W = p.W;
    const int64_t plane = (int64_t)H * W;
    const int64_t member = (int64_t)p.B * p.C * plane;         // one transformed copy of the batch

    for (int c0 = 0; c0 < p.C; c0 += PACK_CG) {
        const int cg = min(PACK_CG, p.C - c0);
        const float* src = p.x + n * p.sn + c0 * p.sc;
#pragma unroll
        for (int r = ty; r < TS; r += TY) {
            const int i = i0 + r, j = j0 + tx;
            if (i < H && j < W) {
                const float* px = src + i * p.sh + j * p.sw;
#pragma unroll
                for (int q = 0; q < PACK_CG; ++q)
                    if (q < cg) tile[q][r][tx] = px[q * p.sc];
            }
        }
        __syncthreads();

        for (int q = 0; q < cg; ++q) {
            const int64_t img = ((int64_t)n * p.C + c0 + q) * plane;   // image (n, c) inside a member
            float* a0 = p.a + img;                             // T0
            float* a2 = a0 + member;                           // T2
            float* a4 = a2 + member;                           // T4
            float* a6 = a4 + member;                           // T6
            float* b1 = p.b + img;                             // T1
            float* b3 = b1 + member;                           // T3
            float* b5 = b3 + member;                           // T5
            float* b7 = b5 + member;                           // T7

            // group A: lanes along an output row.  Source (i, j) lands at T0 (i, j), T6 (i, W-1-j), T4 (H-1-i, j), T2 (H-1-i, W-1-j).
            const int jf = j0 + (TS - 1 - tx);                 // the source column a flipped row takes at this lane
#pragma unroll
            for (int r = ty; r < TS; r += TY) {
                const int i = i0 + r;
                if (i >= H) continue;
                const int64_t row = (int64_t)i * W, rowf = (int64_t)(H - 1 - i) * W;
                if (j0 + tx < W) {
                    const float v = tile[q][r][tx];
                    a0[row + j0 + tx] = v;
                    a4[rowf + j0 + tx] = v;
                }
                if (jf < W) {
                    const float v = tile[q][r][TS - 1 - tx];
                    a6[row + (W - 1 - jf)] = v;
                    a2[rowf + (W - 1 - jf)] = v;
                }
            }
            // group B (W rows of H): lanes along an output row, that is along a source COLUMN of the tile.
            // Source (i, j) lands at T7 (j, i), T3 (W-1-j, i), T1 (j, H-1-i), T5 (W-1-j, H-1-i).
            const int is = i0 + tx, isf = i0 + (TS - 1 - tx);
#pragma unroll
            for (int r = ty; r < TS; r += TY) {
                const int j = j0 + r;
                if (j >= W) continue;
                const int64_t row = (int64_t)j * H, rowf = (int64_t)(W - 1 - j) * H;
                if (is < H) {
                    const float v = tile[q][tx][r];
                    b7[row + is] = v;
                    b3[rowf + is] = v;
                }
                if (isf < H) {
                    const float v = tile[q][TS - 1 - tx][r];
                    b1[row + (H - 1 - isf)] = v;
                    b5[rowf + (H - 1 - isf)] = v;
                }
            }
        }
        __syncthreads();
    }
}

struct MergeParams {
    const void* m[8];
    int64_t s[8][4];              // element strides of member k: batch, channel, row, column
    float* out;                   // [B][C][Ho][Wo]
    int32_t B, C, Ho, Wo;
};

// the pixel (row, col) of channel c of image n of member k
template <typename T>
__device__ __forceinline__ const T* member_px(const MergeParams& p, int k, int n, int c, int row, int col) {
    return static_cast<const T*>(p.m[k]) + (n * p.s[k][0] + c * p.s[k][1] + row * p.s[k][2] + col * p.s[k][3]);
}

template <typename T, int CG>
__global__ __launch_bounds__(TS * TY) void dihedral_merge_kernel(MergeParams p) {
    __shared__ float tb[CG][4][TS][PITCH];                     // members 1, 3, 5, 7 on the output's grid: tb[q][.][j - j0][i - i0]
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int i0 = blockIdx.y * TS, j0 = blockIdx.x * TS;      // tile origin in the output
    const int n = blockIdx.z;
    const int Ho = p.Ho, Wo = p.Wo;

    for (int c0 = 0; c0 < p.C; c0 += CG) {
        const int cg = min(CG, p.C - c0);
        // group B, read along the members' rows: a member's column follows the output's ROW index i (lanes), its row the column j
        //   m1[i][j] = f1[j][Ho-1-i]   m3[i][j] = f3[Wo-1-j][i]   m5[i][j] = f5[Wo-1-j][Ho-1-i]   m7[i][j] = f7[j][i]
        const int iu = i0 + tx, ifl = i0 + (TS - 1 - tx);      // straight, and flipped so that the member's column still rises
#pragma unroll
        for (int r = ty; r < TS; r += TY) {
            const int j = j0 + r;
            if (j >= Wo) continue;
            if (iu < Ho) {
                const T* f3 = member_px<T>(p, 3, n, c0, Wo - 1 - j, iu);
                const T* f7 = member_px<T>(p, 7, n, c0, j, iu);
#pragma unroll
                for (int q = 0; q < CG; ++q)
                    if (q < cg) {
                        tb[q][1][r][tx] = (float)f3[q * p.s[3][1]];
                        tb[q][3][r][tx] = (float)f7[q * p.s[7][1]];
                    }
            }
            if (ifl < Ho) {
                const T* f1 = member_px<T>(p, 1, n, c0, j, Ho - 1 - ifl);
                const T* f5 = member_px<T>(p, 5, n, c0, Wo - 1 - j, Ho - 1 - ifl);
#pragma unroll
                for (int q = 0; q < CG; ++q)
                    if (q < cg) {
                        tb[q][0][r][TS - 1 - tx] = (float)f1[q * p.s[1][1]];
                        tb[q][2][r][TS - 1 - tx] = (float)f5[q * p.s[5][1]];
                    }
            }
        }
        __syncthreads();
        // group A in place, group B from the LDS columns; lanes along the output row
        //   m0[i][j] = f0[i][j]   m2[i][j] = f2[Ho-1-i][Wo-1-j]   m4[i][j] = f4[Ho-1-i][j]   m6[i][j] = f6[i][Wo-1-j]
        const int j = j0 + tx;
        const int64_t plane = (int64_t)Ho * Wo;
        float* out = p.out + ((int64_t)n * p.C + c0) * plane;
#pragma unroll
        for (int r = ty; r < TS; r += TY) {
            const int i = i0 + r;
            if (i >= Ho || j >= Wo) continue;
            const T* f0 = member_px<T>(p, 0, n, c0, i, j);
            const T* f2 = member_px<T>(p, 2, n, c0, Ho - 1 - i, Wo - 1 - j);
            const T* f4 = member_px<T>(p, 4, n, c0, Ho - 1 - i, j);
            const T* f6 = member_px<T>(p, 6, n, c0, i, Wo - 1 - j);
#pragma unroll
            for (int q = 0; q < CG; ++q)
                if (q < cg) {
                    const float m0 = (float)f0[q * p.s[0][1]], m2 = (float)f2[q * p.s[2][1]];
                    const float m4 = (float)f4[q * p.s[4][1]], m6 = (float)f6[q * p.s[6][1]];
                    const float m1 = tb[q][0][tx][r], m3 = tb[q][1][tx][r], m5 = tb[q][2][tx][r], m7 = tb[q][3][tx][r];
                    const float lo = __fadd_rn(__fadd_rn(m0, m1), __fadd_rn(m2, m3));
                    const float hi = __fadd_rn(__fadd_rn(m4, m5), __fadd_rn(m6, m7));
                    out[q * plane + (int64_t)i * Wo + j] = __fmul_rn(__fadd_rn(lo, hi), 0.125f);
                }
        }
        __syncthreads();
    }
}

// grid of 32 x 32 tiles over rows x cols for n batch entries; false where a grid dimension would not hold it
bool tile_grid(int32_t rows, int32_t cols, int32_t n, dim3* grid) {
    const int64_t gy = ((int64_t)rows + TS - 1) / TS, gx = ((int64_t)cols + TS - 1) / TS;
    if (gy > 65535 || n > 65535) return false;
    *grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)n);
    return true;
}

// B * C * H * W * 4 (the four members of a group) below 2^31 elements, every product checked before the next factor
bool group_fits(int32_t B, int32_t C, int32_t H, int32_t W) {
    const int64_t lim = (int64_t)1 << 31;
    int64_t t = (int64_t)H * W;
    if (t >= lim) return false;
    t *= C;
    if (t >= lim) return false;
    t *= B;
    if (t >= lim) return false;
    return t * 4 < lim;
}

}  // namespace

extern "C" int grl_dihedral_pack(void* stream, const GrlDihedralPackArgs* a) {
    if (!a || !a->x || !a->out_a || !a->out_b) return GRL_ERR_BAD_ARG;
    if (a->B <= 0 || a->C <= 0 || a->H <= 0 || a->W <= 0) return GRL_ERR_BAD_ARG;
    if ((uint64_t)a->x % 4 || (uint64_t)a->out_a % 4 || (uint64_t)a->out_b % 4) return GRL_ERR_UNSUPPORTED;
    if (!group_fits(a->B, a->C, a->H, a->W)) return GRL_ERR_UNSUPPORTED;
    dim3 grid;
    if (!tile_grid(a->H, a->W, a->B, &grid)) return GRL_ERR_UNSUPPORTED;

    PackParams p;
    p.x = a->x; p.a = a->out_a; p.b = a->out_b;
    p.sn = a->stride[0]; p.sc = a->stride[1]; p.sh = a->stride[2]; p.sw = a->stride[3];
    p.B = a->B; p.C = a->C; p.H = a->H; p.W = a->W;
    hipLaunchKernelGGL(dihedral_pack_kernel, grid, dim3(TS, TY), 0, (hipStream_t)stream, p);
    GRL_CHECK_LAUNCH();
    return 0;
}

extern "C" int grl_dihedral_merge(void* stream, const GrlDihedralMergeArgs* a) {
    if (!a || !a->out) return GRL_ERR_BAD_ARG;
    if (a->dtype != GRL_DT_F32 && a->dtype != GRL_DT_F16) return GRL_ERR_BAD_ARG;
    if (a->B <= 0 || a->C <= 0 || a->Ho <= 0 || a->Wo <= 0) return GRL_ERR_BAD_ARG;
    const uint64_t align = a->dtype == GRL_DT_F32 ? 4 : 2;
    for (int k = 0; k < 8; ++k) {
        if (!a->member[k]) return GRL_ERR_BAD_ARG;
        if ((uint64_t)a->member[k] % align) return GRL_ERR_UNSUPPORTED;
    }
    if ((uint64_t)a->out % 4) return GRL_ERR_UNSUPPORTED;
    if (!group_fits(a->B, a->C, a->Ho, a->Wo)) return GRL_ERR_UNSUPPORTED;
    dim3 grid;
    if (!tile_grid(a->Ho, a->Wo, a->B, &grid)) return GRL_ERR_UNSUPPORTED;

    MergeParams p;
    for (int k = 0; k < 8; ++k) {
        p.m[k] = a->member[k];
        for (int d = 0; d < 4; ++d) p.s[k][d] = a->stride[k][d];
    }
    p.out = a->out;
    p.B = a->B; p.C = a->C; p.Ho = a->Ho; p.Wo = a->Wo;
    // channels-last members (the network's own output views): three channels of a pixel per pass, so that the line the pixel lies
    // in is met once; planar members gain nothing from that and keep the smaller kernel (a third of the LDS, more waves per CU)
    bool pixels = false;
    for (int k = 0; k < 8; ++k) pixels = pixels || (a->C > 1 && a->stride[k][1] == 1);
    const hipStream_t st = (hipStream_t)stream;
    if (a->dtype == GRL_DT_F32) {
        if (pixels) hipLaunchKernelGGL((dihedral_merge_kernel<float, 3>), grid, dim3(TS, TY), 0, st, p);
        else hipLaunchKernelGGL((dihedral_merge_kernel<float, 1>), grid, dim3(TS, TY), 0, st, p);
    } else {
        if (pixels) hipLaunchKernelGGL((dihedral_merge_kernel<f16, 3>), grid, dim3(TS, TY), 0, st, p);
        else hipLaunchKernelGGL((dihedral_merge_kernel<f16, 1>), grid, dim3(TS, TY), 0, st, p);
    }
    GRL_CHECK_LAUNCH();
    return 0;
}
