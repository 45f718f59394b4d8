/* grl_hip.h -- C ABI of the MI355X-native GRL hot path (libgrl_hip.so).
 *
 * The reference (ofsoundof/GRL-Image-Restoration) is pure Python: its "FFI" for this path is the
 * list of torch ops issued inside models/networks/grl.py::GRL.forward and the modules under
 * models/common/.  Each entry point below replaces one fused group of those ops
 * and is what a ctypes / cpp_extension binding on the reference side would call
 * (INTEGRATION.md shows the binding).  Conventions:
 *
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer owned by the caller;
 *   - no allocation, no host synchronisation; work is enqueued on `stream` (a hipStream_t,
 *     passed as void* so the header needs no HIP include; NULL = default stream);
 *   - return value: 0 on success, a hipError_t (> 0) from the launch, or a GRL_ERR_* (< 0);
 *   - activations are channels-last token matrices [B*H*W, Cpad] with Cpad = channels rounded
 *     up to a multiple of 32 and the pad channels held at zero.
 */
#ifndef GRL_HIP_H
#define GRL_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRL_ERR_BAD_ARG (-1)
#define GRL_ERR_UNSUPPORTED (-2)
#define GRL_ABI_VERSION 46

/* element kinds of activation / weight buffers */
enum { GRL_DT_F32 = 0, GRL_DT_BF16 = 1, GRL_DT_F16 = 2 };

/* ---------------------------------------------------------------------------------------------
 * Token-wise linear layer with fused epilogue.
 *   replaces  QKVProjection.forward        models/common/mixed_attn_block.py:669-676
 *             AnchorLinear.forward         models/common/mixed_attn_block.py:727-736 (pool_df > 1)
 *             MixedAttention.proj + norm1  models/common/mixed_attn_block_efficient.py:379,543-548
 *             Mlp.forward + norm2          models/common/swin_v1_block.py:37-43, efficient.py:554
 * ------------------------------------------------------------------------------------------- */
enum { GRL_EPI_PLAIN = 0, GRL_EPI_GELU = 1, GRL_EPI_GROUPNORM = 2, GRL_EPI_LN_RES = 3,
       GRL_EPI_GELU_GRAD = 4 /* ABI 22: out = (A W^T + bias) * gelu'(resid[m][col]) -- the data gradient through Mlp's activation; fp32 out */ };

typedef struct GrlLinearArgs {
    const void* a;          /* [M, lda] activations: GRL_DT_F32 (converted in-kernel) or GRL_DT_F16 */
    int32_t a_dtype;
    int64_t lda;            /* elements per A row (multiple of 8, >= Kpad)                          */
    int32_t pool_df;        /* >1: A row m is the mean of a df x df block of rows of a [B,H,W,lda]  */
    int32_t pool_H, pool_W; /*     fp32 image (AnchorLinear avg-pool); M = B*(H/df)*(W/df)          */
    const void* w;          /* fp16 [Npad, Kpad], zero padded (row n = output channel n)            */
    const float* bias;      /* [Npad]                                                               */
    int32_t M, Npad, Kpad;
    int32_t epi;            /* GRL_EPI_*                                                            */
    const float* gscale;    /* GROUPNORM: [Npad/32]; g!=0: L2-normalise the 32-col group, times |g|;*/
                            /*            g==0: pass through; g<0: additionally write 1.0 into      */
                            /*            column 31 of the group (spare head-dim slot of a K plane: */
                            /*            carries the attention kernel's running softmax offset)    */
    const float* ln_g;      /* LN_RES: gamma/beta [Npad], n_real real channels, eps, residual scale */
    const float* ln_b;
    int32_t n_real;
    float ln_eps;
    float res_scale;
    const float* resid;     /* LN_RES: fp32 residual [M, ldr]                                       */
    int64_t ldr;
    const void* add2;       /* LN_RES: optional extra branch (CAB output, GRL_DT_F16) added after   */
    int32_t add2_dtype;     /*         the norm, multiplied by add2_scale (required with add2)      */
    int64_t ldadd2;
    const float* add2_scale; /* [B, Npad] per-image channel scale applied to add2 (SE gate)           */
    int32_t rows_per_image;  /*          image of row m = m / rows_per_image                          */
    int32_t a_split;        /* 1 (default, 0 means 1) or 3: split-precision operands.  With 3, Kpad = 3 * Ksrc  */
                            /* and the kernel stages A (fp32) as [hi(a) | lo(a) | hi(a)], hi = fp16(a),         */
                            /* lo = fp16(a - hi); the caller packs W as [hi(w) | hi(w) | lo(w)]: the product    */
                            /* carries ~22 mantissa bits at 3x the MFMA work (small, error-amplifying models)   */
    float a_scale;          /* 0 means 1: fp32 A is multiplied by this before its conversion to fp16 and the          */
    float out_scale;        /* accumulator (before bias / epilogue) by out_scale (0 means 1): the backward pass feeds  */
                            /* gradients as A, pre-scaled into fp16 range, and un-scales the product                  */
    void* out;              /* [M, ldo]: GRL_DT_F32 or GRL_DT_F16 (attention operands, planes)       */
    int32_t out_dtype;
    int64_t ldo;
    int64_t out_plane_stride; /* >0: write 32-column groups as planes: element (m, c) goes to          */
                              /* out[(c/32)*out_plane_stride + m*32 + c%32]  (ldo ignored)             */
    void* out_lo;             /* optional, GRL_DT_F16 outputs: the rounding residual v - fp16(v) of every output value, */
                              /* same layout as out (the low half of a split-precision attention operand)               */
    const void* w_regs;       /* optional, a_split == 3: the weights once more, as the register image of the            */
                              /* weights-stationary kernel (csrc/linear_split.hip; plain / GELU / GROUPNORM epilogues,  */
                              /* fp32 A without pooling): per slab of 192 output columns and compute wave w = 0..5      */
                              /* (columns 192 slab + 32 w ..) 2 x Ksrc/16 MFMA A fragments of 1 KiB, hi = fp16(W) first, */
                              /* then lo = fp16(W - hi); fragment s, lane l, element e = W[column 32 (6 slab + w) +      */
                              /* (l & 31)][16 s + 8 (l >> 5) + e]; columns >= Npad zero.  grl_linear_split_blob_bytes;   */
                              /* ops.pack_linear_split.  NULL, or a shape it does not take: the generic kernel on `w`.   */
    /* ABI 22 -- operands and results at their REAL widths (training path: no padded copies of activations / gradients):  */
    int32_t a_cols;         /* > 0 (fp32 A, no pooling, a_split <= 1): A has a_cols real columns (multiple of 4), lda >= a_cols, */
                            /* lda % 4 == 0; the columns a_cols .. Kpad-1 of the operand are read as 0 ...                        */
    int32_t a_one;          /* ... except column a_cols, read as 1.0, when a_one != 0 (it meets a zero weight column in a        */
                            /* forward launch; the weight-gradient contraction finds the bias gradient there)                     */
    int32_t n_store;        /* > 0 (fp32 output, PLAIN / GELU epilogue, no planes): only the columns < n_store (multiple of 4)    */
                            /* are stored; ldo >= n_store, ldo % 4 == 0                                                           */
    int32_t a_gelu;         /* != 0 (fp32 A, no pooling, a_split <= 1): the operand is gelu(A), taken on the way to fp16 -- fc2 of the Mlp reads    */
                            /* fc1's pre-activation (swin_v1_block.py:37-43); constants of a_cols / a_one are not passed through it              */
    void* a16_out;          /* optional (fp32 A, a_split <= 1): the fp16 operand the kernel contracts -- a_scale * A, pad columns     */
    int64_t lda16;          /* and the a_one column included -- written as [M, lda16] (lda16 >= Kpad, multiple of 8): the weight-     */
                            /* gradient GEMM of the same layer reads it instead of converting the fp32 matrix once per output tile     */
} GrlLinearArgs;

int grl_linear_fwd(void* stream, const GrlLinearArgs* args);
int64_t grl_linear_split_blob_bytes(int32_t Npad, int32_t Ksrc);

/* ---------------------------------------------------------------------------------------------
 * Fused transformer MLP:  out = x + res_scale * LayerNorm(fc2(GELU(fc1(x))))  in one pass over x.
 *   replaces  Mlp.forward             models/common/swin_v1_block.py:37-43
 *             norm2 + residual         models/common/mixed_attn_block_efficient.py:554
 * The hidden activations never reach HBM and x is read once.  The weights arrive as a chunk stream ("blob"),
 * one chunk per 32 hidden channels c = 0 .. Hpad/32-1.  A chunk is the LDS image the kernel DMAs into its ring:
 *     W1c  32 rows x (2*Cpad + 16) bytes   fp16 rows 32c .. 32c+31 of fc1.weight (zero padded), columns in
 *                                          k-slot order per 32-group, 16 pad bytes per row
 *     W2c  Cpad rows x (64 + 16) bytes     fp16 columns of fc2.weight for the chunk's hidden channels in
 *                                          k-slot order, 16 pad bytes per row
 *     b1c  32 fp32                         fc1.bias for the chunk
 *   padded to a multiple of 1024 bytes; k-slot order of a 32-group: slot 8g+e <-> element 4g+e (e < 4),
 *   16+4g+e-4 (e >= 4) -- the 16x16x32 MFMA accumulator fragment of one layer is then the operand fragment of
 *   the next.  grl_mlp_blob_bytes gives the total size; ops.pack_mlp builds it; the blob must be 16-B aligned.
 * ------------------------------------------------------------------------------------------- */
typedef struct GrlMlpArgs {
    const float* x;         /* [M, ldx] fp32 input, also the residual; pad channels (>= n_real) must be 0 */
    int64_t ldx;
    const void* blob;       /* weight chunk stream, see above                                       */
    int32_t M, Cpad, Hpad;  /* Cpad in {64, 128, 192}; Hpad % 32 == 0                               */
    const float* b2;        /* [Cpad] fc2.bias                                                      */
    const float* ln_g;      /* [Cpad] norm2 weight / bias; n_real real channels                     */
    const float* ln_b;
    int32_t n_real;
    float ln_eps;
    float res_scale;
    float* out;             /* [M, ldo] fp32, pad channels = those of x (0); must not alias x       */
    int64_t ldo;
} GrlMlpArgs;

int grl_mlp_fwd(void* stream, const GrlMlpArgs* args);
int64_t grl_mlp_blob_bytes(int32_t Cpad, int32_t Hpad);

/* ---------------------------------------------------------------------------------------------
 * Block tail: everything of an EfficientMixAttnTransformerBlock after the attention and CAB kernels, in one pass:
 *     r1  = x + res_scale * LayerNorm1(att . Wp^T + bp) + cab * gate[image]     (never written to HBM)
 *     out = r1 + res_scale * LayerNorm2(fc2(GELU(fc1(r1))))
 *   replaces  MixedAttention.proj                          models/common/mixed_attn_block_efficient.py:379
 *             norm1 + residual + CAB branch + norm2 + Mlp   :543-556, models/common/swin_v1_block.py:37-43
 * att: fp16 slotted attention output [M, >= Cpad] (K = Cpad, natural order); cab: fp16 raw CAB conv output;
 * gate: [images, Cpad] SE gate (grl_se_scale_fwd); pblob: projection weight stream = Cpad/32 chunks, each 32 rows
 * (output channels) x (2*Cpad + 16) bytes fp16 padded to 1024 bytes (grl_proj_blob_bytes); blob as in GrlMlpArgs.
 * rows_per_image must be >= 128 (GRL_ERR_UNSUPPORTED otherwise).
 *
 * Register-resident variant (round 4, csrc/tail_regs.hip; GRL-Base shape: Cpad 192, Hpad 384, M and rows_per_image multiples
 * of 32, 160 < n_real <= 192): when `rblob` is given and the shape qualifies, the three weight matrices stay in the register
 * file of a persistent 8-wave workgroup as MFMA A fragments and only activations move (`blob` / `pblob` are then unused but
 * still have to be valid: other shapes fall back to the streaming kernel).  `rblob` (grl_tail_regs_blob_bytes() bytes, 16-B
 * aligned): 8 waves x 48 fragments x 1 KiB -- fragment f of wave w = 64 lanes x 16 B, lane l = 8 fp16 of row 32 t + (l & 31),
 * columns 16 s + 8 (l >> 5) + [0..8) of tile t, k-step s of a matrix: wave w < 6: f 0..11 proj tile w, 12..23 fc1 tile w,
 * 24..47 fc2 tile w (K = Hpad, natural order); waves 6, 7: f 0..35 = fc1 tiles 6..8 / 9..11 -- followed by the Hpad fp32 of fc1.bias.
 * ------------------------------------------------------------------------------------------- */
typedef struct GrlTailArgs {
    const void* att;
    int64_t ldatt;
    const float* x;         /* [M, ldx] fp32 block input (residual)                                 */
    int64_t ldx;
    const void* cab;
    int64_t ldcab;
    const float* gate;
    int32_t rows_per_image;
    const void* pblob;
    const float* pb;        /* [Cpad] proj.bias, norm1 weight / bias                                */
    const float* n1_g;
    const float* n1_b;
    const void* blob;       /* MLP weight stream (GrlMlpArgs)                                       */
    int32_t M, Cpad, Hpad;
    const float* b2;        /* [Cpad] fc2.bias, norm2 weight / bias                                 */
    const float* n2_g;
    const float* n2_b;
    int32_t n_real;
    float ln_eps;
    float res_scale;
    float* out;             /* [M, ldo] fp32; must not alias x                                      */
    int64_t ldo;
    const void* rblob;      /* NULL or the register-resident weight image (see above)               */
} GrlTailArgs;

int grl_block_tail_fwd(void* stream, const GrlTailArgs* args);
int64_t grl_tail_regs_blob_bytes(void);
int64_t grl_proj_blob_bytes(int32_t Cpad);

/* ---------------------------------------------------------------------------------------------
 * Streaming QKV projection: head planes out[slot][m][0..31] (fp16) = groupnorm(x[m,:] . W_slot^T + b_slot),
 * one pass over x for any number of slots (the weights-resident grl_linear_fwd needs column slabs above 160 KB).
 *   replaces  QKVProjection.forward   models/common/mixed_attn_block.py:669-676
 *             F.normalize + logit scale of Attention.attn   models/common/mixed_attn_block_efficient.py:39,85-90
 * A slot = 32 output columns (one head of q, k or v; see grl_attention_fwd).  Weight stream ("blob"): chunks of
 * 2 slots (1 if nslots is odd), each slot image = 32 rows x (2*Cpad + 16) bytes fp16 (columns in the k-slot order
 * of GrlMlpArgs, 16 pad bytes per row) | bias 32 fp32 | gscale fp32 + 12 pad bytes; chunk padded to 1024 bytes.
 * gscale as in GRL_EPI_GROUPNORM: != 0 -> L2-normalise the slot and multiply by |gscale|, == 0 -> pass through,
 * < 0 -> additionally column 31 of the slot is written as 1.0 (K planes, see grl_attention_fwd).
 * ------------------------------------------------------------------------------------------- */
typedef struct GrlQkvArgs {
    const float* x;            /* [M, ldx] fp32 tokens                                               */
    int64_t ldx;
    const void* blob;          /* see above; 16-B aligned; grl_qkv_blob_bytes(Cpad, nslots) bytes    */
    int32_t M, Cpad, nslots;   /* Cpad in {64, 128, 192}                                             */
    void* out;                 /* fp16 planes: element (m, slot, c) at slot*out_plane_stride + m*32 + c */
    int64_t out_plane_stride;  /* >= M*32                                                            */
} GrlQkvArgs;

int grl_qkv_fwd(void* stream, const GrlQkvArgs* args);
int64_t grl_qkv_blob_bytes(int32_t Cpad, int32_t nslots);

/* ---------------------------------------------------------------------------------------------
 * QKV projection AND anchor projection in one pass over x (round 3; csrc/qkv_anchor.hip).
 *   replaces  QKVProjection.forward               models/common/mixed_attn_block.py:661-676
 *             AnchorProjection / AnchorLinear     models/common/mixed_attn_block.py:714-736,739-785
 *             (avg_pool2d(2) + Linear C -> C/2; the pool commutes with the linear map and is applied to its outputs)
 *             F.normalize / logit scale of Attention.attn   models/common/mixed_attn_block_efficient.py:85-90,:39
 * x is the token matrix of B images of H x W tokens (H even, W a multiple of 64; other shapes: GRL_ERR_UNSUPPORTED ->
 * grl_qkv_fwd + grl_linear_fwd with pooling).  Anchor tokens are the 2 x 2 pooling cells in row-major order.
 * Weight stream `blob`: chunks of 2 slots, padded to 1 KiB; a slot = 32 rows x (2*Cpad + 16) bytes fp16 (row n = output column
 * n of the slot, K in natural order) | 32 fp32 bias | 1 fp32 gscale (+12 B); slots 0..nslots-1 = q/k/v, then nanc anchor slots.
 * gscale as in grl_qkv_fwd.
 *
 * Split-precision variant (round 4; `lo_blob` != NULL, GRL-Base shape only: Cpad 192, 18 + 3 slots, otherwise
 * GRL_ERR_UNSUPPORTED): for the normalised slots (gscale != 0: q, k, anchors) the projection is evaluated as
 *     W_hi . x_hi  +  W_hi . x_lo  +  2^-e W_lo8 . x_8,
 * W_hi = fp16(W) from `blob`, x_hi = fp16(x), x_lo = fp16(x - x_hi), W_lo8 = e4m3((W - W_hi) 2^(e+4)), x_8 = e4m3(clamp(x_hi / 16, +-448)):
 * the fp16 rounding of BOTH operands is carried (~2^-15 relative instead of 2^-11) at the cost of one more fp16 MFMA term on
 * register-resident weights and one fp8 MFMA term whose weights live in LDS.  Needed for checkpoints whose logit scales sit
 * near the clamp (exp(min(logit_scale, ln 100)), mixed_attn_block_efficient.py:39): the q.k logits multiply the operand
 * rounding by up to 144.  `lo_blob`: float 2^-e | float 2^e | 8 pad bytes | one image per normalised slot in slot order,
 * 32 rows x 192 e4m3 bytes: byte 64 c + 32 h + 8 u + t of row j = channel 64 c + 16 u + 8 h + t (the order in which one
 * 32x32x64 fp8 MFMA consumes a lane half's 32 bytes), and the 16-byte segments of a row are stored XOR-swizzled, segment s
 * at position s ^ ((j >> 2) & 3) (the image is copied to LDS verbatim).  Pass-through slots (gscale == 0: v) are not split.
 * ------------------------------------------------------------------------------------------- */
typedef struct GrlQkvAnchorArgs {
    const float* x;            /* [B*H*W, ldx] fp32 tokens                                            */
    int64_t ldx;
    int32_t B, H, W;
    int32_t Cpad;              /* 64, 128 or 192                                                      */
    const void* blob;          /* 16-B aligned; grl_qkv_anchor_blob_bytes(Cpad, nslots, nanc) bytes   */
    int32_t nslots, nanc;
    void* out;                 /* fp16 planes: element (m, slot, c) at slot*out_plane_stride + m*32 + c */
    int64_t out_plane_stride;  /* >= B*H*W*32                                                         */
    void* anc;                 /* fp16 planes of the anchors: (a, slot, c) at slot*anc_plane_stride + a*32 + c (nanc > 0) */
    int64_t anc_plane_stride;  /* >= B*(H/2)*(W/2)*32                                                 */
    const void* lo_blob;       /* NULL: fp16 operands; else the fp8 low parts of the normalised slots' weights (see above), 16-B aligned */
} GrlQkvAnchorArgs;

int grl_qkv_anchor_fwd(void* stream, const GrlQkvAnchorArgs* args);
int64_t grl_qkv_anchor_blob_bytes(int32_t Cpad, int32_t nslots, int32_t nanc);
int64_t grl_qkv_anchor_lo_blob_bytes(int32_t Cpad, int32_t nsplit);   /* nsplit = number of slots with gscale != 0 */

/* ---------------------------------------------------------------------------------------------
 * Cosine window / anchored-stripe attention (one call = one softmax(QK^T)V over all windows).
 *   replaces  WindowAttention.forward        models/common/mixed_attn_block_efficient.py:128-165
 *             AnchorStripeAttention.forward  models/common/mixed_attn_block_efficient.py:215-270
 *             (called twice: anchors->window tokens, then window tokens->anchors)
 *             Attention.attn / AffineTransform  :77-94 / :36-58
 *             roll / window_partition / window_reverse / masks / relative index
 *                                            models/common/ops.py:36-157,352-375 (all as index math)
 * Operands are fp16 token tensors with one 32-wide slot per head (fp32 accumulation):
 *   q: already L2-normalised and multiplied by logit_scale*log2(e); k: L2-normalised;
 *   v: raw values, slot column `ones_col` (>= head_dim) holding 1.0 so that the row sum of the
 *      softmax weights falls out of the PV product (ones_col < 0: summed explicitly).
 * Softmax offset (keeps the fp16 weights in range for ANY logit scale up to the clamp exp(ln 100)): a running offset that
 * follows the row maximum.  32-aligned geometries evaluate it lazily (only when a weight reaches 2^14) and keep it in
 * head-dim slot 31 of q: K must then hold 1.0 in slot 31 (`k_one31`, head_dim <= 30) and `lazy_floor[head]` (an integer
 * valued lower bound of every unmasked logit, log2 domain) must be given; otherwise the generic kernel runs an ordinary
 * online softmax.
 * ------------------------------------------------------------------------------------------- */
typedef struct GrlTokenGrid {
    const void* ptr;      /* fp16 base (o: fp16 or fp32 per out_dtype)                              */
    int64_t ld;           /* elements between consecutive tokens                                    */
    int64_t hstride;      /* elements between the 32-wide slots of consecutive heads: 32 for a      */
                          /* token-major matrix [tokens, heads*32]; tokens*32 for head planes       */
                          /* [heads][tokens][32] (the layout the QKV projection writes: a key tile  */
                          /* of 32 consecutive tokens is then 2 KB contiguous)                      */
    int32_t col0;         /* element offset of head 0's slot                                        */
    int32_t Himg, Wimg;   /* token image size                                                       */
    int32_t wh, ww;       /* window (stripe) size on this grid                                      */
    int32_t shy, shx;     /* cyclic shift (rolled[y] = orig[(y+sh) % H]); 0 = none                  */
    int32_t transposed;   /* 0: token (y, x) of image b is row (b*Himg + y)*Wimg + x of the matrix.  */
                          /* 1: the grid is the TRANSPOSED VIEW of a (Wimg x Himg) row-major image:  */
                          /* token (y, x) is row (b*Wimg + x)*Himg + y.  Attention is invariant under */
                          /* a joint transposition of the image axes (with wh/ww, shy/shx swapped and */
                          /* the bias table transposed by the caller), which brings a 128x64 stripe   */
                          /* with 32x16 anchors onto the 32-aligned fast path as 64x128 / 16x32.      */
                          /* All four grids of a launch must agree.  Forward only.                    */
} GrlTokenGrid;

typedef struct GrlAttnArgs {
    GrlTokenGrid q, k, v, o; /* v shares k's grid geometry; o shares q's                            */
    int32_t B, nh;
    int32_t nwy, nwx;        /* windows per image (same on both grids)                              */
    const float* table;      /* [nh, tstride] fp32: bias*log2e,                                     */
                             /* stored REVERSED: entry trows-1-i is row i of the reference's         */
                             /* relative-position table (keys then read ascending addresses)         */
    int32_t trows;           /* (q.wh + k.wh - 1) * (q.ww + k.ww - 1)                               */
    int32_t tstride;         /* floats between heads: trows rounded up to a multiple of 4           */
    int32_t masked;          /* 1: apply the shifted-window region mask (-100)                      */
    int32_t ones_col;        /* see above                                                           */
    int32_t head_dim;        /* real head dim (<= 32)                                               */
    int32_t out_dtype;       /* GRL_DT_F16 or GRL_DT_F32                                            */
    int32_t k_one31;         /* 1: every K row holds 1.0 in head-dim slot 31 (lazy offset possible) */
    const float* lazy_floor; /* [nh] see above (may be NULL: generic kernel)                        */
    float* lse;              /* optional [nh][lse_stride] fp32: log2-sum-exp2 of the kernel-domain  */
    int64_t lse_stride;      /* logits per query token row (what the backward kernel re-normalises with) */
    const void* q_lo;        /* optional split-precision operands (precision "high"): fp16 residuals q - fp16(q), ... on   */
    const void* k_lo;        /* the grids of q, k, v (same ld / hstride / col0).  With any of them the generic kernel forms */
    const void* v_lo;        /* S = q_hi k_hi + q_lo k_hi + q_hi k_lo and O = P_hi v_hi + P_lo v_hi + P_hi v_lo (~22-bit operands; P_lo = p - fp16(p))            */
    void* o_lo;              /* optional, GRL_DT_F16 output: residual o - fp16(o) on o's grid (the next attention's v_lo)    */
    const float* lazy_ceil;  /* optional [nh]: upper bound of every logit of the head (log2 domain: ceil(scale*log2e) + max of its   */
                             /* table).  Once the running offsets of a wave's queries are within 13.5 of it no weight can reach     */
                             /* 2^14 any more and the row-streaming kernel stops testing for it (NULL: always test)                 */
} GrlAttnArgs;

int grl_attention_fwd(void* stream, const GrlAttnArgs* args);

/* 1 when grl_attention_fwd would serve these arguments with the row-streaming kernel (csrc/attention_rows.hip): 32-aligned
 * window widths, table window within its LDS buffer, 16-aligned shifts.  Reads the geometry fields, head_dim, ones_col and
 * masked only (pointers may be NULL): lets the host choose between a grid and its transposed view at plan time. */
int grl_attention_rows_geometry_ok(const GrlAttnArgs* args);

/* ---------------------------------------------------------------------------------------------
 * 3x3 convolution (stride 1, zero pad 1) on channels-last token matrices, fused epilogue.
 *   replaces  CAB.cab[0], GELU, CAB.cab[2]          models/common/mixed_attn_block.py:970-983
 *             TransformerStage.conv (+ residual)     models/networks/grl.py:137,168-170
 *             conv_first / conv_after_body / conv_before_upsample / Upsample convs + PixelShuffle /
 *             conv_last                              models/networks/grl.py:293,348,352-379,515-518
 *                                                    models/common/upsample.py:16-19,45-46
 * ------------------------------------------------------------------------------------------- */
typedef struct GrlConvArgs {
    const void* x;          /* [B*H*W, ldx] GRL_DT_F32 or GRL_DT_F16, channels-last                 */
    int32_t x_dtype;
    int64_t ldx;
    const void* w;          /* fp16 [9][*][CinP] (tap = ky*3+kx): first output channel of this call */
    int64_t w_tap_stride;   /* elements between taps (= full layer Cout_pad * CinP)                  */
    const float* bias;      /* [CoutP]                                                              */
    int32_t B, H, W;
    int32_t CinP, CoutP;    /* CinP % 32 == 0, CoutP % 16 == 0, CoutP <= 192 per call               */
    int32_t x_split;        /* 1 (0 means 1) or 3: split-precision operands as in GrlLinearArgs.a_split: CinP =     */
                            /* 3 * CinSrc, x (fp32, CinSrc wide) is staged as [hi | lo | hi], w packed [hi | hi | lo] */
    float x_scale;          /* 0 means 1: fp32 x is multiplied by this before its conversion to fp16, the accumulator */
    float out_scale;        /* (before bias) by out_scale (0 means 1) -- gradient inputs of the backward pass         */
    int32_t act;            /* 0 none, 1 exact GELU, 2 LeakyReLU(slope)                             */
    float slope;
    const float* resid;     /* optional fp32 [B*H*W, ldr] added after the activation                */
    int64_t ldr;
    float* pool_partial;    /* optional [grl_conv3x3_num_workgroups(B,H,W), pool_stride]: per-       */
                            /* workgroup channel sums of the output (two-stage global average pool) */
    int64_t pool_stride;    /* floats per workgroup row (>= CoutP; the full layer's channel count    */
                            /* when the layer is computed as several output-channel slabs)          */
    void* out;              /* [rows, ldo] GRL_DT_F32 or GRL_DT_F16.  16-bit outputs without residual /  */
                            /* pixel shuffle: channels CoutP .. round_up(CoutP, 32) are written as zeros  */
                            /* when ldo is at least that wide (the consumer's K is padded to 32)          */
    int32_t out_dtype;
    int64_t ldo;
    int32_t shuffle_r;      /* >1: PixelShuffle(r) store into a [B, H*r, W*r, shuffle_cg] matrix;    */
    int32_t shuffle_cg;     /*     output channels are packed in (i, j, c) order, this call's        */
    int32_t shuffle_ij0;    /*     channel 0 belongs to sub-pixel group shuffle_ij0                  */
    /* ABI 22 (see GrlLinearArgs.a_cols / n_store): */
    int32_t x_cols;         /* > 0 (fp32 x, x_split <= 1): x has x_cols real channels (multiple of 4), ldx >= x_cols,   */
                            /* ldx % 4 == 0; channels x_cols .. CinP-1 are read as 0                                    */
    int32_t n_store;        /* > 0 (fp32 output, no pixel shuffle): only channels < n_store (multiple of 4) are stored  */
} GrlConvArgs;

int grl_conv3x3_fwd(void* stream, const GrlConvArgs* args);
int grl_conv3x3_num_workgroups(int32_t B, int32_t H, int32_t W);

/* CAB.cab[2] of the GRL-Base shape with the filter bank resident in registers (csrc/cab_conv2.hip): the same result as
 * grl_conv3x3_fwd on a 16-bit input with <= 48 (padded) input and 192 (padded) output channels, bias, no activation,
 * 16-bit output + the partial channel sums of the SE pool.   models/common/mixed_attn_block.py:948-983
 *   blob: grl_cab_conv2_blob_bytes() bytes, fp16 [12 channel groups][14 k-steps][64 lanes][8]: lane (g4 = lane / 16,
 *         r = lane % 16) of (group G, k-step s) holds W[16 G + r][k = 32 s + 8 g4 .. + 7], k = (ky * 3 + kx) * 48 + cin,
 *         zero for cin >= Cin, k >= 432 and output channels >= Cout.
 *   pool_partial: optional [B * wgs_per_image, pool_stride] -- one row of channel sums per workgroup (grl_se_scale_fwd's input
 *         with this wgs_per_image).  wgs_per_image persistent workgroups share the 8 x 32 pixel tiles of an image. */
typedef struct GrlCabConv2Args {
    const void* x;          /* GRL_DT_F16 [B*H*W, ldx], ldx >= 56, channels >= Cin are zero                  */
    int64_t ldx;
    const void* blob;
    const float* bias;      /* [192], zero beyond Cout                                                       */
    int32_t B, H, W;
    int32_t wgs_per_image;
    void* out;              /* GRL_DT_F16 [B*H*W, ldo], ldo >= 192: all 192 channels are written            */
    int64_t ldo;
    float* pool_partial;
    int64_t pool_stride;    /* >= 192 */
} GrlCabConv2Args;

int grl_cab_conv2_fwd(void* stream, const GrlCabConv2Args* args);
int64_t grl_cab_conv2_blob_bytes(void);

/* Squeeze-excite gate from the pooled sums: scale[b,c] = sigmoid(W2 relu(W1 mean_b + b1) + b2)
 *   replaces  ChannelAttention.attention   models/common/mixed_attn_block.py:956-967            */
int grl_se_scale_fwd(void* stream, const float* pool_partial, int32_t B, int32_t wgs_per_image, int32_t CP, int32_t C,
                     int32_t Cmid, int32_t HW, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* scale);

/* ---------------------------------------------------------------------------------------------
 * Row LayerNorm on a padded token matrix (norm_start / norm_end, models/networks/grl.py:494,501).
 * ------------------------------------------------------------------------------------------- */
int grl_layernorm_fwd(void* stream, const float* x, int64_t ldx, float* y, int64_t ldy, const float* gamma,
                      const float* beta, int32_t M, int32_t n_real, int32_t n_pad, float eps);

/* y = resid + res_scale * LayerNorm(x) (+ add2 * add2_scale[image]): the un-fused form of GRL_EPI_LN_RES
 *   replaces  norm1 / norm2 + residual (+ CAB branch)   models/common/mixed_attn_block_efficient.py:543-556
 * used by the split-precision path, whose slab-split projections cannot carry the row norm in their epilogue. */
typedef struct GrlLnResArgs {
    const float* x;         /* [M, ldx] fp32 projection output                                       */
    int64_t ldx;
    const float* resid;     /* [M, ldr] fp32                                                         */
    int64_t ldr;
    const float* gamma;     /* [n_pad]                                                               */
    const float* beta;
    const void* add2;       /* optional [M, ldadd2] GRL_DT_F32 or GRL_DT_F16, times add2_scale[image][n_pad] */
    int32_t add2_dtype;
    int64_t ldadd2;
    const float* add2_scale;
    int32_t rows_per_image;
    int32_t M, n_real, n_pad; /* n_pad <= 256, multiple of 4; pad channels written as 0              */
    float eps, res_scale;
    float* y;               /* [M, ldy] fp32                                                         */
    int64_t ldy;
} GrlLnResArgs;

int grl_layernorm_res_fwd(void* stream, const GrlLnResArgs* args);

/* ---------------------------------------------------------------------------------------------
 * Training path (BASELINE config 5; reference: engines/base.py:221-236, autograd through the modules above).
 *
 * The data gradients of the linears and convolutions re-use grl_linear_fwd / grl_conv3x3_fwd with transposed / flipped
 * weights (a_scale / x_scale bring the fp32 gradients into fp16 range).  The entry points below are the remaining
 * contractions of the backward pass and the optimizer step.
 * ------------------------------------------------------------------------------------------- */

/* Weight gradient: c[tap][n][k] += out_scale * sum_m (a_scale * a[m][n]) * b[row(m, tap)][k]   (fp32 atomics; zero c first)
 *   taps = 1: row = m (token-wise linear: dW = dY^T X)
 *   taps = 9: 3x3 convolution, a / b are [images*H*W, ld] channels-last pixel matrices, tap = (dy+1)*3 + (dx+1),
 *             row = pixel (y + dy, x + dx) of the same image, zero outside: dW[tap][co][ci]
 *   taps = 16 (ABI 34): 4x4 stride-2 pad-1 convolution (models/aux_archs/discriminator.py:102-104).  a is [images*H*W, lda] on the
 *             OUTPUT grid, b [images*2H*2W, ldb] on the input grid, tap = ky*4 + kx, row = pixel (2y + ky - 1, 2x + kx - 1) of
 *             the same image, zero outside; M = images*H*W; b_ones is not available                                    */
typedef struct GrlGemmTnArgs {
    const float* a;         /* [M, lda] fp32 (output gradient)                                      */
    int64_t lda;
    const void* b;          /* [M, ldb] GRL_DT_F32 or GRL_DT_F16 (the layer's input)                */
    int32_t b_dtype;
    int64_t ldb;
    int32_t M, N, K;        /* N, K multiples of 4 (of 8 for fp16 b)                                */
    int32_t taps, H, W;     /* 1, or 9 / 16 with the image size (of a)                              */
    int32_t splits;         /* M is cut into this many slabs (one workgroup column each)            */
    float a_scale, out_scale;
    float* c;               /* [taps][N][ldc] fp32                                                  */
    int64_t ldc, c_tap_stride;
    int64_t* c_fix;         /* optional (ABI 21): deterministic accumulation.  The slabs' partial tiles are added as 64-bit  */
                            /* fixed point (2^30 x the a_scale-d sums; integer atomics commute, fp32 atomics do not) into     */
                            /* this zeroed [taps][N][ldc] array instead of `c`; the caller converts:                          */
                            /* c = c_fix * 2^-30 * out_scale.  Bit-identical results run to run.  Range: a slab's a_scale-d   */
                            /* partial sum and the total must stay below 2^33 in magnitude (int64 / 2^30; the conversion      */
                            /* saturates, the sum wraps); resolution 2^-30, i.e. one rounding of at most 2^-31 per slab.       */
    /* ABI 22: a / b at their real widths -- N, K multiples of 4 (fp32 operands), lda >= N, ldb >= K, nothing is read beyond   */
    /* column N / K of a row -- and the bias gradient without a ones column in memory:                                          */
    int32_t b_ones;         /* != 0: b has a VIRTUAL column K that holds 1.0 (taps = 9: inside the image); its products, the   */
    int32_t reserved0;      /* column sums of a, go to c_bias[n] (taps = 9: of the centre tap) instead of a column of c         */
                            /* (reserved0: ignored)                                                                          */
    float* c_bias;          /* [N] fp32, zeroed by the caller (required with b_ones unless c_bias_fix)                          */
    int64_t* c_bias_fix;    /* [N], the deterministic counterpart (with c_fix)                                                  */
    int32_t a_dtype;        /* 0 / GRL_DT_F32: a is fp32 (the field `a`); GRL_DT_F16: a points at fp16 values that are ALREADY     */
    int32_t reserved1;      /* multiplied by a_scale (GrlLinearArgs.a16_out of the data-gradient launch).  16-bit operands: lda /  */
                            /* ldb multiples of 8 and at least N / K rounded up to 8 (the pad columns are read)                    */
} GrlGemmTnArgs;

int grl_gemm_tn(void* stream, const GrlGemmTnArgs* args);

/* Cosine attention backward (flash-style recompute from q, k, v, the forward's output and its log2-sum-exp2):
 *   replaces autograd through Attention.attn / AffineTransform  models/common/mixed_attn_block_efficient.py:36-58,77-94
 * Inputs as grl_attention_fwd (`fwd`: the same argument block, o = the forward OUTPUT (GRL_DT_F32), lse required) plus the
 * output gradient d_o (fp32, o's grid).  Outputs (fp32, gradients w.r.t. the kernel's own operands -- the normalisation,
 * the logit scale and the CPB-MLP are differentiated by the caller): d_q, d_k, d_v on the grids of q, k, v (same
 * ld / hstride / col0 in ELEMENTS as the fp16 operands), d_table [nh, tstride] (accumulated with atomics: zero it first).
 * g_scale brings d_o into fp16 range for the contractions (results are un-scaled). */
typedef struct GrlAttnBwdArgs {
    GrlAttnArgs fwd;
    const float* d_o;
    float* d_q;
    float* d_k;
    float* d_v;
    float* d_table;
    float g_scale;
    int64_t* d_table_fix;   /* optional (ABI 21): deterministic mode.  Non-null: no split launches (their partial dQ / dK / dV  */
                            /* meet in fp32 atomics), the dq kernel runs one wave per workgroup (its LDS histogram is then      */
                            /* filled in program order) and the workgroups' tables are added as 64-bit fixed point (2^32 x the   */
                            /* g_scale-d sums) into this zeroed [nh, tstride] array instead of `d_table`; the caller converts:   */
                            /* d_table = d_table_fix * 2^-32 / g_scale.  Bit-identical gradients run to run.  Range: a           */
                            /* workgroup's g_scale-d sum per entry and the total must stay below 2^31 in magnitude (int64 /       */
                            /* 2^32); resolution 2^-32, i.e. one rounding of at most 2^-33 per workgroup and entry.                */
    int64_t d_o_ld;         /* optional (ABI 22): row stride of d_o in floats when it differs from o's (0 = o's): d_o as a column  */
                            /* block of a wider gradient matrix -- the two branches' outputs are concatenated along the channels     */
                            /* before the projection (mixed_attn_block_efficient.py:374-379), so their gradients arrive that way     */
} GrlAttnBwdArgs;

int grl_attention_bwd(void* stream, const GrlAttnBwdArgs* args);

/* torch.optim.AdamW over a list of fp32 tensors in one launch (config/optimizer/adamw.yaml):
 *   w *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  w -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
 * Host-built work list: chunk c covers elements [chunk_offset[c], +4096) of tensor chunk_tensor[c].  All pointer arrays
 * live in DEVICE memory. */
typedef struct GrlAdamWArgs {
    void* const* params;
    const void* const* grads;
    void* const* exp_avg;
    void* const* exp_avg_sq;
    const int64_t* numel;
    const int32_t* weight_decay_flags;   /* optional per tensor: 0 = no decay                        */
    const int32_t* chunk_tensor;
    const int64_t* chunk_offset;
    int32_t num_chunks;
    float lr, beta1, beta2, eps, weight_decay;
    float bias_correction1, bias_correction2_sqrt;
    float grad_scale;                    /* gradients are multiplied by this (1 / loss scale, DDP averaging) */
    const float* bias_corrections_dev;   /* optional: {bias_correction1, bias_correction2_sqrt} in DEVICE memory, computed on the */
                                         /* device from a device-side step count; the two host fields above are then ignored --   */
                                         /* a launch captured in a HIP graph stays correct when it is replayed                    */
    const float* hyper_dev;              /* optional (ABI 20): {lr, weight_decay} in DEVICE memory; the host fields `lr` and           */
                                         /* `weight_decay` are then ignored -- an LR scheduler (the reference trains with MultiStepLR / */
                                         /* cosine / warm-up schedules, config/lr_scheduler) keeps working across replays of a captured  */
                                         /* launch: the caller refreshes the two floats before each replay                              */
    const float* grad_clip_dev;          /* optional (ABI 44): the clip coefficient in DEVICE memory (grl_grad_clip_finish's out[0]).   */
                                         /* The gradient scale becomes  s = grad_scale * grad_clip_dev[0]  (formed once, in fp32) and     */
                                         /* every gradient is read as  g[i] * s ; null: s = grad_scale, as before.  A coefficient of      */
                                         /* exactly 1 gives the weights of a step without clipping, bit for bit                           */
    void* const* ema;                    /* optional (ABI 44): a pointer table like exp_avg -- per tensor an fp32 average of the weights. */
                                         /* After the new weight w' is computed and stored:  e[i] = fmaf(1 - ema_decay, w' - e[i], e[i])  */
                                         /* (1 - ema_decay in fp32); null: no average, and neither the arithmetic nor the memory traffic   */
                                         /* of the launch differs from ABI 43's                                                            */
    float ema_decay;
} GrlAdamWArgs;

int grl_adamw_step(void* stream, const GrlAdamWArgs* args);

/* Gradient clipping by global norm (ABI 44; torch.nn.utils.clip_grad_norm_ with norm_type 2), without a host read and without
 * rewriting the gradients: the coefficient stays in device memory and grl_adamw_step folds it into its gradient scale.
 *
 * grl_grad_sqnorm: over the work list grl_adamw_step takes (fp32 gradients; chunk c covers [chunk_offset[c], +4096) of tensor
 *   chunk_tensor[c]), one workgroup per chunk:  partials[base + c] = sum_i (double)g[i]^2 , every element converted to double
 *   and accumulated in double, reduced in a fixed order.  No atomics: the same gradients give the same bits.  Several launches
 *   (one per parameter group) fill one buffer at their own `base`. */
typedef struct GrlGradNormArgs {
    const void* const* grads;
    const int64_t* numel;
    const int32_t* chunk_tensor;
    const int64_t* chunk_offset;
    int32_t num_chunks;
    double* partials;
    int64_t base;
} GrlGradNormArgs;

int grl_grad_sqnorm(void* stream, const GrlGradNormArgs* args);

/* grl_grad_clip_finish: one workgroup sums partials[0 .. n_partials) in a fixed order, then, in double,
 *   norm = sqrt(sum) * |grad_scale| ;  coef = max_norm / (norm + 1e-6), capped at 1 as torch.clamp(max=1) caps it
 *   (an infinite norm gives 0, a NaN norm gives NaN) ;  out[0] = (float)coef, out[1] = (float)norm  -- one rounding each.
 * `grad_scale` is the one the AdamW launch will apply (1 / world for summed data-parallel gradients): the norm is that of the
 * scaled gradient.  max_norm <= 0 or a null pointer: GRL_ERR_BAD_ARG. */
typedef struct GrlGradClipArgs {
    const double* partials;
    int64_t n_partials;
    float grad_scale;
    float max_norm;
    float* out;
} GrlGradClipArgs;

int grl_grad_clip_finish(void* stream, const GrlGradClipArgs* args);

/* Row LayerNorm of the training path (ABI 21): forward with the row statistics kept, and backward.
 *   replaces nn.LayerNorm on token matrices and autograd through it: norm1 / norm2  models/common/mixed_attn_block_efficient.py:543-556,
 *   norm_start / norm_end  models/networks/grl.py:494,501.  n <= 256 channels, a multiple of 4; row strides in elements, multiples of 4.
 * forward: y, mean[M], rstd[M];  backward: dx, and dgamma / dbeta ACCUMULATED with atomics into arrays the caller zeroes. */
typedef struct GrlLnTrainArgs {
    const float* x;  int64_t ldx;
    const float* gamma;
    const float* beta;       /* forward only */
    float* y;        int64_t ldy;      /* forward only */
    float* mean;             /* [M] written by the forward, read by the backward */
    float* rstd;
    const float* dy; int64_t lddy;     /* backward only */
    float* dx;       int64_t lddx;
    float* dgamma;
    float* dbeta;
    int32_t M, n;
    float eps;
    /* ABI 22 -- the post-norm residual of a block in the same pass (mixed_attn_block_efficient.py:543-556: x + res_scale *    */
    /* DropPath(norm(f(x)))):  forward, resid != NULL: y = resid + c_row * LayerNorm(x);  backward, alpha != 0: dy is dL/dy of   */
    /* that sum and is multiplied by c_row first (dL/dresid = dy is the caller's).  c_row = alpha * row_scale[row /              */
    /* rows_per_image] (row_scale: one keep-mask entry per image, NULL = 1).                                                     */
    const float* resid; int64_t ldr;
    const float* row_scale;
    int32_t rows_per_image;
    float alpha;
    int32_t stat_replicas;   /* backward: dgamma / dbeta are [stat_replicas][n] arrays each (0 = 1); workgroup b adds into replica      */
    int32_t reserved0;       /* b % stat_replicas and the caller sums the replicas: a few thousand atomics on ONE address serialise      */
                             /* (~36 ns each on MI355X: 2048 workgroups on 180 + 180 addresses were 75 us of a 20-us kernel)              */
} GrlLnTrainArgs;

int grl_layernorm_train_fwd(void* stream, const GrlLnTrainArgs* args);
int grl_layernorm_bwd(void* stream, const GrlLnTrainArgs* args);

/* Weight / bias packing of a 3x3 convolution for grl_conv3x3_fwd in one launch (ABI 21, training path: the weights move every step):
 *   w [Cout][Cin][3][3] fp32 (nn.Conv2d.weight: grl.py:137,293,348; mixed_attn_block.py:970-983) -> out_w fp16 [9][rows_pad][cols_pad],
 *   tap = ky*3+kx, zero padded; flip_t = 0: rows = output channels, columns = input channels (the forward operand);
 *   flip_t = 1: the data-gradient operand out_w[tap][ci][co] = w[co][ci][2-ky][2-kx] (rows = Cin side, columns = Cout side).
 *   out_b (optional): fp32 [rows_pad] = b padded with zeros (b may be NULL: all zeros). */
int grl_pack_conv3x3(void* stream, const float* w, const float* b, void* out_w, float* out_b, int32_t Cout, int32_t Cin,
                     int32_t rows_pad, int32_t cols_pad, int32_t flip_t);

/* nn.Linear weight for grl_linear_fwd and for its data-gradient launch in one launch (ABI 22, training path):
 *   w [N][K] fp32 (mixed_attn_block.py:669-676, 727-736; mixed_attn_block_efficient.py:379; swin_v1_block.py:29-33)
 *   -> out_w fp16 [Np][Kp] zero padded, (optional) out_wt fp16 [Kp][Np], its transpose, and (optional) out_b fp32 [Np] = the bias b [N]
 *   zero padded (b NULL: zeros). */
int grl_pack_linear(void* stream, const float* w, const float* b, void* out_w, void* out_wt, float* out_b, int32_t N, int32_t K, int32_t Np,
                    int32_t Kp);

/* out[i] = a[i] + b[i] (+ c[i]) (+ d[i]) on flat fp32 arrays (ABI 22; 16-byte aligned, n a multiple of 4; c, d optional): the gradient of a
 * tensor with several consumers in one launch (a block's input x feeds QKVProjection, AnchorLinear, the CAB and the residual:
 * mixed_attn_block_efficient.py:539-556) instead of autograd's pairwise adds. */
int grl_sum4(void* stream, const float* a, const float* b, const float* c, const float* d, float* out, int64_t n);

/* Head planes of the training path (ABI 21): projection output x [T, S_in, nh, d] (fp32) -> the attention operands, fp32 planes
 * out32 [S_out][nh][T][32] and their fp16 copy out16, forward; dx and the scale gradients, backward.
 *   replaces F.normalize(q) * exp(min(logit_scale, ln 100)), F.normalize(k) and the head reshape / permute of
 *   models/common/mixed_attn_block_efficient.py:36-47,85-90,147-150,240-250 and autograd through them.
 * Output slot s reads input slot src[s];  raw[s] != 0: copied as it is (v), else y = x * scale[s][h] / max(|x|, 1e-12);
 * one_col[s] >= 0: that column of the plane holds 1.0 (pad columns are otherwise 0).  d even, <= 32; S_in, S_out, nh <= 8.
 * Backward: dy[s] = gradient of output slot s as an fp32 plane [nh][T][32] (NULL: none); dx [T, S_in, nh, d] is written, dscale
 * [S_out][nh] ACCUMULATED (zero it first) for the slots with want_dscale[s] != 0. */
typedef struct GrlPlanesArgs {
    const float* x;
    const float* scale;      /* [S_out][nh] (ignored for raw slots) */
    float* out32;            /* forward; optional (NULL: only out16 is written) */
    void* out16;             /* forward: fp16 [S_out][nh][T][32] */
    const float* dy[8];      /* backward */
    float* dx;
    float* dscale;
    int32_t T, S_in, S_out, nh, d;
    int32_t src[8], raw[8], one_col[8], want_dscale[8];
    int32_t dscale_replicas; /* backward (ABI 22): dscale is [dscale_replicas][S_out][nh] (0 = 1), workgroup b adds into replica b % replicas,   */
    int32_t reserved0;       /* the caller sums them (see GrlLnTrainArgs.stat_replicas)                                                          */
} GrlPlanesArgs;

int grl_head_planes_fwd(void* stream, const GrlPlanesArgs* args);
int grl_head_planes_bwd(void* stream, const GrlPlanesArgs* args);

/* Squeeze-excite gate MLP of the CAB in a training step (ABI 22), forward and backward:
 *   replaces  ChannelAttention.attention[1..4]  models/common/mixed_attn_block.py:956-963  (Conv2d(C, C/r, 1) -> ReLU -> Conv2d(C/r, C, 1)
 *   -> Sigmoid on the pooled [B, C] means) and autograd through it.  C <= 256, Cmid <= 64; all arrays fp32, contiguous.
 * forward: hidden [B, Cmid] = relu(w1 pool + b1), gate [B, C] = sigmoid(w2 hidden + b2);  backward: d_pool [B, C] and the parameter
 * gradients d_w1 [Cmid, C], d_b1 [Cmid], d_w2 [C, Cmid], d_b2 [C] (see `parallel`). */
typedef struct GrlSeMlpArgs {
    const float* pool;       /* [B, C] */
    const float* w1;         /* [Cmid, C] */
    const float* b1;
    const float* w2;         /* [C, Cmid] */
    const float* b2;
    float* gate;             /* forward output / backward input */
    float* hidden;           /* forward output / backward input */
    const float* d_gate;     /* backward */
    float* d_pool;
    float* d_w1;
    float* d_b1;
    float* d_w2;
    float* d_b2;
    int32_t B, C, Cmid;
    int32_t parallel;        /* backward: != 0: one workgroup per image that ADDS the parameter gradients with atomics into              */
                             /* arrays the caller zeroed; 0: one workgroup walks the batch and writes them (bit-reproducible, serial)    */
} GrlSeMlpArgs;

int grl_se_mlp_fwd(void* stream, const GrlSeMlpArgs* args);
int grl_se_mlp_bwd(void* stream, const GrlSeMlpArgs* args);

/* The two passes over the token matrix around that MLP (ABI 22; [M, ld] fp32 matrices, rows 16-byte aligned, C <= 256 a multiple of 4,
 * image of row m = m / rows_per_image):
 *   grl_se_colsum: out[b][c] += k * sum over the rows of image b of a[row][c] (* f[row][c] when f != NULL); out [M / rows_per_image, C],
 *                  zeroed by the caller (atomics).  AdaptiveAvgPool2d(1) of ChannelAttention (mixed_attn_block.py:956-958) with k = 1 / HW;
 *                  backward: the gate's gradient sum_rows dy * u.
 *   grl_se_apply : out[row][c] = a[row][c] * g[b][c] (+ f[row][c]) (+ k * h[b][c]).  Forward x + cab(x) * gate (:965-967 and the residual
 *                  of mixed_attn_block_efficient.py:548); backward d_u = dy * gate + d_pool / HW. */
typedef struct GrlSeRowsArgs {
    const float* a; int64_t lda;
    const float* f; int64_t ldf;     /* optional */
    const float* g;                  /* apply: [images, C] */
    const float* h;                  /* apply, optional: [images, C] */
    float* out;     int64_t ldo;     /* colsum: [images, C] (ldo ignored); apply: [M, ldo] */
    float k;
    int32_t M, C, rows_per_image;
} GrlSeRowsArgs;

int grl_se_colsum(void* stream, const GrlSeRowsArgs* args);
int grl_se_apply(void* stream, const GrlSeRowsArgs* args);

/* Relative-position bias tables for MANY AffineTransforms at once, forward and backward (ABI 21, training path):
 *   replaces  16 * sigmoid(cpb_mlp(relative_coords_table))  models/common/mixed_attn_block_efficient.py:23-34,49-58  (cpb_mlp =
 *   Linear(2, 512, bias) -> ReLU -> Linear(512, nh, no bias)) and autograd through it, without the [G, rows, 512] hidden layer in
 *   memory (1.5 GB for the 80 stripe transforms of GRL-Base at the checkpoint geometry).
 * out[g][n][i] = 16 log2(e) sigmoid(pre[g][n][rows-1-i]) for i < rows -- the REVERSED, exp2-domain layout grl_attention_fwd reads --
 * and the value of source row 0 in the pad entries i = rows .. rows4-1.  Backward: d_w1 / d_b1 / d_w2 must be zeroed by the caller
 * (accumulated with atomics).  nh in {1, 2, 3, 4, 6, 8}, hidden = 512. */
typedef struct GrlCpbArgs {
    const float* coords;    /* [rows, 2]   relative coordinates table (tables.coords_table), shared by all transforms */
    const float* w1;        /* [G, hidden, 2]   cpb_mlp.0.weight  */
    const float* b1;        /* [G, hidden]      cpb_mlp.0.bias    */
    const float* w2;        /* [G, nh, hidden]  cpb_mlp.2.weight  */
    float* out;             /* [G, nh, rows4]   (forward)         */
    const float* d_out;     /* [G, nh, rows4]   (backward)        */
    float* d_w1;            /* [G, hidden, 2], d_b1 [G, hidden], d_w2 [G, nh, hidden]  (backward; zeroed by the caller) */
    float* d_b1;
    float* d_w2;
    int32_t G, rows, rows4, nh, hidden;
} GrlCpbArgs;

int grl_cpb_table_fwd(void* stream, const GrlCpbArgs* args);
int grl_cpb_table_bwd(void* stream, const GrlCpbArgs* args);

/* Image-quality metrics of the reference's validation (ABI 23; evaluation, not the network):
 *   replaces  tensor_round / shave / rgb2ycbcr (Y)   engines/base.py:256-271, utils/utils_image.py:8-11,30-33,43-79
 *             psnr                                   utils/metrics/psnr.py:44-48
 *             ssim (Gaussian 11x11, sigma 1.5)       utils/metrics/ssim.py:17-85
 *             psnrb (blocking effect factor)         utils/metrics/psnrb.py:22-115
 * restored / target: fp32 (B, C, H, W) with arbitrary element strides (views: crops, shaves), C = 1 or 3.  Both are rounded to 8 bit
 * (clamp to [0, 1], round(x 255) / 255) on load; the metrics see the H-2 border x W-2 border interior.  Two launches: a tile pass writes
 * per-workgroup fp64 partial sums into `workspace`, a second pass adds them per image in a fixed order and writes
 * out[b][GRL_METRIC_COUNT] (fp64; entries of metrics not asked for are NaN).  No atomics: bitwise reproducible.
 * Errors (GRL_ERR_BAD_ARG): shapes differ, C not 1 / 3, a _Y metric with C = 1, 2 border >= H or W, unknown / no metric bits,
 * workspace smaller than grl_image_metrics_workspace_bytes. */
enum { GRL_METRIC_PSNR = 1, GRL_METRIC_PSNR_Y = 2, GRL_METRIC_SSIM = 4, GRL_METRIC_SSIM_Y = 8, GRL_METRIC_PSNRB = 16,
       GRL_METRIC_PSNRB_Y = 32, GRL_METRIC_COUNT = 6 /* out column of bit (1 << i) is i */ };

typedef struct GrlMetricArgs {
    const float* restored;      /* the prediction ("preds"); PSNR-B's blocking term is measured on it alone  */
    int64_t restored_stride[4]; /* element strides of dims b, c, h, w                                        */
    int32_t shape[4];           /* B, C, H, W of restored                                                    */
    const float* target;
    int64_t target_stride[4];
    int32_t target_shape[4];    /* must equal shape                                                          */
    int32_t border;             /* shave (the SR scale; 0 otherwise)                                         */
    int32_t metrics;            /* GRL_METRIC_* bits                                                         */
    double taps[11];            /* 1-D Gaussian taps: ssim.py's window, normalised in float64, times the     */
                                /* square root of the sum of its fp32 11x11 window (the caller computes them) */
    float y_coef[3];            /* fp32 65.481/255, 128.553/255, 24.966/255: Y = round(fma chain of x*255 + 16) */
    int32_t reserved0;
    void* workspace;            /* grl_image_metrics_workspace_bytes(B, H, W, border) bytes, no initialisation */
    int64_t workspace_bytes;
    double* out;                /* [B][GRL_METRIC_COUNT] */
} GrlMetricArgs;

int64_t grl_image_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t border);
int grl_image_metrics(void* stream, const GrlMetricArgs* args);

/* Demosaicking of an RGGB Bayer mosaic by MATLAB's gradient-corrected linear filters (ABI 24; the input front end of the
 * demosaicking task, not the network):
 *   replaces  dm_matlab   utils/utils_mosaic.py:36-111 (applied to every batch by engines/base.py:126-128)
 * plane[0..3]: R (even rows, even columns), G (even, odd), G (odd, even), B (odd, odd) of the mosaic, each N x h x w fp32 with the
 * element strides `stride` (batch, row, column) shared by all four: the packed (N, 4, h, w) CFA4 tensor of the reference, or an RGB
 * image (N, 3, 2h, 2w) read in place on the RGGB lattice (strides 3*4hw, 4w, 2).  out: contiguous fp32 (N, 3, 2h, 2w), 8-byte aligned.
 * The full-resolution mosaic is reflect-padded by 2 (as torch's "reflect") and every interpolated sample is its 5x5 stencil summed in
 * fp64 and rounded once to fp32 (on 8-bit inputs: bitwise the reference run in float64, cast to fp32); native samples are copied.
 * Errors (GRL_ERR_BAD_ARG): a null pointer, N <= 0, h < 2 or w < 2 (the reference's reflection fails there too). */
typedef struct GrlDemosaicArgs {
    const float* plane[4];      /* R, G at even rows, G at odd rows, B                        */
    int64_t stride[3];          /* element strides of batch, packed row, packed column          */
    int32_t N, h, w;            /* batch and packed size; the output is 2h x 2w                 */
    int32_t reserved0;
    float* out;
} GrlDemosaicArgs;

int grl_demosaic_matlab(void* stream, const GrlDemosaicArgs* args);

/* Separable resampling by per-axis tap tables: MATLAB's antialiased bicubic imresize (ABI 25; the LQ synthesis of classical SR):
 *   replaces  imresize               utils/matlab_functions.py:91-188 (the double loop over output rows and columns)
 *             its callers            data/datasets/restoration_sr.py:130-141, utils/utils_bsr/utils_sisr.py:210-219,
 *                                    utils/metrics/niqe.py:470
 * The caller computes the tables once per (input length, scale, antialiasing) in float64 -- calculate_weights_indices,
 * matlab_functions.py:20-88, with the symmetric padding of lines 137-148 / 161-172 resolved into zero-based input indices -- and
 * uploads them: for output row o, wh[o][0..taps_h) and ih[o][0..taps_h); for output column o, ww[o][..] and iw[o][..].  The
 * kernel is scale-agnostic (down- and upsampling, any factor; indices outside the image are clamped).
 * src: fp32, read in place through four ELEMENT strides (batch, channel, row, column): crops, channels-last tensors, views.
 * out: contiguous fp32 (N, C, out_h, out_w).  Rows first, columns second; every weighted sum is accumulated in fp64, the row
 * pass result is held in fp64, and an output is rounded once to fp32.  quantize != 0 fuses the reference's tensor_round
 * (utils/utils_image.py:30-33: clamp to [0, 1], x 255, round half to even, / 255, in fp32) into the store.
 * Errors (GRL_ERR_BAD_ARG): a null pointer, a non-positive size, taps < 1, misaligned tables, a grid beyond 2^31 - 1 workgroups. */
typedef struct GrlResizeArgs {
    const float* src;
    int64_t stride[4];          /* element strides of batch, channel, row, column                 */
    int32_t N, C, H, W;
    int32_t out_h, out_w;
    int32_t taps_h, taps_w;
    const double* wh;           /* [out_h][taps_h] row weights                                    */
    const int32_t* ih;          /* [out_h][taps_h] input rows, zero-based, reflection resolved    */
    const double* ww;           /* [out_w][taps_w] column weights                                 */
    const int32_t* iw;          /* [out_w][taps_w] input columns                                  */
    float* out;
    int32_t quantize;
    int32_t out_f64;            /* ABI 26: != 0: out is double (N, C, out_h, out_w), the fp64 sums unrounded; not with quantize */
} GrlResizeArgs;

int grl_imresize(void* stream, const GrlResizeArgs* args);

/* NIQE's feature matrix (ABI 26; the no-reference metric of blind / real-world SR validation, config/metric/restorer_niqe.yaml):
 *   replaces  niqe() up to `distparam`       utils/metrics/niqe.py:400-473 (MSCN by two 7x7 convolutions, the imresize pyramid,
 *             estimate_aggd_param / compute_feature  niqe.py:341-397       10 AGGD fits per 96 x 96 block in Python)
 *             calculate_niqe's plane         niqe.py:493-546 on what NaturalImageQualityEvaluator.update hands it (niqe.py:566-574)
 * img: fp32 (B, C, H, W) with arbitrary element strides, C = 1 or 3.  It is rounded to 8 bit on load (tensor_round, as the engine
 * does before the metric, engines/base_gan.py:149-168).  C = 3: the plane is the reference's to_y_channel of a CHW RGB array, which
 * assumes BGR (niqe.py:143-156,573): round(fl32((24.966 R + 128.553 G + 65.481 B + 16) / 255) * 255), the sum in float64 -- red
 * and blue swapped against rgb2ycbcr, kept because the published numbers were computed this way.  C = 1: the rounded image.
 * The plane is cropped (top-left) to nbh x nbw whole 96 x 96 blocks, nbh = H / 96, nbw = W / 96.  Scale 1 scores it; scale 2 scores
 * imresize(plane / 255, 0.5) * 255, taken as imresize(plane, 0.5) and held in fp64 (grl_imresize with out_f64), resampled with the caller's tables for 96 nbh -> 48 nbh rows and 96 nbw -> 48 nbw
 * columns (tasks.resize_tables).  Per block and scale: MSCN with `window` (7 x 7, edge replicate at the borders of
 * the cropped plane), then the sums of the block and of its products with its four circularly shifted copies, all in fp64 in a
 * fixed order (no atomics: two calls are bitwise equal), then the 18 features; alpha is the nearest point of `grid`'s r_gam row.
 * out[b][block][36]: scale 1 then scale 2, blocks with columns outer and rows inner (niqe.py:458-465).  A block without negative or
 * without positive samples has nan features where the reference has them.  Five launches on `stream`.
 * Errors (GRL_ERR_BAD_ARG): a null pointer, C not 1 / 3, H or W below 96 (no block), B outside 1..65535, a negative stride, ngrid or
 * taps < 1, misaligned pointers, workspace smaller than grl_image_niqe_workspace_bytes. */
typedef struct GrlNiqeArgs {
    const float* img;
    int64_t stride[4];          /* element strides of dims b, c, h, w                                         */
    int32_t shape[4];           /* B, C, H, W                                                                 */
    double window[49];          /* fspecial('gaussian', 7, 7/6), row major                                    */
    const double* grid;         /* [5][ngrid] device: gam = arange(0.2, 10.001, 0.001), r_gam (niqe.py:352-356), */
                                /* gamma(1 / gam), gamma(2 / gam), gamma(3 / gam) (niqe.py:368-369,395)       */
    int32_t ngrid;
    int32_t taps_h, taps_w;     /* taps of the two half-scale tables                                          */
    int32_t reserved0;
    const double* wh;           /* [48 nbh][taps_h] as GrlResizeArgs                                          */
    const int32_t* ih;
    const double* ww;           /* [48 nbw][taps_w]                                                           */
    const int32_t* iw;
    void* workspace;            /* grl_image_niqe_workspace_bytes(B, H, W) bytes, 16-byte aligned, no initialisation */
    int64_t workspace_bytes;
    double* out;                /* [B][nbh * nbw][36]                                                         */
} GrlNiqeArgs;

int64_t grl_image_niqe_workspace_bytes(int32_t B, int32_t H, int32_t W);
int grl_image_niqe_features(void* stream, const GrlNiqeArgs* args);

/* A batch of training patches cut out of a device-resident store of 8-bit images (ABI 27; the data path of training):
 *   replaces  _pad_images / _sample_patches   data/datasets/base_image.py:276-293 (zero padding at the bottom / right, the crop)
 *             _augment                        data/datasets/base_image.py:356-372 (x[::-1], x[:, ::-1], np.swapaxes(x, 0, 1))
 *             ascontiguousarray + to_tensor   data/datasets/restoration_sr.py:111-115, restoration_dn.py:123-124
 *             and the DataLoader's collation and host-to-device copy of the batch
 * store: N images back to back, each H x W x C interleaved uint8 (C = 1 or 3, one value per store); offsets[n] is the first byte of
 * image n, dims[n] = (H, W).  work[b] = (image index, x, y, flags), read from DEVICE memory by the kernel: the launch takes no
 * per-sample scalar and stays valid inside a captured graph while the list's contents change.  With S = P * scale, sample b is the
 * crop of rows x * scale .. x * scale + S - 1 and columns y * scale .. y * scale + S - 1 (pixels outside the image read as 0), then
 * flags bit 0: rows reversed, bit 1: columns reversed, bit 2: the two axes swapped, in that order.  A paired LQ / GT batch is two
 * calls over two stores with one work list (scale 1 and s).
 * out: contiguous fp32 (B, C, S, S), 16-byte aligned; every value is float(v) / 255 by IEEE division (bitwise to_tensor).
 * An image index outside 0 .. N - 1 yields a zero patch; offsets / dims are trusted.  One launch on `stream`.
 * Errors (GRL_ERR_BAD_ARG): a null pointer, C not 1 / 3, N, B or P <= 0, scale < 1, out or work not 16-byte aligned, a grid beyond
 * 2^31 - 1 workgroups. */
typedef struct GrlPatchArgs {
    const uint8_t* store;
    const int64_t* offsets;     /* [N] byte offset of every image                               */
    const int32_t* dims;        /* [N][2] H, W                                                  */
    int32_t N, C;
    const int32_t* work;        /* [B][4] image, x (top row), y (left column), flags            */
    int32_t B, P, scale;
    int32_t reserved0;
    float* out;                 /* (B, C, P * scale, P * scale)                                 */
} GrlPatchArgs;

int grl_sample_patches(void* stream, const GrlPatchArgs* args);

/* Up to four VIEWS of one work list cut in one launch (ABI 39; the data path of dual-pixel defocus deblurring, csrc/patches.hip):
 *   replaces  the paired data set's dual-pixel item       data/datasets/restoration_paired_dataset.py:144-162 (left view, right view
 *             and GT padded, cropped at ONE position and augmented by ONE set of flips)
 *             _pad_images / _sample_patches               data/datasets/base_image.py:276-293
 *             _augment                                    data/datasets/base_image.py:356-372
 *             and torch.cat([img_lq_l, img_lq_r], dim=1)  engines/base.py:119-120
 * A view is a store (store, offsets, dims, N, C as in GrlPatchArgs), its scale, and the place of its patches in an output batch:
 * out is contiguous fp32 (B, Ctot, P * scale, P * scale), 16-byte aligned, and the view writes channels c0 .. c0 + C - 1 of it;
 * the other channels are not touched.  Several views may share one out (left view: c0 = 0, right view: c0 = 3, Ctot = 6), so no
 * concatenation follows the launch.  work, B and P are shared: work[b] = (image index, x, y, flags) in DEVICE memory, read by the
 * kernel, so the launch takes no per-sample scalar and stays valid inside a captured graph while the list's contents change.
 * Per view the semantics are those of grl_sample_patches, word for word: with S = P * scale the crop of rows x * scale ..
 * x * scale + S - 1 and columns y * scale .. y * scale + S - 1 (pixels outside the image read as 0), then flags bit 0: rows
 * reversed, bit 1: columns reversed, bit 2: the two axes swapped, in that order; every value is float(v) / 255 by IEEE division;
 * an image index outside 0 .. N - 1 of a view's store yields zeros in that view.  Views may differ in scale and C; whether a view
 * stores float4 (S a multiple of 4) is decided per view.  One launch on `stream` whatever V is.
 * NOT checked: two views whose channel windows of one out overlap -- which of them is left in the overlap is undefined.
 * Errors (GRL_ERR_BAD_ARG): those of grl_sample_patches for every view 0 .. V - 1 and the shared fields (a null pointer, C not 1 / 3,
 * N, B or P <= 0, scale < 1, out or work not 16-byte aligned, a grid beyond 2^31 - 1 workgroups over all views), V outside 1 .. 4,
 * c0 < 0 or c0 + C > Ctot.  view[V ..] is ignored. */
typedef struct GrlPatchView {
    const uint8_t* store;
    const int64_t* offsets;     /* [N] byte offset of every image                               */
    const int32_t* dims;        /* [N][2] H, W                                                  */
    int32_t N, C;
    int32_t scale;
    int32_t Ctot, c0;           /* the view fills channels c0 .. c0 + C - 1 of Ctot             */
    int32_t reserved0;
    float* out;                 /* (B, Ctot, P * scale, P * scale)                              */
} GrlPatchView;

typedef struct GrlPatchViewsArgs {
    GrlPatchView view[4];
    const int32_t* work;        /* [B][4] image, x (top row), y (left column), flags            */
    int32_t B, P, V;
    int32_t reserved0;
} GrlPatchViewsArgs;

int grl_sample_patch_views(void* stream, const GrlPatchViewsArgs* args);

/* Depthwise K x K blur of an image batch (ABI 28; the LQ synthesis of non-blind deblurring, data module `db`):
 *   replaces  input_ += F.conv2d(target, blur_kernel, groups=3, padding=(bkh, bkw))   engines/base.py:131-139
 *             input_[:, :, bkh:-bkh, bkw:-bkw], target[:, :, bkh:-bkh, bkw:-bkw]        engines/base.py:140-142 (training)
 * x: fp32 (N, C, H, W), read in place through four ELEMENT strides (batch, channel, row, column): crops, channels-last tensors.
 * taps: K x K fp32 correlation taps in DEVICE memory, row major, one table for every plane (the reference repeats its kernel over the
 * channels; utils/utils_deblur.py:127-128 has already flipped it); K odd, 1 .. 31.  The kernel reads them when it runs: no constant
 * upload, no host synchronisation, so the launch can be captured and the table rewritten between replays.
 * pad = K / 2: zero padding, out is (N, C, H, W) (validation).  pad = 0: the valid region, out is (N, C, H-K+1, W-K+1) (training: a
 * (P+K-1)^2 patch gives a P^2 LQ).  out: contiguous fp32.
 *   out[oy][ox] = fl32(sum_ky sum_kx taps[ky][kx] * x[oy - pad + ky][ox - pad + kx]) + add[oy][ox]
 * one fp32 fmaf chain from 0 per output, ky outer and kx inner: deterministic, and independent of the tiling (a `valid` output is
 * bitwise the `same` output at that place).  add (optional, the reference's noise): the output's shape, element strides add_stride
 * (batch, channel, row) and unit column stride, added after the sum was rounded.  center (optional, pad = 0 only): contiguous fp32 of
 * the output's shape that receives x[oy + K/2][ox + K/2], the reference's cropped target, from the tile already on chip.
 * One launch on `stream`.
 * Errors (GRL_ERR_BAD_ARG): a null x / taps / out, K even or outside 1 .. 31, pad neither 0 nor K / 2, H or W below K with pad = 0,
 * center with pad != 0, a non-positive N, C, H or W, a pointer not 4-byte aligned, a grid beyond 2^31 - 1 workgroups. */
typedef struct GrlBlurArgs {
    const float* x;
    int64_t stride[4];          /* element strides of batch, channel, row, column                */
    int32_t N, C, H, W;
    const float* taps;          /* [K][K] device                                                  */
    int32_t K, pad;             /* pad: K / 2 (same size) or 0 (valid region)                     */
    const float* add;           /* optional, the output's shape                                   */
    int64_t add_stride[3];      /* element strides of batch, channel, row of add                  */
    float* out;                 /* (N, C, H + 2 pad - K + 1, W + 2 pad - K + 1)                   */
    float* center;              /* optional (pad = 0), the output's shape                         */
} GrlBlurArgs;

int grl_blur_depthwise(void* stream, const GrlBlurArgs* args);

/* JPEG compression and decompression of an image batch (ABI 29; the LQ synthesis of JPEG artifact removal, data module `jpeg`):
 *   replaces  cv2.imencode(".jpg", img, [cv2.IMWRITE_JPEG_QUALITY, q]) + cv2.imdecode   data/datasets/restoration_jpeg.py:62-79
 * The entropy coding is lossless and left out; everything else is libjpeg's integer arithmetic with the defaults that OpenCV and
 * Pillow use (4:2:0 chroma, JDCT_ISLOW, baseline tables of jpeg_set_quality, fancy upsampling), restated in int32 bit for bit:
 * RGB -> YCbCr, edge replication to whole blocks, 2 x 2 chroma averaging, forward DCT, quantisation, dequantisation, inverse DCT,
 * triangle-filter chroma upsampling (plain replication for images of at most four columns, as libjpeg), YCbCr -> RGB.
 * x: contiguous fp32 (N, C, H, W), C = 3 (RGB) or 1 (gray), values k / 255; the kernel takes k = rint(255 x) clamped to 0 .. 255.
 * quality: [N] int32 in DEVICE memory, one per sample, clamped to 1 .. 100 as libjpeg clamps it.  The kernel reads it when it runs:
 * a captured call stays valid while the qualities change.
 * workspace: grl_jpeg_workspace_bytes(N, C, H, W) bytes, 8-byte aligned, no initialisation: the decoded 8-bit component planes (Y at
 * 8 ceil(H / 8) x 8 ceil(W / 8); Cb and Cr at 8 ceil(ceil(H / 2) / 8) x 8 ceil(ceil(W / 2) / 8)).
 * out: contiguous fp32 (N, C, H, W); every value is float(v) / 255 by IEEE division (bitwise to_tensor, as grl_sample_patches).
 * Two launches on `stream` (the block pass and the merge pass); no allocation, no synchronisation.
 * Errors (GRL_ERR_BAD_ARG): a null pointer, C not 1 / 3, a non-positive N, H or W, x / out / quality not 4-byte or workspace not
 * 8-byte aligned, a grid beyond 2^31 - 1 workgroups.  grl_jpeg_workspace_bytes returns GRL_ERR_BAD_ARG for such sizes. */
typedef struct GrlJpegArgs {
    const float* x;             /* (N, C, H, W)                                                   */
    const int32_t* quality;     /* [N] device                                                     */
    int32_t N, C, H, W;
    void* workspace;            /* grl_jpeg_workspace_bytes(N, C, H, W) bytes                     */
    float* out;                 /* (N, C, H, W)                                                   */
} GrlJpegArgs;

int64_t grl_jpeg_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int grl_jpeg_roundtrip(void* stream, const GrlJpegArgs* args);

/* 8-bit pack of an image batch for saving (ABI 30; the validation images the reference writes, save_images: True):
 *   replaces  tensor_round(img, 1.0)                                  utils/utils_image.py:30-33, engines/base.py:259-261
 *             F.interpolate(tn_input, scale_factor=scale)             engines/base.py:529-530 (rep = scale: the LQ of the SR tasks)
 *             to_pil_image(tn[0].detach())                            engines/base.py:545-554 (float tensor: mul(255).byte(), HWC)
 * x: fp32 (N, C, H, W), C = 1 or 3, read in place through four ELEMENT strides (batch, channel, row, column): a crop such as
 * sr[..., :h, :w] needs no copy.  rep: 1 .. 8, every source pixel becomes a rep x rep block (nearest upscale, never materialised).
 * out: contiguous uint8 (N, H rep, W rep, C), 4-byte aligned.
 *   out[n][y][x][c] = uint8(rint(clamp(x[n][c][y / rep][x / rep], 0, 1) * 255.0f))
 * rint rounds half to even, as torch.round; the multiply is one fp32 multiply of the clamped value.  NaN gives 0 (the reference's
 * result for it is undefined); -inf gives 0 and +inf gives 255.
 * One launch on `stream`; no allocation, no synchronisation.
 * Errors (GRL_ERR_BAD_ARG, nothing is launched): a null args / x / out, C not 1 / 3, a non-positive N, H or W, rep outside 1 .. 8,
 * x or out not 4-byte aligned, an output of 2^31 bytes or more, a grid beyond 2^31 - 1 workgroups. */
typedef struct GrlPack8Args {
    const float* x;
    int64_t stride[4];          /* element strides of batch, channel, row, column                */
    int32_t N, C, H, W;
    int32_t rep;                /* 1 .. 8                                                         */
    uint8_t* out;               /* (N, H rep, W rep, C)                                           */
} GrlPack8Args;

int grl_image_pack8(void* stream, const GrlPack8Args* args);

/* Unsharp-mask sharpening of an image batch (ABI 31; the sharpened GT of the real-world-SR PSNR stage, `use_usm` / `use_usm_pixel`):
 *   replaces  usm_sharp(img, weight=0.5, radius=50, threshold=10)    utils/utils_bsr/utils_usm.py:34-60 (cv2.GaussianBlur twice)
 *             USMSharp.forward                                        utils/utils_bsr/utils_usm.py:63-82 (its torch twin)
 *             uint2single + usm_sharp + single2uint on the GT         data/datasets/restoration_sr.py:105-109 (validation)
 *             self.usm_sharpener(gt)                                  data/datasets/restoration_bsr.py:56-59, 103-104 (training)
 * x, out: contiguous fp32 (N, C, H, W), C = 1 or 3; every (n, c) plane is treated on its own, all arithmetic is fp32.
 * taps: [K] fp32 in DEVICE memory (cv2.getGaussianKernel(K, 0); the reference's K is 51), K odd, 1 .. 63.  The kernels read them when
 * they run: no constant upload, no host synchronisation, so the call can be captured and the taps rewritten between replays.
 *   idx(i, n)  = reflect-101 (cv2's default border), reflected repeatedly: n == 1 -> 0; else j = i mod 2(n-1); j >= n ? 2(n-1) - j : j
 *   G(a)[y][x] = column pass(row pass(a)), each pass one fp32 fmaf chain from 0 over taps t = 0 .. K-1 reading a[idx(. + t - K/2)]
 *   blur = G(x);  res = x - blur;  m = (fabsf(res) * 255.0f > threshold) ? 1.0f : 0.0f
 *   soft = G(m);  sharp = clamp(x + weight * res, 0, 1);  out = soft * sharp + (1 - soft) * x        (each operation rounded once)
 *   quantise != 0:  out = float(rint(clamp(out, 0, 1) * 255.0f)) / 255   (half to even, IEEE division: single2uint, then to_tensor;
 *                   bitwise grl_image_pack8 of the plain result divided by 255)
 * The result of a plane does not depend on the tiling or on where the plane sits in the batch.
 * workspace: grl_usm_workspace_bytes(N, C, H, W) bytes, 4-byte aligned, no initialisation.  After the call it holds blur, then m,
 * each contiguous fp32 (N, C, H, W).
 * Two launches on `stream` (x -> blur, m; then m, x, blur -> out); no allocation, no synchronisation.
 * Errors (GRL_ERR_BAD_ARG, nothing is launched): a null args / x / taps / workspace / out, C not 1 / 3, K even or outside 1 .. 63, a
 * non-positive N, H or W, H or W above 2^30, a pointer not 4-byte aligned, a grid beyond 2^31 - 1 workgroups.
 * grl_usm_workspace_bytes returns GRL_ERR_BAD_ARG for such sizes. */
typedef struct GrlUsmArgs {
    const float* x;             /* (N, C, H, W)                                                   */
    const float* taps;          /* [K] device                                                     */
    int32_t N, C, H, W;
    int32_t K;                  /* odd, 1 .. 63                                                   */
    int32_t quantise;           /* != 0: 8-bit levels / 255                                       */
    float weight, threshold;    /* the reference: 0.5, 10                                         */
    void* workspace;            /* grl_usm_workspace_bytes(N, C, H, W) bytes                      */
    float* out;                 /* (N, C, H, W)                                                   */
} GrlUsmArgs;

int64_t grl_usm_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int grl_usm_sharp(void* stream, const GrlUsmArgs* args);

/* ITEM LIST: the contract of the six entries of the blind-SR data path that work on lists of images whose sizes differ --
 * grl_cv_resize, grl_blur_items (ABI 32, bsr_degrade.py), grl_isp_unprocess / grl_isp_process / grl_isp_roundtrip (ABI 37, isp.py)
 * and grl_color_jitter (ABI 38, jitter.py); csrc/item_list.h is its code.  Inside one batch every sample has its own size and
 * parameters, so an entry reads an item list from DEVICE memory, the idiom of grl_sample_patches: one launch serves all items of a
 * call, nothing is allocated, the host does not synchronise, and the launch stays valid inside a captured graph while the list's
 * contents change.
 *   items[i] = eight int64: {src_off, dst_off, h, w, and four slots the entry names}.  The source image is contiguous fp32 (C, h, w)
 *   at ELEMENT offset src_off of the source arena `src` (src_elems floats), the destination image contiguous fp32 at element offset
 *   dst_off of the destination arena `dst` (dst_elems floats).  The two arenas may be one buffer as long as no item's destination
 *   overlaps any item's source (an entry that may run an item in place, src_off == dst_off, says so).  The result of an item does
 *   not depend on which other items share the launch.
 *   On the host (GRL_ERR_BAD_ARG, nothing is launched): a null args / src / dst / items, src / dst not 4-byte or items not 8-byte
 *   aligned, n_items (times C where a workgroup owns one plane) outside 1 .. 65535, a non-positive src_elems or dst_elems, a vouched
 *   maximum below 1 (the entry's least side) or above 2^20, more than 2^31 - 1 tiles; and what the entry adds.
 *   The HOST WRAPPER VOUCHES for what exists in the device table only: that the maxima it passes (max_ho / max_wo, max_h / max_w,
 *   max_K) are at least every item's -- the grid is sized from them, surplus workgroups leave, and an item beyond them would be
 *   computed only where the grid reaches -- and that the destinations of a call do not overlap.
 *   Everything else THE KERNEL CHECKS: an item with a side (or stride) below 1 (the entry's least side) or above 2^20, or of which
 *   any part -- source, destination, and the taps, tables or normals the entry names -- does not lie inside the buffer's stated
 *   length, or whose entry-specific slots are out of range, is skipped whole.  "Lies inside" is off >= 0, count <= elems and
 *   off <= elems - count: no sum is formed, so no offset, however large, wraps into range, and no list content makes a kernel read
 *   or write outside the buffers its arguments describe.
 *
 * grl_cv_resize: OpenCV's resize, INTER_LINEAR / INTER_CUBIC / INTER_AREA
 *   replaces  cv2.resize(img, (int(1/2 w), int(1/2 h)), interpolation=random.choice([1, 2, 3]))        utils/utils_bsr/utils_sisr.py:299-303
 *             cv2.resize(img, (int(1/sf1 w), int(1/sf1 h)), interpolation=random.choice([1, 2, 3]))    utils/utils_bsr/utils_sisr.py:350-354
 *             cv2.resize(img, (int(1/sf a), int(1/sf b)), interpolation=random.choice([1, 2, 3]))      utils/utils_bsr/utils_sisr.py:416-420
 * items[i] = {src_off, dst_off, h, w, ho, wo, interp, 0}: (C, h, w) -> (C, ho, wo); interp 1, 2, 3 are cv2.INTER_LINEAR, INTER_CUBIC,
 * INTER_AREA.  Per axis, scale = n / no; coordinates and weights in float64, each weight rounded once to fp32; tap indices outside
 * the image clamp to the edge:
 *   linear  f = (d + 0.5) scale - 0.5, i = floor(f), t = f - i; i < 0: i = 0, t = 0; i >= n - 1: i = n - 1, t = 0; taps i, i + 1: 1 - t, t
 *   cubic   the same f, i, t without the clamps; taps i - 1 .. i + 2, A = -0.75: c0 = ((A(t+1) - 5A)(t+1) + 8A)(t+1) - 4A,
 *           c1 = ((A+2)t - (A+3))t^2 + 1, c2 = c1's form at 1 - t, c3 = 1 - c0 - c1 - c2
 *   area    h >= ho and w >= wo: the coverage table -- f1 = d scale, f2 = f1 + scale, cell = min(scale, n - f1), s1 = ceil(f1),
 *           s2 = min(floor(f2), n - 1), s1 = min(s1, s2); (s1 - f1) / cell on s1 - 1 if s1 - f1 > 1e-3; 1 / cell on s1 .. s2 - 1;
 *           min(min(f2 - s2, 1), cell) / cell on s2 if f2 - s2 > 1e-3
 *           otherwise: the linear taps (and clamps) with i = floor(d scale), t = (d + 1) - (i + 1) / scale, t = 0 if t <= 0 else
 *           t - floor(t), on both axes
 *   out[oy][ox] = chain_ky wy[ky] * fl32(chain_kx wx[kx] * src[iy(ky)][ix(kx)]), each chain an fp32 fmaf chain from 0 in ascending tap
 *   order: the horizontal pass, then the vertical one.
 * This is OpenCV's sampling rule with float64 coordinates.  OpenCV rounds the coordinate to fp32 first, which moves a weight by up to
 * n * 2^-24; equality with OpenCV's bytes is not claimed.
 * Errors (GRL_ERR_BAD_ARG): those of ITEM LIST (the maxima are max_ho, max_wo), C not 1 / 3. */
typedef struct GrlCvResizeArgs {
    const float* src;           /* source arena                                                   */
    float* dst;                 /* destination arena                                              */
    int64_t src_elems, dst_elems; /* their lengths in floats: no item reads / writes beyond them  */
    const int64_t* items;       /* [n_items][8] device: src_off, dst_off, h, w, ho, wo, interp, 0 */
    int32_t n_items, C;
    int32_t max_ho, max_wo;     /* host-known maxima of ho, wo over the items (vouched for)       */
} GrlCvResizeArgs;

int grl_cv_resize(void* stream, const GrlCvResizeArgs* args);

/* grl_blur_items: K x K blur with scipy's `mirror` boundary, per-item taps and a stride
 *   replaces  ndimage.filters.convolve(img, np.expand_dims(k, axis=2), mode="mirror")                  utils/utils_bsr/utils_sisr.py:341-343, 410-412
 *             ndimage.filters.convolve(img, k_shifted[..., None], mode="mirror"); img[0::sf, 0::sf]     utils/utils_bsr/utils_sisr.py:359-362
 * items[i] = {src_off, dst_off, h, w, K, s, taps_off, 0}: (C, h, w) -> (C, ceil(h / s), ceil(w / s)); K odd, 1 .. max_K <= 31; s >= 1;
 * the item's K x K fp32 taps, row major, at element taps_off of `taps`.  One tap table serves the item's channels.
 *   out[oy][ox] = sum over ky (outer), kx (inner) of taps[ky][kx] * x[m(oy s - K/2 + ky, h)][m(ox s - K/2 + kx, w)]
 *   m(i, n): scipy's mirror (reflect-101), folded as often as needed: n == 1 -> 0; else j = i mod 2(n-1); j >= n ? 2(n-1) - j : j
 * (after a large downscale the image is smaller than the kernel).  One fp32 fmaf chain from 0 in that order, as grl_blur_depthwise.
 * The taps are CORRELATION taps: ndimage.convolve convolves, so the caller passes the kernel flipped over both axes
 * (tasks.blur_taps).  Only the strided outputs are computed.
 * Errors (GRL_ERR_BAD_ARG): those of ITEM LIST (the maxima are max_ho, max_wo; n_items * C at most 65535), C not 1 / 3, max_K even or
 * outside 1 .. 31, a null or not 4-byte aligned taps, a non-positive taps_elems. */
typedef struct GrlBlurItemsArgs {
    const float* src;           /* source arena                                                   */
    float* dst;                 /* destination arena                                              */
    const float* taps;          /* taps buffer, device                                            */
    int64_t src_elems, dst_elems, taps_elems;
    const int64_t* items;       /* [n_items][8] device: src_off, dst_off, h, w, K, s, taps_off, 0 */
    int32_t n_items, C;
    int32_t max_ho, max_wo;     /* host-known maxima of ceil(h / s), ceil(w / s) (vouched for)    */
    int32_t max_K;              /* host-known maximum of K: odd, 1 .. 31                          */
    int32_t reserved0;
} GrlBlurItemsArgs;

int grl_blur_items(void* stream, const GrlBlurItemsArgs* args);

/* ---------------------------------------------------------------------------------------------
 * U-Net discriminator of the GAN stage (ABI 34, csrc/disc.hip): the contractions the 3x3 kernels do not cover.
 *   replaces  UNetDiscriminatorSN.conv1 / conv2 / conv3 (+ leaky_relu)      models/aux_archs/discriminator.py:102-104,118-120
 *             F.interpolate(scale_factor=2, mode="bilinear", align_corners=False)   models/aux_archs/discriminator.py:123,128,133
 *             and autograd through both in the two optimizer steps            engines/base_gan.py:86-147
 *
 * grl_conv4x4s2_fwd: Conv2d(Cin, Cout, 4, 2, 1, bias=False) on a channels-last token matrix, out[b, oy, ox, co] =
 *   act(out_scale * sum_{ky,kx,ci} w[ky*4+kx][co][ci] * x_scale * x[b, 2 oy + ky - 1, 2 ox + kx - 1, ci]), zero outside the image.
 *   GrlConvArgs: H, W = the size of x (even; odd: GRL_ERR_UNSUPPORTED), out is [B*(H/2)*(W/2), ldo]; w = grl_pack_conv4x4(transpose
 *   = 0): fp16 [16][CoutP][CinP], w_tap_stride >= CoutP * CinP; CinP % 32 == 0, CoutP % 16 == 0; x / out GRL_DT_F32, 16-byte aligned,
 *   ldx / ldo multiples of 4 and at least the real widths (GRL_ERR_BAD_ARG otherwise); x_cols / n_store as grl_conv3x3_fwd;
 *   act 0 or 2 (LeakyReLU(slope)); bias, resid, pool_partial must be NULL, x_split <= 1, shuffle_r <= 1 (GRL_ERR_UNSUPPORTED).
 * grl_conv4x4s2_bwd_data: the transposed convolution, dx[b, iy, ix, ci] = out_scale * sum w[ky*4+kx][co][ci] * x_scale * dy[b, oy, ox, co]
 *   over 2 oy + ky - 1 = iy, 2 ox + kx - 1 = ix -- per parity class of (iy, ix) a 2 x 2-tap convolution of dy.
 *   GrlConvArgs: x = dy [B*(H/2)*(W/2), ldx] with x_cols = Cout, out = dx [B*H*W, ldo] with n_store = Cin, H, W = the size of dx;
 *   w = grl_pack_conv4x4(transpose = 1): fp16 [16][CoutP = pad16(Cin)][CinP = pad32(Cout)]; act must be 0; x_scale / out_scale as in
 *   the 3x3 data gradient.  Same checks as the forward; nothing is launched when one fails.
 * grl_pack_conv4x4: w [Cout][Cin][4][4] fp32 -> fp16 [16][rows_pad][cols_pad] zero padded, tap = ky*4 + kx; transpose = 0: rows =
 *   output channels, columns = input channels; transpose = 1: rows = input channels, columns = output channels. */
int grl_conv4x4s2_fwd(void* stream, const GrlConvArgs* args);
int grl_conv4x4s2_bwd_data(void* stream, const GrlConvArgs* args);
int grl_pack_conv4x4(void* stream, const float* w, void* out_w, int32_t Cout, int32_t Cin, int32_t rows_pad, int32_t cols_pad,
                     int32_t transpose);

/* x2 bilinear upsampling (align_corners=False) of a channels-last token matrix and its adjoint:
 *   forward  x [B*H*W, ldx] -> out [B*2H*2W, ldo]: per axis weights 0.75 / 0.25 on the two nearest inputs, the index clamped at the
 *            edges (output 0 reads input 0 alone), combined in torch's order h0 (w0 v00 + w1 v01) + h1 (w0 v10 + w1 v11);
 *   backward dy [B*2H*2W, lddy] -> dx [B*H*W, lddx]: each input gathers its <= 16 outputs in a fixed order (no atomics).
 * C real channels, a multiple of 4 (16-byte accesses); leading dimensions multiples of 4 and >= C; 16-byte aligned bases
 * (GRL_ERR_BAD_ARG otherwise, nothing is launched). */
int grl_upsample2x_bilinear_fwd(void* stream, const float* x, int64_t ldx, float* out, int64_t ldo, int32_t B, int32_t H, int32_t W,
                                int32_t C);
int grl_upsample2x_bilinear_bwd(void* stream, const float* dy, int64_t lddy, float* dx, int64_t lddx, int32_t B, int32_t H, int32_t W,
                                int32_t C);

/* ---------------------------------------------------------------------------------------------
 * VGG19 perceptual loss of the GAN stage (ABI 35, csrc/vgg.hip): everything between the 3x3 convolutions.
 *   replaces  VGGFeatureExtractor.forward: range_norm, input norm, ReLU, MaxPool2d(2, 2), the feature taps
 *                                                                            models/aux_archs/vgg.py:223,240-246,257-266
 *             PerceptualLoss.forward: L1Loss per tapped layer * layer weight * perceptual_weight   losses/losses.py:126-143
 *             and autograd through them for the restored image (the VGG is frozen, gt is detached: losses.py:127, vgg.py:229-232)
 * The convolutions themselves are grl_conv3x3_fwd launches (act = 2, slope = 0: ReLU in the epilogue of the untapped layers).
 *
 * grl_vgg_prep_fwd: image (fp32, any element strides stride[0..3] over (b, c, y, x), 3 channels) -> tok [B*H*W, ldt] fp32, columns
 *   0..2 = the channels, column 3 = 0: t = range_norm ? (x + 1) / 2 : x;  t = use_input_norm ? (t - mean[c]) / std[c] : t with the
 *   float32 values of mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225).  `scale` is not read.
 * grl_vgg_prep_bwd: the adjoint, tok = the gradient [B*H*W, ldt] (columns 0..2 read) -> image[b, c, y, x] = (use_input_norm ?
 *   g / std[c] : g) * scale; the caller folds 1 / S of the operand scale and the 1/2 of range_norm into `scale`.
 *   ldt >= 4, a multiple of 4; tok 16-byte aligned (GRL_ERR_BAD_ARG otherwise; nothing is launched). */
typedef struct GrlVggPrepArgs {
    float* image;               /* forward: read; backward: written                               */
    int64_t stride[4];          /* element strides of image over (b, c, y, x)                     */
    float* tok;                 /* forward: written; backward: read                               */
    int64_t ldt;
    int32_t B, H, W;
    int32_t use_input_norm, range_norm;
    float scale;                /* backward only                                                  */
} GrlVggPrepArgs;

int grl_vgg_prep_fwd(void* stream, const GrlVggPrepArgs* args);
int grl_vgg_prep_bwd(void* stream, const GrlVggPrepArgs* args);

/* One tapped layer.  fx / fg: the pre-ReLU features [B*H*W, ldf] fp32 of the restored image and of the target (two halves of one
 * matrix or two matrices), C real channels (C % 4 == 0), 16-byte aligned, ldf % 4 == 0.
 * grl_vgg_tap_fwd:
 *   (a) partial[w] (fp64, one per workgroup; n_partial >= grl_vgg_tap_num_workgroups(B, H, W, C)) = that workgroup's share of
 *       sum |fx - fg|; a finishing launch adds them in a fixed order: loss[0] = (accumulate ? loss[0] : 0) + (float)(coef * sum), and
 *       layer_sum[0] = (float)sum when layer_sum is not NULL.  No atomics: bit-identical from run to run.
 *   (b) pool != 0: px / pg [B*(H/2)*(W/2), ldp] = maxpool2x2(relu(fx)) / (fg), floor sizes as nn.MaxPool2d(2, 2) (an odd last row /
 *       column is not pooled); pool_dtype GRL_DT_F32 or GRL_DT_F16 (what the next convolution's loader rounds to anyway).
 * grl_vgg_tap_bwd: dfx [B*H*W, lddf] = k * sign(fx - fg) + (fx > 0 and fx is the first maximum of its window in (dy, dx) row-major
 *   order ? dpool : 0); sign(0) = 0; dpool [B*(H/2)*(W/2), lddp] fp32 or NULL (the last tap); pixels outside the floor-pooled region
 *   get the first term alone.  k = S * layer_weight * perceptual_weight * upstream / (B*C*H*W) with S the chain's operand scale.
 * Bad pointers / leading dimensions: GRL_ERR_BAD_ARG, nothing is launched. */
typedef struct GrlVggTapArgs {
    const float* fx;
    const float* fg;
    int64_t ldf;
    int32_t B, H, W, C;
    int32_t pool, pool_dtype;
    void* px;
    void* pg;
    int64_t ldp;
    double* partial;
    int32_t n_partial, accumulate;
    float* loss;
    float* layer_sum;
    float coef;                 /* forward: layer_weight * perceptual_weight / (B*C*H*W)          */
    float k;                    /* backward: S * coef * upstream gradient                         */
    const float* dpool;
    int64_t lddp;
    float* dfx;
    int64_t lddf;
} GrlVggTapArgs;

int grl_vgg_tap_num_workgroups(int32_t B, int32_t H, int32_t W, int32_t C);
int grl_vgg_tap_fwd(void* stream, const GrlVggTapArgs* args);
int grl_vgg_tap_bwd(void* stream, const GrlVggTapArgs* args);

/* The style half of that PerceptualLoss (ABI 40, csrc/gram.hip): Gram matrices of the tapped features, criterion "l1".
 *   replaces  PerceptualLoss._gram_mat and the style branch of PerceptualLoss.forward                 losses/losses.py:147-187
 * f: the pre-ReLU token matrix [images*hw, ldf] fp32 of a tapped layer (restored images first, then the targets), C real channels,
 * C one of 64 / 128 / 256 / 512 (GRL_ERR_UNSUPPORTED otherwise), ldf % 4 == 0, 16-byte aligned.  f32-input MFMA throughout: the
 * features are never rounded below fp32.
 * grl_vgg_gram_fwd (losses.py:174-187): gram [nb, C, C] fp32 = F_b^T F_b / (C*hw) per image.  The token axis is cut into chunks inside
 *   an image (never across two), each chunk an fp32 fmaf chain of at most 2048 terms; the chunks are added in float64 in a fixed
 *   order, no atomics: the same bits on every run, and gram[b] is exactly symmetric (the upper triangle is computed and mirrored).
 *   ws: workspace of ws_bytes >= grl_vgg_gram_workspace_bytes(nb, hw, C).  rowbound (NULL or [nb]): rowbound[b] = sum_c max_t
 *   |F_b[t, c]| >= max_t sum_c |F_b[t, c]|, a bound on every entry of F_b * Sigma for Sigma of entries -1 / 0 / 1.
 * grl_vgg_gram_loss (losses.py:160-168): nb == 2 * B; diff [B, C, C] = gram[:B] - gram[B:]; loss[0] = (accumulate ? loss[0] : 0) +
 *   (float)(coef * sum |diff|), layer_sum[0] = (float)sum when not NULL; the sum in float64 in a fixed order through partial (fp64,
 *   n_partial >= grl_vgg_gram_loss_num_workgroups(B, C)) as grl_vgg_tap_fwd forms its own.  NaN features give a NaN loss.
 * grl_vgg_gram_bwd (autograd through losses.py:147-187): d[b*hw + t, c'] += k * sum_c f[b*hw + t, c] * sign(diff[b, c, c']) for the B
 *   restored images, sign(0) = 0; rows of other images and columns >= C of d are not touched.  gram being symmetric, Sigma + Sigma^T =
 *   2 * Sigma, so k = S * upstream * style_weight * layer_weight / (B*C*C) * 2 / (C*hw) with S the chain's operand scale.
 * Bad pointers / leading dimensions: GRL_ERR_BAD_ARG, nothing is launched. */
typedef struct GrlVggGramArgs {
    const float* f;
    int64_t ldf;
    int32_t nb, B, hw, C;       /* fwd: nb images; loss: nb == 2 * B; bwd: the B restored images  */
    float* gram;                /* fwd: written; loss: read                                       */
    void* ws;
    int64_t ws_bytes;
    float* rowbound;
    float* diff;                /* loss: written; bwd: read                                       */
    double* partial;
    int32_t n_partial, accumulate;
    float* loss;
    float* layer_sum;
    float coef;                 /* loss: style_weight * layer_weight / (B*C*C)                    */
    float k;                    /* bwd                                                            */
    float* d;
    int64_t ldd;
} GrlVggGramArgs;

int64_t grl_vgg_gram_workspace_bytes(int32_t nb, int32_t hw, int32_t C);
int grl_vgg_gram_loss_num_workgroups(int32_t B, int32_t C);
int grl_vgg_gram_fwd(void* stream, const GrlVggGramArgs* args);
int grl_vgg_gram_loss(void* stream, const GrlVggGramArgs* args);
int grl_vgg_gram_bwd(void* stream, const GrlVggGramArgs* args);

/* ---------------------------------------------------------------------------------------------
 * LPIPS, net = "vgg" (ABI 36, csrc/lpips.hip): everything between the 3x3 convolutions of the metric's VGG16 trunk.
 *   replaces  lpips.LPIPS(net="vgg").forward(img1, img2, normalize=True) of package version 0.1, as
 *             LearnedPerceptualImagePatchSimilarity calls it                              utils/metrics/lpips.py:20,40
 *             (config/metric/restorer_perceptual.yaml: val_lpips)
 * The convolutions themselves are grl_conv3x3_fwd launches (act = 2, slope = 0: ReLU in the epilogue of the untapped layers).
 *
 * grl_lpips_prep: image (fp32 in [0, 1], any element strides stride[0..3] over (b, c, y, x), 3 channels) -> tok [B*H*W, ldt] fp32,
 *   columns 0..2 = ((2x - 1) - shift[c]) / scale[c] with the float32 values of shift = (-0.030, -0.088, -0.188), scale = (0.458,
 *   0.448, 0.450), column 3 = 0: the layout of grl_vgg_prep_fwd.  ldt >= 4, a multiple of 4; tok 16-byte aligned. */
typedef struct GrlLpipsPrepArgs {
    const float* image;
    int64_t stride[4];          /* element strides of image over (b, c, y, x)                     */
    float* tok;
    int64_t ldt;
    int32_t B, H, W;
    int32_t reserved0;
} GrlLpipsPrepArgs;

int grl_lpips_prep(void* stream, const GrlLpipsPrepArgs* args);

/* One tapped layer.  f: the fp32 pre-activation [2*B*H*W, ldf] of a block-closing convolution, the B restored images' rows first,
 * then the B targets'; C = 64, 128, 256 or 512 real channels (GRL_ERR_UNSUPPORTED otherwise, and for B > 65535), 16-byte aligned,
 * ldf % 4 == 0.  w [C] fp32, 16-byte aligned: the layer's 1x1 weights, any sign.
 *   (a) out[b] (fp64, b < B) = (accumulate ? out[b] : 0) + mean over the H*W pixels of sum_c w[c] * (u0_c - u1_c)^2 with
 *       u = relu(f) / (sqrt(sum_c relu(f)_c^2) + 1e-10) per pixel and image (an all-zero pixel gives zeros).  fp32 inside a pixel,
 *       fp64 from the pixel on; partial [n_partial >= grl_lpips_tap_num_workgroups(B, H, W, C)] fp64 holds one sum per (workgroup,
 *       image), a finishing launch adds them in a fixed order.  No atomics: bit-identical from run to run; equal halves give 0.
 *   (b) pool != 0: pool_out [2*B*(H/2)*(W/2), ldp] 16-bit (GRL_DT_F16) = maxpool2x2(relu(f)) of both halves in f's order, floor
 *       sizes as nn.MaxPool2d(2, 2) (an odd last row / column is not pooled, and still counts in (a)); NaN is kept.
 *   (c) gmax != NULL (ABI 43, the training forward): gmax[0] (fp32) = G = max over the restored half's pixels and the channels with
 *       f0_c > 0 of |r * (e_c - (f0_c / n) * sum_j e_j u0_j)|, the tap term's gradient of grl_lpips_tap_bwd before its k (0 where no
 *       channel qualifies); gpartial [n_partial] fp32 holds one maximum per (workgroup, image), the finishing launch reduces them.
 *       No atomics.  (a) and (b) are the same bits with and without (c); gmax == NULL is the call of ABI 36.
 * Bad pointers / leading dimensions: GRL_ERR_BAD_ARG, nothing is launched. */
typedef struct GrlLpipsTapArgs {
    const float* f;
    int64_t ldf;
    const float* w;
    int32_t B, H, W, C;
    int32_t pool, accumulate;
    void* pool_out;
    int64_t ldp;
    double* partial;
    double* out;
    int32_t n_partial, reserved0;
    float* gpartial;            /* (c): [n_partial] fp32, else NULL                               */
    float* gmax;                /* (c): [1] fp32; NULL: no gradient bound                         */
} GrlLpipsTapArgs;

int grl_lpips_tap_num_workgroups(int32_t B, int32_t H, int32_t W, int32_t C);
int grl_lpips_tap(void* stream, const GrlLpipsTapArgs* args);

/* LPIPS as a training loss (ABI 43): the adjoints of grl_lpips_tap and grl_lpips_prep for the restored half.
 *   replaces  torch autograd through lpips.LPIPS(net="vgg").forward(img1, img2, normalize=True): normalize_tensor, the 1x1 lin
 *             layers, spatial_average, and the ReLU + MaxPool2d(2, 2) of torchvision's vgg16().features that follow a tapped layer
 * loss = mean_b sum_l mean_pixels sum_c w_c (u0_c - u1_c)^2.  Per pixel of the restored half, with f0 = relu(pre0), n = ||f0||_2 over
 * channels, r = 1 / (n + 1e-10), u0 = f0 * r (u1 likewise from the target), e_c = 2 w_c (u0_c - u1_c), k_l = upstream / (B*H*W):
 *     dL/df0_c   = k_l * r * (e_c - (f0_c / n) * sum_j e_j u0_j),   f0_c / n := 0 where n = 0
 *     dL/dpre0_c = pre0_c > 0 ? dL/df0_c + (the pool gradient where this pixel holds the first maximum of its 2 x 2 window) : 0
 * grl_lpips_tap_bwd: f, w, B, H, W, C as in grl_lpips_tap (only the restored half gets a gradient; the target half is read);
 *   dpool [B*(H/2)*(W/2), lddp] fp32 or NULL (the last tap): the gradient of the pooled output, already under the scale S;
 *   d [B*H*W, ldd] fp32 = k * r * (...) + routed dpool under the select, k = S * k_l.  u0 - u1 is evaluated as in the forward
 *   (normalise, then subtract).  Pixels MaxPool's floor drops (odd H or W) get the tap term and no pool term; masked entries and
 *   pixels whose post-ReLU features are all zero are exactly 0.  No atomics: bit-identical from run to run. */
typedef struct GrlLpipsTapBwdArgs {
    const float* f;
    int64_t ldf;
    const float* w;
    int32_t B, H, W, C;
    const float* dpool;
    int64_t lddp;
    float* d;
    int64_t ldd;
    float k;                    /* S * upstream / (B*H*W)                                         */
    int32_t reserved0;
} GrlLpipsTapBwdArgs;

int grl_lpips_tap_bwd(void* stream, const GrlLpipsTapBwdArgs* args);

/* grl_lpips_prep_bwd: tok [B*H*W, ldt >= 4] fp32 (the gradient token matrix, columns 0..2) -> dx (fp32, element strides stride[0..3]
 *   over (b, c, y, x)): dx_c = 2 * tok_c / scale[c] * scale, scale = 1 / S. */
typedef struct GrlLpipsPrepBwdArgs {
    const float* tok;
    int64_t ldt;
    float* dx;
    int64_t stride[4];
    int32_t B, H, W;
    float scale;
} GrlLpipsPrepBwdArgs;

int grl_lpips_prep_bwd(void* stream, const GrlLpipsPrepBwdArgs* args);

/* ---------------------------------------------------------------------------------------------
 * The camera-noise stage of the blind-SR degradation (ABI 37, csrc/isp.hip): stage 2 of degradation_sr2, the ISP model.
 *   replaces  img, HR = ispmodel.forward(img.copy(), HR)                                   utils/utils_bsr/utils_sisr.py:365-370
 *             ISPModel.forward: isp.reverse(x, True), isp.forward(., True); isp.reverse(x1, False), isp.forward(., False)
 *                                                                                          utils/utils_bsr/utils_isp.py:539-543
 *             ISPNet.reverse / forward (431-454) with GammaCorrect (206-212), ToneMapping (354-360), XYZ2LinearRGB (85-89),
 *             Raw2XYZ (57-67), ExposureCompensation (105-109), Demosaic (270-309), AddNoise.reverse (374-377);
 *             utils_color.linear2gamma colour space 0 (utils_color.py:172-180); utils_noise.add_noise (utils_noise.py:95-103)
 * The three entries follow the ITEM LIST contract above (before grl_cv_resize), with a least side of 3; the tone tables and the
 * normals are checked against tables_elems / normals_elems as the images against the arenas.  grl_isp_roundtrip may also run an
 * item in place, src == dst and src_off == dst_off: a thread reads its pixel's three channels before it writes them.
 *   items[i]  = {src_off, dst_off, h, w, yi_off, yi_inv_off, z_off, 0}: element offsets of the images into the arenas, of the
 *               item's forward and inverse tone tables (1,000,001 fp32 each, delta = 1e-6: ToneMapping.yi / yi_inv) into `tables`,
 *               and of its h * w unit normals into `normals` (read by grl_isp_unprocess alone).  The offsets live here and not in
 *               the fp32 record: a float does not hold an offset beyond 2^24.
 *   params[i] = 40 floats: W1i, W2i, W2, W1 (3 x 3 each, row major; W2 = camera -> XYZ(D50), W1 = XYZ(D50) -> linear sRGB, W1i and
 *               W2i their inverses), 2^e, 2^-e (carried for the caller; the kernels divide by 2^e as the reference does), shot, read.
 * All arithmetic is fp32 (the compiler may contract a multiply and an add); clamp(x) = min(max(x, 0), 1), NaN -> 0; M x is
 * (m0 x0 + m1 x1) + m2 x2 per row; lut(t, x) = t[min(rint(x / 1e-6f), 1000000)].  Per pixel:
 *   unprocess chain   x = clamp(x); x = x > 0.04045 ? ((200 x + 11) / 211)^2.4 : max(x, 1e-8) / 12.92; x = clamp(lut(yi_inv, clamp(x)));
 *                     x = W1i x; x = W2i x; x = clamp(x / 2^e)
 *   process chain     x = clamp(x * 2^e); x = W2 x; x = W1 x; x = clamp(lut(yi, clamp(x)));
 *                     x = x > 0.0031308 ? 1.055 x^(1/2.4) - 0.055 : 12.92 x; x = clamp(x)
 * grl_isp_unprocess: (3, h, w) -> the noisy RGGB raw plane (h, w): the unprocess chain, of which pixel (y, x) keeps channel
 *   (y & 1) + (x & 1) -- R at even row and column, B at odd row and column, G elsewhere; only that row of W2i is evaluated --,
 *   r = clamp(r), then r = clamp(r + sqrt(r * shot + read) * z[y * w + x]).
 * grl_isp_process: raw plane (h, w) -> (3, h, w): the plane reflect-padded by 2 (torch's "reflect": -1 -> 1, n -> n - 2), the four
 *   5 x 5 filters of Demosaic.__init__ (kgrb at R and B sites for G; krbg0 / krbg1 for R and B at the G sites of a red / blue row and
 *   swapped for the other colour; krbbr for B at R sites and R at B sites; every weight is an exact binary fraction), native samples
 *   copied, clamp, then the process chain.  0::2 / 1::2 indexing: odd sides are served.
 * grl_isp_roundtrip: (3, h, w) -> (3, h, w): the unprocess chain on all three channels, then the process chain -- the HR pass,
 *   without mosaic and noise.
 * Errors (GRL_ERR_BAD_ARG, nothing is launched): those of ITEM LIST (the maxima are max_h, max_w, at least 3), C not 3, a null params /
 * tables (normals for grl_isp_unprocess), a non-positive normals_elems there, tables_elems below 1,000,001, params / tables /
 * normals not 4-byte aligned. */
typedef struct GrlIspArgs {
    const float* src;           /* source arena                                                   */
    float* dst;                 /* destination arena                                              */
    int64_t src_elems, dst_elems; /* their lengths in floats: no item reads / writes beyond them  */
    const int64_t* items;       /* [n_items][8] device: src_off, dst_off, h, w, yi_off, yi_inv_off, z_off, 0 */
    const float* params;        /* [n_items][40] device                                           */
    const float* tables;        /* the tone tables, device                                        */
    int64_t tables_elems;
    const float* normals;       /* unit normals, device; grl_isp_unprocess only (else NULL)       */
    int64_t normals_elems;
    int32_t n_items, C;         /* C = 3                                                          */
    int32_t max_h, max_w;       /* host-known maxima of h, w over the items (vouched for)         */
} GrlIspArgs;

int grl_isp_unprocess(void* stream, const GrlIspArgs* args);
int grl_isp_process(void* stream, const GrlIspArgs* args);
int grl_isp_roundtrip(void* stream, const GrlIspArgs* args);

/* ---------------------------------------------------------------------------------------------
 * The colour jitter of the blind-SR training branch (ABI 38, csrc/jitter.hip).
 *   replaces  self.jitter = T.ColorJitter(brightness=0.2, contrast=0.2, saturation=0.2, hue=0.05)
 *             img_gt = self.jitter(util.uint2tensor4(img_gt))                       data/datasets/restoration_bsr.py:66-68,100
 *             i.e. torchvision's ColorJitter.forward on a float RGB tensor in [0, 1]: the ops of get_params' permutation, each one of
 *             adjust_brightness, adjust_contrast, adjust_saturation, adjust_hue (transforms/_functional_tensor.py: _blend,
 *             rgb_to_grayscale, _rgb2hsv, _hsv2rgb).
 * The statement below is written from torchvision's published source; torchvision is not a dependency and no run of it backs the
 * tests: they hold the kernels to a float64 evaluation of this statement and its hue step to Python's colorsys.  Not claimed:
 * bit equality with a torchvision run, and the summation order of torch.mean behind the contrast mean.
 * The entry follows the ITEM LIST contract above (before grl_cv_resize).  An item may run in place, src == dst and
 * src_off == dst_off: a thread reads its pixels' three channels before it writes them.  The grid and the partial buffer are sized
 * from max_h / max_w; beyond the shared checks the kernels skip whole -- the image and its mean stay unwritten -- an item whose
 * h * w needs more workgroups than grl_color_jitter_num_workgroups(max_h, max_w), or whose ops are no permutation of 0 .. 3.  The
 * same inputs give the same bits on every run: there are no atomics.
 *   items[i]  = {src_off, dst_off, h, w, op0, op1, op2, op3}: element offsets of the (3, h, w) images into the arenas (the offsets
 *               live here and not in the fp32 record: a float does not hold an offset beyond 2^24), and the ops in the order
 *               they run: 0 brightness, 1 contrast, 2 saturation, 3 hue (get_params' torch.randperm(4)).
 *   params[i] = 4 floats: b, c, s (ColorJitter draws them from [0.8, 1.2]) and h (from [-0.05, 0.05]).
 * All arithmetic is fp32 (the compiler may contract a multiply and an add) except the sum behind the contrast mean;
 * clamp(x) = min(max(x, 0), 1), NaN -> 0;  gray(x) = (0.2989 r + 0.587 g) + 0.114 b   (rgb_to_grayscale);
 * blend(x, y, f) = clamp(f x + (1 - f) y)   (_blend).  Per image, in the order of the item:
 *   brightness   x = blend(x, 0, b)                                                                      adjust_brightness
 *   contrast     m = the mean of gray(x) over the h * w pixels of the image as it stands at this point of the chain;
 *                x = blend(x, m, c) on all three channels                                                adjust_contrast
 *                (m: gray in fp32, summed in fp64 -- per thread, per wave, per workgroup, then the workgroups' sums in a fixed
 *                order --, divided by h * w in fp64, rounded to fp32 for the blend and written to means[i] in fp64)
 *   saturation   x = blend(x, gray(x), s) per pixel                                                      adjust_saturation
 *   hue          _rgb2hsv: maxc, minc the channel max / min, eq = maxc == minc, cr = maxc - minc; S = cr / (eq ? 1 : maxc);
 *                d = eq ? 1 : cr; rc, gc, bc = (maxc - r | g | b) / d;
 *                H = maxc == r ? bc - gc : maxc == g ? (2 + rc) - bc : (4 + gc) - rc;  H = fmod(H / 6 + 1, 1);  V = maxc
 *                adjust_hue: H = (H + h) mod 1 with a non-negative result (torch.remainder: fmod, plus 1 when negative)
 *                _hsv2rgb: i = floor(6 H), f = 6 H - i; p = clamp(V (1 - S)), q = clamp(V (1 - S f)), t = clamp(V (1 - S (1 - f)));
 *                i = i mod 6 (i is 6 when the remainder rounded to 1); (r, g, b) = row i of
 *                (V, t, p) (q, V, p) (p, V, t) (p, q, V) (t, p, V) (V, p, q)
 * The call is two launches.  Pass 1 walks the ops that precede contrast per pixel and writes one fp64 sum of gray per (item,
 * workgroup) to partial[i * W + g], W = grl_color_jitter_num_workgroups(max_h, max_w) (a workgroup owns 4096 consecutive pixels:
 * a 400 x 400 image has 40 partials); pass 2 adds the item's partials, writes means[i], and walks the whole chain.
 * Errors (GRL_ERR_BAD_ARG, nothing is launched): those of ITEM LIST (the maxima are max_h, max_w; the tile count does not apply), C not
 * 3, a null params / partial / means, n_partial below n_items * W, params not 4-byte or partial / means not 8-byte aligned.
 * grl_color_jitter_num_workgroups returns
 * GRL_ERR_BAD_ARG for a max_h or max_w out of that range. */
typedef struct GrlColorJitterArgs {
    const float* src;           /* source arena                                                   */
    float* dst;                 /* destination arena                                              */
    int64_t src_elems, dst_elems; /* their lengths in floats: no item reads / writes beyond them  */
    const int64_t* items;       /* [n_items][8] device: src_off, dst_off, h, w, op0, op1, op2, op3 */
    const float* params;        /* [n_items][4] device: b, c, s, h                                */
    double* partial;            /* [n_partial] device scratch, written by pass 1                  */
    int64_t n_partial;          /* >= n_items * grl_color_jitter_num_workgroups(max_h, max_w)     */
    double* means;              /* [n_items] device: the contrast mean of every item that ran     */
    int32_t n_items, C;         /* C = 3                                                          */
    int32_t max_h, max_w;       /* host-known maxima of h, w over the items (vouched for)         */
} GrlColorJitterArgs;

int grl_color_jitter_num_workgroups(int32_t max_h, int32_t max_w);
int grl_color_jitter(void* stream, const GrlColorJitterArgs* args);

/* ---------------------------------------------------------------------------------------------
 * x8 geometric self-ensemble at test time (ABI 41, csrc/ensemble.hip, ensemble.py): the image under the eight flips and rotations of
 * the square, each result mapped back, the eight averaged.
 *   restates  Augment_RGB_torch.transform0 .. transform7                            utils/dataset_utils.py:6-39
 *             (torch.rot90(t, k, dims=[-1, -2]) for k = 0 .. 3, and the same with .flip(-2) after it for k = 4 .. 7; the reference
 *             lists the transforms and never calls them from its engine)
 * y = T_k(x), x of H rows and W columns:
 *   k   y[i][j] =               shape of y   inverse
 *   0   x[i][j]                 H x W        T0
 *   1   x[H-1-j][i]             W x H        T3
 *   2   x[H-1-i][W-1-j]         H x W        T2
 *   3   x[j][W-1-i]             W x H        T1
 *   4   x[H-1-i][j]             H x W        T4
 *   5   x[H-1-j][W-1-i]         W x H        T5
 *   6   x[i][W-1-j]             H x W        T6
 *   7   x[j][i]                 W x H        T7
 * Group A = T0, T2, T4, T6 keeps the shape; group B = T1, T3, T5, T7 transposes it.
 *
 * grl_dihedral_pack: x fp32 (B, C, H, W), read in place through four ELEMENT strides (batch, channel, row, column), every value
 * once.  out_a: contiguous (4 B, C, H, W) = T0, T2, T4, T6 of the batch; out_b: contiguous (4 B, C, W, H) = T1, T3, T5, T7; the batch
 * index inside a group is member-major, (position in the group) * B + b.  For H == W the two may be the halves of one
 * (8 B, C, H, H) buffer: a square tile becomes one batch of eight.  One launch.
 *
 * grl_dihedral_merge: member[k] is what the model made of T_k(x): (B, C, Ho, Wo) for group A, (B, C, Wo, Ho) for group B, all fp32
 * or all fp16 (dtype), each with its own base pointer and its own four element strides, read where the model left it.  With
 * m_k = T_k^-1(member[k]) (the inverse column above; (B, C, Ho, Wo) each),
 *   out = (((m0 + m1) + (m2 + m3)) + ((m4 + m5) + (m6 + m7))) * 0.125f
 * in fp32: fp16 values are widened first, the adds are IEEE adds in exactly this order and the scaling is exact, so the same
 * expression in torch on the CPU gives the same bits, on every run; NaN and Inf propagate.  out: contiguous fp32 (B, C, Ho, Wo).
 * One launch, no workspace, no atomics.
 *
 * Errors, nothing is launched.  GRL_ERR_BAD_ARG: a null args / x / out_a / out_b / member / out, a non-positive B, C, H or W, a dtype
 * other than GRL_DT_F32 / GRL_DT_F16.  GRL_ERR_UNSUPPORTED: a pointer not aligned to its element, 4 B C H W (one group) of 2^31
 * elements or more, H above 32 * 65535 or B above 65535. */
typedef struct GrlDihedralPackArgs {
    const float* x;
    int64_t stride[4];          /* element strides of batch, channel, row, column                */
    int32_t B, C, H, W;
    float* out_a;               /* (4 B, C, H, W): T0, T2, T4, T6                                 */
    float* out_b;               /* (4 B, C, W, H): T1, T3, T5, T7                                 */
} GrlDihedralPackArgs;

typedef struct GrlDihedralMergeArgs {
    const void* member[8];      /* member[k] = model(T_k(x))                                      */
    int64_t stride[8][4];       /* element strides of member k: batch, channel, row, column      */
    int32_t dtype;              /* GRL_DT_F32 or GRL_DT_F16, of all eight                         */
    int32_t B, C, Ho, Wo;       /* the OUTPUT's shape                                             */
    int32_t reserved0;
    float* out;                 /* (B, C, Ho, Wo)                                                 */
} GrlDihedralMergeArgs;

int grl_dihedral_pack(void* stream, const GrlDihedralPackArgs* args);
int grl_dihedral_merge(void* stream, const GrlDihedralMergeArgs* args);

/* ---------------------------------------------------------------------------------------------
 * Progressive training and MixUp (ABI 42, csrc/remix.hip, remix.py): what the reference's engine does to every training batch
 * between the data loader and the model.
 *   restates  the progressive mini-batch / mini-patch of the training forward       engines/base.py:144-169
 *             MixUp_AUG.aug                                                          utils/dataset_utils.py:43-60
 * Inputs: lq (B, Cl, P, P) fp32 and gt (B, Cg, s P, s P) fp32, s the scale; Cl != Cg is legal (dual-pixel: 6 / 3).  Stage lengths
 * L_0 .. L_{k-1} with cumulative sums S_g, batches b_g <= B, patches p_g <= P (LQ side).
 *   Stage        the stage of optimizer step n is bisect.bisect_left(S, n): step n == S_0 still belongs to stage 0.
 *   Mini-batch   idx = rng.sample(range(B), k=b) when b < B; sample i of the output is sample idx[i] of the input, in that order.
 *                No draw when b == B.
 *   Mini-patch   x0 = rng.randrange(P - p + 1), then y0 likewise, when p < P.  LQ rows x0 : x0 + p, columns y0 : y0 + p (x0 indexes
 *                ROWS, as in the reference); the target is the same window times s.  No draw when p == P.
 *   MixUp        perm = randperm(b), then lam = Beta(1.2, 1.2).rsample((b, 1)); out_i = lam_i * x_i + (1 - lam_i) * x_perm[i] for
 *                lq and gt alike, in fp32, on the already reduced batch.  A fixed point of the permutation is still computed:
 *                lam * x + (1 - lam) * x is not x in floating point.
 *   Draw order   per step: sample, x0, y0 from a random.Random; then randperm, Beta from a CPU torch.Generator.
 *
 * grl_batch_remix does the whole transform for both tensors in one launch.  items[i], i < b, in DEVICE memory (rewritten in place
 * from step to step, so a captured launch follows the table on replay):
 *   out[i] = mix ? lam * A + (1 - lam) * B : A,   A / B = the window (x0, y0) of input sample src_a / src_b
 * evaluated as __fadd_rn(__fmul_rn(lam, a), __fmul_rn(__fsub_rn(1.0f, lam), b)): four IEEE operations, no FMA, so the torch
 * expression lam * a + (1 - lam) * b on the CPU gives the same bits; NaN and Inf propagate.  With mix == 0 the kernel copies A and
 * reads neither B nor lam.  For the reference's transform src_a = idx[i], src_b = idx[perm[i]] and (x0, y0) is the same for every i.
 * lq and gt are read in place through four ELEMENT strides (batch, channel, row, column); lq_out (b, Cl, p, p) and gt_out
 * (b, Cg, s p, s p) are contiguous.  16-byte accesses are used for a row segment only where source A, source B and the destination
 * are all 16-byte aligned there, 4-byte accesses elsewhere; no byte outside a window or outside the outputs is touched.
 * The host validates a plan before it uploads it; the kernel still leaves an output sample unwritten rather than follow an item
 * whose src_a / src_b is outside [0, B) or whose window leaves [0, P).  One launch, no workspace, no atomics, no host
 * synchronisation.
 *
 * Errors, nothing is launched.  GRL_ERR_BAD_ARG: a null args / lq / gt / items / lq_out / gt_out, a non-positive B, P, Cl, Cg, b,
 * p or s, p > P.  GRL_ERR_UNSUPPORTED: a pointer not aligned to 4 bytes, B C s P s P or b C s p s p of 2^31 elements or more for
 * either tensor, b above 65535, 2^31 or more four-element row slots in one output sample of lq and gt together. */
typedef struct GrlRemixItem {
    int32_t src_a, src_b;       /* input samples blended into this output sample                  */
    int32_t x0, y0;             /* LQ-side window origin: first row, first column                 */
    float lam;                  /* weight of src_a; read only when mix != 0                       */
} GrlRemixItem;

typedef struct GrlBatchRemixArgs {
    const float* lq;            /* (B, Cl, P, P)                                                  */
    int64_t lq_stride[4];       /* element strides of batch, channel, row, column                */
    const float* gt;            /* (B, Cg, s P, s P)                                              */
    int64_t gt_stride[4];
    int32_t B, P, Cl, Cg;
    int32_t b, p, s;            /* output batch, LQ-side output patch, scale                      */
    int32_t mix;
    const GrlRemixItem* items;  /* [b], device                                                    */
    float* lq_out;              /* (b, Cl, p, p)                                                  */
    float* gt_out;              /* (b, Cg, s p, s p)                                              */
} GrlBatchRemixArgs;

int grl_batch_remix(void* stream, const GrlBatchRemixArgs* args);

/* ---------------------------------------------------------------------------------------------
 * Spectral normalisation of the discriminator's convolutions (ABI 45, csrc/spectral_norm.hip, discriminator.py): every normalised
 * layer of a network in one call.
 *   restates  spectral_norm(nn.Conv2d(...)) on conv1 .. conv8                        models/aux_archs/discriminator.py:92-144
 *             SpectralNorm.compute_weight, one power iteration                       torch/nn/utils/spectral_norm.py
 * Per layer l < n_layers: W = w[l], fp32 row-major (cout[l], k[l]) -- the contiguous weight_orig (Cout, Cin, kh, kw) seen as a matrix,
 * k = Cin kh kw; u[l] (cout[l]) and v[l] (k[l]) the power-iteration vectors; out[l] of W's shape.  Any cout >= 1 and k >= 1.
 *
 * grl_spectral_norm_fwd, advance = 1 (a training forward):
 *   t = W^T u,  v' = t / max(|t|, 1e-12),  s = W v',  u' = s / max(|s|, 1e-12),  sigma = u' . s,  out = W / sigma
 * u[l] and v[l] are overwritten with u' and v'.  advance = 0 (eval): s = W v, sigma = u . s, out = W / sigma; u and v are only read.
 * In both modes u_keep[l] / v_keep[l] (each optional) receive the vectors sigma was formed with and *sigma[l] (optional) sigma itself:
 * the backward of THIS forward needs them after a later forward has advanced u and v.
 * Three launches (two with advance = 0), whatever n_layers.
 *
 * grl_spectral_norm_bwd: g[l] = d/d out[l]; u[l], v[l], *sigma[l] = what the forward left in u_keep, v_keep, sigma (read only);
 *   out[l] = dW = g / sigma - (<g, W> / sigma^2) u v^T        (u, v constants, as autograd treats them)
 * <g, W> is summed in double.  u_keep, v_keep and advance are not read.  Two launches.
 *
 * No atomics: every sum runs in an order fixed by the shapes, so equal inputs give equal bits, in any process.
 * ws: device scratch, 8-byte aligned, written before it is read.  ws_bytes at least
 *   fwd  4 * sum_l (ceil(cout[l] / 64) * k[l] + cout[l])        bwd  8 * sum_l ceil(cout[l] * k[l] / 4096)
 * Errors, nothing is launched.  GRL_ERR_BAD_ARG: a null args / ws / w / u / v / out (bwd: g / sigma too), n_layers outside
 * 1 .. GRL_SN_MAX_LAYERS, a non-positive cout or k, advance not 0 / 1, a pointer not 4-byte aligned, ws_bytes too small.
 * GRL_ERR_UNSUPPORTED: cout * k of 2^31 or more. */
#define GRL_SN_MAX_LAYERS 16
typedef struct GrlSpectralNormArgs {
    const float* w[GRL_SN_MAX_LAYERS];
    float* u[GRL_SN_MAX_LAYERS];
    float* v[GRL_SN_MAX_LAYERS];
    float* out[GRL_SN_MAX_LAYERS];      /* fwd: W / sigma; bwd: dW                                 */
    float* u_keep[GRL_SN_MAX_LAYERS];   /* fwd, optional                                            */
    float* v_keep[GRL_SN_MAX_LAYERS];   /* fwd, optional                                            */
    float* sigma[GRL_SN_MAX_LAYERS];    /* one float each; fwd: written (optional), bwd: read       */
    const float* g[GRL_SN_MAX_LAYERS];  /* bwd                                                      */
    int32_t cout[GRL_SN_MAX_LAYERS];
    int32_t k[GRL_SN_MAX_LAYERS];
    int32_t n_layers;
    int32_t advance;
    void* ws;
    int64_t ws_bytes;
} GrlSpectralNormArgs;

int grl_spectral_norm_fwd(void* stream, const GrlSpectralNormArgs* args);
int grl_spectral_norm_bwd(void* stream, const GrlSpectralNormArgs* args);

/* ---------------------------------------------------------------------------------------------
 * Tiled inference, the stitch (ABI 46, csrc/stitch.hip, tiling.py): the canvas accumulation of tiled whole-image inference for a
 * contiguous range of the tile list in one launch, with an optional blending window.
 *   restates  forward_tile: E += out, W += 1, E / W                                   engines/base.py:100-116
 * Inputs.  The reference's tile grid oy = tile_origins(h, tile, overlap), ox = tile_origins(w, tile, overlap) (input pixels,
 * strictly ascending); tile t = iy * nx + ix in row-major order, the reference's loop order; ts = tile * scale; a 1-D fp32 window
 * win[0 .. ts), strictly positive, a null pointer meaning all ones; a contiguous range [lo, hi) of the tile list; the fp32 outputs
 * of those tiles, each (b, c, ts, ts), read in place through their batch / channel / row ELEMENT strides (column stride 1).
 * tiles: DEVICE table of hi - lo rows of eight int64, row k for tile lo + k: the address of its element (0, 0, 0, 0), the batch,
 * channel and row stride, four reserved.  canvas: (b, c, h * scale, w * scale) fp32, contiguous.
 *
 * For a canvas pixel (y, x) the covering tiles C are those with oy[iy] * scale <= y < oy[iy] * scale + ts and likewise in x: a
 * contiguous range of iy times a contiguous range of ix -- of any length: with overlap > tile / 2, or a last tile that lands close to
 * its neighbour, three or more tiles per axis cover a pixel -- visited in row-major order.  For each channel and batch item:
 *   - if no tile of C lies in [lo, hi) the pixel is not touched: neither read nor written;
 *   - the running value starts at +0.0f if the first tile of C has index >= lo, else at the canvas value;
 *   - for each tile of C in [lo, hi), in order: acc = acc + o * wgt, wgt = win[y - oy * scale] * win[x - ox * scale]: three
 *     separately rounded fp32 operations, no FMA (the file is compiled with -ffp-contract=off);
 *   - if the last tile of C has index < hi the pixel is complete: acc = acc / wsum, an IEEE division, where wsum starts at +0.0f
 *     and adds wgt over ALL tiles of C in the same order;
 *   - the pixel is written once.
 * So the canvas may be uninitialised memory; a pixel is read only when an earlier chunk started it; there are no atomics and no
 * workspace; calling the entry chunk after chunk in list order gives the bits of one call with [0, n); with a null window that is
 * tiling.stitch (0 + o1 + o2 ... in the same order, divided by the exact count), and -0.0 inputs come out as +0.0, as in torch.
 * The grid covers the bounding box of the chunk's tiles only: its band of tile rows, and all columns unless it lies in one tile row.
 *
 * Errors, nothing is launched.  GRL_ERR_BAD_ARG: a null args / canvas / tiles, a non-positive b, c, h, w, tile, scale, ny or nx,
 * tile > h or tile > w, lo < 0, lo >= hi, hi > ny * nx, an origin list that does not ascend strictly or holds a tile outside the
 * canvas.  GRL_ERR_UNSUPPORTED: more than GRL_STITCH_MAX_ORIGINS origins on an axis, canvas or win not 4-byte or tiles not 8-byte
 * aligned, b * c above 65535, more than 4 * 65535 canvas rows in the chunk's band. */
#define GRL_STITCH_MAX_ORIGINS 256
typedef struct GrlTileStitchArgs {
    float* canvas;              /* (b, c, h * scale, w * scale), device                            */
    const int64_t* tiles;       /* [hi - lo][8], device                                            */
    const float* win;           /* [tile * scale], device, or null                                 */
    int32_t b, c, h, w;         /* the INPUT's shape                                               */
    int32_t tile, scale;
    int32_t ny, nx;
    int32_t lo, hi;
    int32_t oy[GRL_STITCH_MAX_ORIGINS];
    int32_t ox[GRL_STITCH_MAX_ORIGINS];
} GrlTileStitchArgs;

int grl_tile_stitch(void* stream, const GrlTileStitchArgs* args);

/* Debug aid (ABI 21; no reference counterpart): fills the LDS of every CU with 0xFF bytes (fp32 / fp16 NaN) by a launch on
 * `stream`.  LDS keeps what the previous workgroup left in it; a kernel that reads LDS it has not written is otherwise right or
 * wrong depending on what ran before it.  The Python wrappers call this before every launch when GRL_DIRTY_LDS=1 (tests). */
int grl_debug_dirty_lds(void* stream);

/* Library self-description (used by the loader to refuse a stale build). */
int grl_abi_version(void);
const char* grl_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* GRL_HIP_H */
