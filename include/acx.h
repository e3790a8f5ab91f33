/* acx.h -- C ABI of libacx, the MI355X (gfx950) hot-path library for AnomalyCLIP.
 *
 * The reference (lucazanella/AnomalyCLIP) is pure Python over stock PyTorch ops and has NO FFI of
 * its own; this header therefore defines the boundary SURVEY.md section 8(b) recommends: plain C
 * types, raw device pointers, caller-owned memory, one HIP stream per call.  Each entry point
 * names the reference code it replaces (paths relative to the reference repo).
 *
 * Conventions
 *   - every function returns 0 on success, a negative ACX_E_* code otherwise; the text of the
 *     last error is available from acx_last_error(ctx) (ctx may be NULL: thread-local slot).
 *   - never aborts, never throws across the ABI; asynchronous kernel faults surface at the
 *     caller's next synchronisation.
 *   - ALL buffers (inputs, outputs, weights, workspace) are owned by the caller (PyTorch);
 *     the library never allocates or frees device memory and retains no pointer after a call.
 *   - tensors are row-major; leading dimensions are in ELEMENTS.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).
 */
#ifndef ACX_H_
#define ACX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACX_VERSION 100 /* 0.1.0 */

enum {
  ACX_OK = 0,
  ACX_E_BADARG = -1,   /* null pointer, bad shape, misaligned leading dimension */
  ACX_E_UNSUPPORTED = -2, /* dtype / geometry this build has no kernel for */
  ACX_E_HIP = -3,      /* a HIP runtime call failed (text in acx_last_error) */
  ACX_E_WORKSPACE = -4, /* workspace too small */
  ACX_E_RCCL = -5      /* RCCL could not be opened, or an RCCL call failed (acx_comm_* / acx_allreduce / acx_allgather) */
};

enum { ACX_F32 = 0, ACX_BF16 = 1,                    /* storage dtypes */
       ACX_BF16X3 = 2,    /* OUTPUT only (acx_layernorm y_dtype, acx_gemm c_dtype of a pairs = 6 product): the value as three dense
                             bf16 planes hi | mid | lo [rows, ld] each, plane p at base + p * rows * ld elements -- the producer
                             writes the A operand of a pairs = 6 product directly */
       ACX_BF16X3P = 3 }; /* the same three planes in K-PANEL layout: a plane is [ld / 32][rows][32] -- the 32 columns of K-step kp
                             of all rows are contiguous (element (r, c) at ((c / 32) * rows + r) * 32 + c % 32; ld % 32 == 0,
                             dense).  The plane-reuse kernel then stages a 256-row x 32-column unit from ONE contiguous 16 KB block
                             instead of 256 half cache lines (acx_gemm_desc.panels) */
enum { ACX_F16 = 5,        /* acx_gemm_desc.a_dtype with pairs = 3: A and W are TWO fp16 planes each (acx_split_f16x2: x = hi + lo,
                              hi = fp16(x), lo = fp16(x - hi)) -- the ACX_PREC_F16X3 arithmetic: products (lo,hi) (hi,lo) (hi,hi) on
                              v_mfma_f32_32x32x16_f16, an error of ~2^-22 of sum |a||w| for operands inside fp16's range */
       ACX_F16X2P = 6 };   /* the two fp16 planes in K-panel layout (plane = [ld / 32][rows][32], plane p at base + p * rows * ld
                              elements): output of acx_layernorm / acx_vit_patches / an ACX_F16 product, input of the next one */
enum { ACX_BF16X2P = 4 };  /* acx_layernorm y_dtype / acx_vit_patches out_dtype: the ACX_BF16X3P image with the hi and mid planes written
                              only (the lo plane's bytes are left as they are): the A operand of a pairs = 3 product, which never reads
                              the lo plane.  A producer that does not special-case it writes all three planes. */
enum { ACX_PREC_F32 = 0, ACX_PREC_BF16 = 1,          /* MFMA arithmetic: exact f32 (v_mfma_f32_32x32x2_f32) or bf16 in / f32 acc */
       ACX_PREC_F32X3 = 3,    /* the same drivers and plane layouts with the THREE leading products only (acx_gemm_desc.pairs = 3:
                                 (mid, hi) (hi, mid) (hi, hi)): sixteen significant bits per operand -- an error of ~1e-5 of sum |a||w| per
                                 product, between TF32 and f32 -- at about twice the GEMM rate of ACX_PREC_F32X6.  NOT an f32-accurate
                                 path: opt-in (precision "bf16x3"); the planes attention takes its three-product form too (acx_attention_p3n) */
       ACX_PREC_F16X3 = 4,    /* the same drivers with TWO fp16 planes per operand and the three products (lo,hi) (hi,lo) (hi,hi):
                                 the fp16 pair holds the f32 value to 2^-24 (lo normal), every product is exact in f32, the dropped
                                 (lo,lo) term is <= 2^-22: f32-MFMA-level results at the three-product rate, for operands inside fp16's
                                 range (|x| < 65504; weights are pre-scaled by a power of two per matrix).  Opt-in (precision "f16x3") */
       ACX_PREC_F32X6 = 2 };  /* acx_vit_encode / acx_transformer_forward only: f32 everywhere, the four large GEMMs of a layer as
                                 f32-accurate bf16 x 6 products (acx_gemm_desc.pairs); the *_w_bf16 weight fields then hold THREE
                                 planes each (acx_split_bf16x3 of the f32 weight) */
enum { ACX_PREC_BF16X6 = 5 }; /* acx_resnet_encode only: the ResNet encoder's products as pairs = 6 products of bf16 planes (f32-accurate:
                                 the arithmetic ACX_PREC_F32X6 names in the ViT drivers).  A value of its own because ACX_PREC_F32X6 in
                                 acx_resnet_desc.prec means -- and keeps meaning -- the f32 MFMA kernels.  Opt-in (precision "bf16x6") */
enum { ACX_PREC_F32X6_LN16 = 6 }; /* acx_vit_encode_ln16 only: ACX_PREC_F32X6 with the two LayerNorm-fed products of a body layer -- the
                                 in-projection and c_fc -- as three-product GEMMs of fp16 planes (the ACX_PREC_F16X3 arithmetic) wherever
                                 they take the plane kernel.  ln_1 / ln_2 then write the two ACX_F16X2P planes of s * y, s a power of two
                                 per LayerNorm which the CALLER proves safe from the weights alone (|y_i| <= |gamma_i| sqrt(D - 1) +
                                 |beta_i| for any finite row); in_proj_w_bf16 / fc_w_bf16 hold two fp16 planes of 2^10 w
                                 (acx_split_f16x2, K-panel layout), out_proj_w_bf16 / proj_w_bf16 the three bf16 planes.  Per A element
                                 the planes' error is max(2^-22 |y|, 2^-25 / s).  Attention, out-proj, c_proj, the patch embedding and the
                                 pruned last layer are ACX_PREC_F32X6's.  Widths 768 and 1024 (the fp16 LayerNorm store).  A tools build with
                                 -DACX_LN16_FC_DEFAULT=0 keeps c_fc a six-product GEMM (fc_w_bf16: three bf16 planes; the A/B arm that
                                 measures the in-projection alone): acx_transformer_plan's ln2_dtype tells the caller which it is */
enum { ACX_PREC_F32X6_R16 = 7 };  /* acx_vit_encode_r16 only: ACX_PREC_F32X6_LN16 one step wider -- in every body layer the two residual
                                 products (out-proj, c_proj) read fp16 pair planes as well, where they and their producers take the plane
                                 kernels: the planes attention (acx_attention_p3f16) writes the two planes of s_att * o, c_fc's activation
                                 epilogue those of s_hid * hidden (acx_gemm_desc.c_scale); the weights come as acx_split_f16x2(2^10 w).
                                 s_att and s_hid are per-layer powers of two the CALLER proves from the weights alone (|o| is a convex
                                 combination of V rows; |act(x)| <= |x| for QuickGELU and for the exact GELU alike: x times a factor in [0, 1],
                                 sigmoid(1.702 x) or Phi(x)).  Everything else is ACX_PREC_F32X6_LN16's plan, record for
                                 record.  Tools builds: -DACX_R16_OUT_DEFAULT=0 / -DACX_R16_PROJ_DEFAULT=0 keep that product six-product */
enum { ACX_PREC_F32X6_QKV16 = 8 }; /* acx_vit_encode_qkv16 only: ACX_PREC_F32X6_R16 one step wider -- in every body layer whose attention is
                                 the planes attention behind an UNSPLIT plane-kernel in-projection, the in-projection writes the two fp16
                                 planes of s_qkv * (q | k | v) (acx_gemm_desc.c_scale, where ACX_PREC_F32X6_R16 writes f32 rows: the same
                                 bytes) and the attention runs its three-product fp16 form on them (acx_attention_p3h16: planes in by
                                 LDS-DMA, no split in the kernel), writing the planes of s_att * o.  s_qkv is a per-layer power of two the
                                 CALLER proves from the weights alone for ALL 3 W in-projection rows (the bound of s_att, taken over the Q
                                 and K rows too).  Everything else is ACX_PREC_F32X6_R16's plan, record for record; weights are bound as
                                 for ACX_PREC_F32X6_R16.  A tools build with -DACX_QKV16_DEFAULT=0 keeps ACX_PREC_F32X6_R16's records */
enum { ACX_PREC_F16X3S = 9 };     /* ACX_PREC_F16X3 on every ViT sequence length: the same planes (ACX_F16X2P), the same weights
                                 (acx_split_f16x2(2^10 w)), the same three products, the same "all four products on the plane kernel, or
                                 none" rule and the same fall-back to the f32 plan with an f32-sized workspace -- except the attention
                                 rule: non-causal 192 < L <= 208 keeps ACX_TF_ATT_P3N (products 103: ACX_PREC_F16X3's plan, record for
                                 record), every other non-causal L <= 1024 takes the streaming planes attention (ACX_TF_ATT_S16,
                                 acx_attention_s16).  Operands must lie inside fp16's range, as for ACX_PREC_F16X3: opt-in */
#define ACX_F16X3_WSCALE 1024.0f  /* ACX_PREC_F16X3: the weights' fp16 planes hold 2^10 * w (acx_split_f16x2: lifts CLIP-sized weights into
                                      fp16's normal range so that the lo plane keeps its 11 bits; |w| < 63.9); the drivers' products undo it */
enum { ACX_ACT_NONE = 0, ACX_ACT_QUICKGELU = 1, ACX_ACT_LEAKYRELU = 2,
       ACX_ACT_RELU = 3,      /* max(x, 0) in the activation slot (clip/model.py:18-22,122-130 ReLU after a folded BatchNorm) */
       ACX_ACT_RESRELU = 4 }; /* ReLU AFTER the residual add: C = max(residual + (acc + bias), 0) (clip/model.py:62-64, Bottleneck's
                                 `out += identity; relu3`); needs `residual`.  Both: f32 products (prec ACX_PREC_F32, pairs <= 1) on
                                 the identity or CONV3X3 row maps, no a_sub / positional epilogue; and pairs = 6 products: RELU on
                                 identity or CONV3X3 rows to f32 or plane output (ACX_BF16X3[P]: the planes of the value AFTER the
                                 ReLU), without a residual; RESRELU on identity rows to f32 output (whole tiles, no K split: both).
                                 pairs = 3 takes neither; ACX_E_UNSUPPORTED otherwise */
enum { ACX_ACT_GELU = 5 };    /* the exact GELU 0.5 x (1 + erf(x / sqrt 2)) (nn.GELU: every CLIP checkpoint NOT trained with QuickGELU --
                                 open_clip's LAION-2B / DataComp ViT-B/32, B/16, L/14), f32-accurate (erf, no tanh / sigmoid form).  The
                                 routes the two towers take: f32 products (prec ACX_PREC_F32, f32 A and C: the few-row, 64 x 64, 8-wave,
                                 strip-stream and generic kernels, with their K splits) and pairs = 6 / 3 products of planes, everywhere
                                 QuickGELU is taken, on identity rows.  ACX_E_UNSUPPORTED on the bf16 MFMA routes (prec ACX_PREC_BF16
                                 with pairs <= 1: no parity path) and on the CONV3X3 / tile row maps (no CLIP tower has a GELU there) */
enum { ACX_AMAP_IDENTITY = 0, ACX_AMAP_CONV3X3 = 1, ACX_AMAP_TESTTILE = 2, ACX_AMAP_TILETABLE = 3 };
enum { ACX_NORM_LAYER = 0, ACX_NORM_CHAN = 1 };     /* nn.LayerNorm vs axial_attention ChanLayerNorm (eps added to std) */

typedef struct acx_ctx acx_ctx;

int acx_version(void);
int acx_create(acx_ctx** out, int device);
void acx_destroy(acx_ctx* ctx);
const char* acx_last_error(acx_ctx* ctx);

/* Per-context tuning options (dispatch thresholds; results never depend on them beyond summation order).
 *   ACX_OPT_RING_MIN_TILES  bf16 GEMMs with at least this many 256x256 output tiles take the persistent
 *                           256x256 LDS-DMA kernel instead of the 128x128 one (default 512). */
/*   ACX_OPT_SK_MAX_M        f32 acx_gemm problems with at most this many rows take the few-row kernel (32x32 tiles,
 *                           K split over the waves, no split-K reduction launch; default 320; 0 disables it except
 *                           for the a_act / gelu_grad_of fusions, which always need it). */
/*   ACX_OPT_TN_P256_MIN_ROWS acx_gemm_tn problems with at least this many rows (and >= 8 output tiles of 256 x 256, no
 *                           b_sub) take the 256 x 256 LDS-DMA kernel (default 4096). */
/*   ACX_OPT_X6_CUS          the pairs = 6 kernels (acx_gemm, acx_gemm_tn_x6) are persistent, ONE workgroup per CU with the whole
 *                           register file and 144 KB of LDS: nothing else runs on a CU they hold.  value > 0 caps their grid
 *                           (and the K split is chosen for that many workgroups) so that the remaining CUs stay free for
 *                           kernels of OTHER streams -- the data-parallel step runs the text tower's ~160 few-row launches
 *                           beside the head's convolutions; 0 (default): all CUs. */
/*   ACX_OPT_X6_TAIL_SPLIT   pairs = 6 problems with more 256 x 256 tiles than CUs whose last round of tiles fills only part of the chip
 *                           (and a caller-provided workspace): 1 = the whole tile rows of the full rounds as one launch, the
 *                           remaining rows as a K-split problem + reduce launch (ViT c_proj at 512 frames: +0.7 %; the four
 *                           products at 256 frames: +4-5 % frames/s).  The tail rows then sum K in another order than the
 *                           rows before them: identical frames are no longer bit-identical wherever they sit in a launch, which
 *                           is why the default is 0. */
/*   ACX_OPT_X6_STRIP_TAIL   pairs = 6 problems (identity rows, N % 256 == 0) whose last round of 256 x 256 tiles fills only part of the
 *                           chip: 1 (default) = the tiles of that round are cut into 128- or 64-column strips (one work item each)
 *                           when the cost model says the round gets shorter.  A strip runs the same K order and product order
 *                           per output element as a whole tile: results are BIT-IDENTICAL to 0 (= whole tiles only); 2 / 3 force
 *                           128- / 64-column strips (measurements). */
/*   ACX_OPT_X6_MIN_TILES    ACX_PREC_F32X6 drivers (acx_vit_encode, acx_transformer_forward): a product with at least this many
 *                           256 x 256 output tiles runs as a pairs = 6 product, smaller ones on the f32 MFMA kernels (default 18:
 *                           the ViT from 8 frames per launch; measured crossover, profiles/r06_x6_strip_tail.txt). */
/*   ACX_OPT_LN_RIDER        acx_gemm_ln (and the ACX_PREC_F32X6 drivers, which call it for out-proj -> ln_2 and c_proj -> the next ln_1):
 *                           1 (default) = the workgroups that have no tile in a residual product's partly filled last round run
 *                           LayerNorm rows beside it, as many as the cost model says fit; 0 = product, then LayerNorm; > 1 = ride up
 *                           to this many of the completed rows (measurements).  Results are BIT-IDENTICAL for every value. */
/*   ACX_OPT_ATTN_F32IN     ACX_PREC_F32X6 drivers, six-product mode, layers whose attention is acx_attention_p3: 1 (default) = the
 *                           in-projection writes f32 rows and the attention splits q | k | v into planes itself (acx_attention_p3f:
 *                           no plane round trip through memory); 0 = the in-projection's epilogue writes the three planes and
 *                           acx_attention_p3 reads them.  Results are BIT-IDENTICAL for both values. */
/*   ACX_OPT_CLS_FOLD       acx_vit_encode, every precision but ACX_PREC_BF16: 1 (default) = the pruned last layer runs without its
 *                           K | V product -- ln_1 and Q for the CLS rows, then acx_attention_cls_fold on the residual stream; 0 = ln_1
 *                           of all rows, the K | V product and acx_attention_cls.  Both are f32-level evaluations of the same layer:
 *                           the features differ by round-off (not bit-identical).  A geometry with 2 heads > 3 tokens per frame (the
 *                           fold's scratch would not fit in the layer's free q | k | v buffer) runs the K | V path for both values. */
enum { ACX_OPT_RING_MIN_TILES = 1, ACX_OPT_SK_MAX_M = 2, ACX_OPT_TN_P256_MIN_ROWS = 3, ACX_OPT_X6_CUS = 4, ACX_OPT_X6_TAIL_SPLIT = 5,
       ACX_OPT_X6_STRIP_TAIL = 6, ACX_OPT_X6_MIN_TILES = 7, ACX_OPT_LN_RIDER = 8, ACX_OPT_ATTN_F32IN = 9, ACX_OPT_CLS_FOLD = 10 };
int acx_set_option(acx_ctx* ctx, int32_t option, int64_t value);
/* *value = the option as acx_create set it or acx_set_option last stored it (what the library acts on: a value the setter clamps
 * reads back clamped).  ACX_E_UNSUPPORTED for an unknown option, as the setter. */
int acx_get_option(acx_ctx* ctx, int32_t option, int64_t* value);

/* ------------------------------------------------------------------------------------------
 * acx_gemm: C[M,N] = epilogue( amap(A)[M,K] . W[N,K]^T )            (MFMA-bound workhorse)
 * replaces every nn.Linear / F.linear / `@` / nn.Conv2d on the path:
 *   clip/model.py:192,197-199 (QKV, out-proj, MLP), :246-252 (patch conv as GEMM), :287-288
 *   (proj), text_encoder.py:23, temporal_model.py:31,43 (projection), axial_attention
 *   SelfAttention.to_q/to_kv/to_out and the two 3x3 convs of each feed-forward (implicit GEMM),
 *   selector_model.py:62 is a separate HBM-bound kernel (acx_selector_*).
 * epilogue order: +bias[n] -> activation -> +pos0[(m/gl)%gn][n] -> +pos1[m%gl][n] -> +residual[m][n]
 */
typedef struct acx_gemm_desc {
  const void* A;          /* [rows_of_A, lda]  f32 or bf16 */
  const void* W;          /* [N, ldw]          f32 (PREC_F32) or bf16 (PREC_BF16) */
  void* C;                /* [M, ldc]          f32 or bf16 */
  int32_t M, N, K;
  int32_t lda, ldw, ldc;
  int32_t a_dtype, c_dtype;
  int32_t prec;
  const float* bias;      /* [N] or NULL */
  int32_t act;
  const float* residual;  /* [M, ldr] f32 or NULL (may alias C) */
  int32_t ldr;
  const float* a_sub;     /* [K] subtracted from every A row before the product, or NULL
                             (selector_model.py:54 / anomaly_clip.py:143,201 re-centring) */
  int32_t amap;           /* ACX_AMAP_* */
  int32_t gn, gl;         /* grid (num_segments, seg_length) for CONV3X3 / TESTTILE / pos */
  int32_t cin;            /* CONV3X3: input channels; K == 9*cin, W laid out [N][tap=kh*3+kw][cin] */
  int32_t seg;            /* TESTTILE: segment_size S; row ((b s) n l) reads source row ((b n s l))
                             (temporal_model.py:46-53) */
  const float* pos0;      /* [gn, N] axial positional embedding param_0 (or NULL) */
  const float* pos1;      /* [gl, N] axial positional embedding param_1 (or NULL) */
  void* workspace;        /* optional: enables split-K for skinny problems (few output tiles, long K); */
  size_t workspace_bytes; /* how much to bring: acx_gemm_scratch; less is fine (fewer splits or none)  */
  /* Few-row fusions of the text tower (clip/model.py:183-185,188-230 and its dX chain).  Both need the few-row f32
   * kernel: f32 operands, identity row map, K % 256 == 0, N % 4 == 0, 16-byte aligned C / residual / gelu_grad_of;
   * ACX_E_UNSUPPORTED otherwise. */
  const void* zero_page;  /* optional: >= 256 bytes of zeros, 16-byte aligned, caller-owned.  With it, large CONV3X3 problems
                             (N >= 512, power-of-two grid, no residual) run on the LDS-DMA strip kernel: a tap outside the
                             token grid is a DMA from this page */
  int32_t a_act;          /* ACX_ACT_QUICKGELU / ACX_ACT_GELU: the activation is applied to A as it is read (x_next = gelu(pre) @ W^T) */
  const float* gelu_grad_of; /* [M, ldg] saved pre-activation p: C = (A W^T + bias) * d gelu(p)/dp  (no residual).  WHICH gelu: `act`
                                names it -- act = 0 (ACX_ACT_NONE) keeps meaning QuickGELU's derivative, act = ACX_ACT_GELU selects the
                                exact GELU's, Phi(p) + p phi(p); no activation is applied to C either way.  Any other act: refused */
  int32_t ldg;
  const float* a_norm_w;  /* LayerNorm over K applied to the A rows as they are read (y = LN(A) W^T + bias): weight / bias [K], or
                             NULL.  Few-row f32 kernel only, K == 512, no a_act / residual / gelu_grad_of / activation
                             (clip/model.py:214-216 ln_1 -> in_proj, ln_2 -> c_fc of the text tower); ACX_E_UNSUPPORTED otherwise */
  const float* a_norm_b;
  float a_norm_eps;
  uint32_t* counters;     /* optional: n_counters uint32, ZERO before the first call and left zero by every call (caller-owned,
                             one table per stream).  With it and `workspace`, few-row problems with K >= 1024 split K across
                             workgroups whose partial tiles meet through a last-arriver reduction (no second launch). */
  int32_t n_counters;
  const int32_t* tile_table; /* TILETABLE: [M / (gn gl)][2] device ints (base row, row stride between segments): output row
                                (tile, n, l) reads source row base + n * stride + l -- the test-mode tiling of
                                temporal_model.py:46-53 for a batch of videos with DIFFERENT segment sizes (video v, tile s:
                                base = row0_v + s gl, stride = S_v gl) */
  int32_t pairs;          /* 0 / 1: plain.  6 (with prec = ACX_PREC_BF16, a_dtype = ACX_BF16): f32-ACCURATE product on the bf16 matrix
                             cores.  A and W are each THREE bf16 planes (acx_split_bf16x3: x = hi + mid + lo to 24 bits; plane p of
                             A at A + p * a_plane_stride bytes, of W at W + p * w_plane_stride), and C accumulates, in f32, the six
                             cross products whose magnitude is >= 2^-16 of the leading one -- (hi,lo) (mid,mid) (lo,hi) (hi,mid)
                             (mid,hi) (hi,hi): per 32-wide k range, smallest first.  Every bf16 x bf16 product is exact in f32; the
                             three dropped terms and the split remainders are <= 2^-23 of the product: the error is that of an
                             f32 dot product, at 6/16 of the f32 MFMA's cost (2.5 PFLOP/s bf16 against 157 TFLOP/s f32 on gfx950).
                             Kernel: gemm_x6_p4_kernel (csrc/acx_gemm_x6.h).  K % 32 == 0, N % 4 == 0, 16-byte aligned planes; row
                             maps IDENTITY and CONV3X3 (cin % 32 == 0, zero_page, an A plane below 4 GiB); epilogues bias,
                             QuickGELU / GELU / LeakyReLU / ReLU, residual (f32 C), c_dtype ACX_F32 / ACX_BF16 / ACX_BF16X3[P] (plane output:
                             N % 8 == 0, no residual).  CONV3X3 on a power-of-two (gn, gl) grid with M % 256 == 0 takes every one of
                             these; on ANY other grid or row count (gn, gl >= 1, M % (gn gl) == 0: a 256-row tile may straddle frames
                             and end behind M) the row map works by division and the epilogues are bias / ReLU to f32 and ReLU to
                             planes, without a residual or a K split.  With `workspace`, launches of fewer output tiles than CUs
                             split K across workgroups (fixed split per shape; partial tiles + the generic reduce launch) -- except
                             the ReLU epilogues and the general convolution map, which never split (acx_gemm_scratch answers 0).
                             3: the same planes and kernel with the THREE leading products only -- (mid,hi) (hi,mid) (hi,hi); the lo
                             planes are never read.  The dropped terms are <= 2^-16 of the leading one: NOT f32-accurate (about 1e-5 of
                             sum |a||w|).  Identity rows, f32 or plane outputs, bias / QuickGELU / GELU / residual epilogues. */
  int32_t panels;         /* pairs = 6: bit 0 -- the A planes are in K-panel layout (ACX_BF16X3P, rows = a_plane_stride / (2 K));
                             bit 1 -- the W planes are (rows = N).  Identity row map only. */
  int64_t a_plane_stride, w_plane_stride;   /* bytes */
  int64_t c_plane_rows;   /* plane outputs (ACX_BF16X3 / ACX_BF16X3P): rows of the WHOLE plane image when C addresses a row sub-range of
                             it (plane p of the output at C + p * c_plane_rows * ldc elements; K-panel rows counted over c_plane_rows);
                             0: M.  acx_gemm uses it itself when it splits a launch into full rounds of tiles + a K-split tail. */
  float out_scale;        /* pairs = 3 with fp16 planes (a_dtype = ACX_F16): the accumulator is multiplied by this power of two before bias
                             / activation / residual (operand planes that were scaled by acx_split_f16x2); 0 = 1 */
  float c_scale;          /* pairs = 3 with fp16 planes and c_dtype = ACX_F16X2P: the output planes hold c_scale * value -- one multiply by
                             this power of two behind the activation (the next product's A operand, whose out_scale undoes it); 0 = 1.
                             Not read otherwise.  (It fills the padding behind out_scale: the descriptor's size is what it was.) */
} acx_gemm_desc;
int acx_gemm(acx_ctx* ctx, const acx_gemm_desc* d, void* stream);

/* The scratch to hand to acx_gemm / acx_gemm_ln with this descriptor (the *_workspace_bytes query of acx_gemm): workspace_bytes of
 * `workspace` (0: hand none -- a workspace can change the route as well as the split), counters != 0: hand the arrival-counter table
 * too.  The routes choose their K split from the size they are given, so two callers that follow the query sum in the same order.
 * Host arithmetic only, no device work: it reads the shape fields and tests residual, a_sub, pos0, zero_page, ... for NULL; no pointer
 * of the descriptor is dereferenced, d->workspace and d->counters are ignored.  allow_split = 0: no K split across workgroups is
 * wanted (nothing to bring).  ctx == NULL: 256 workgroups and the option values acx_create sets; else the context's CU count,
 * ACX_OPT_SK_MAX_M, ACX_OPT_X6_CUS and ACX_OPT_X6_TAIL_SPLIT. */
typedef struct acx_gemm_scratch_t {
  size_t workspace_bytes;
  int32_t counters;
} acx_gemm_scratch_t;
int acx_gemm_scratch(const acx_ctx* ctx, const acx_gemm_desc* d, int32_t allow_split, acx_gemm_scratch_t* out);

/* acx_gemm_route: which kernel route acx_gemm takes with this descriptor, and how it splits K -- answered by the dispatcher's own
 * walk through its routes, which stops where the first launch would be (there is no second copy of the gates).  Host arithmetic, no
 * device, nothing launched; no operand is dereferenced (A, W and C must be non-NULL and aligned as for acx_gemm: dummy addresses do).
 * Unlike acx_gemm_scratch it READS workspace, workspace_bytes, counters and n_counters as values: the route and the split depend on
 * them.  Returns what acx_gemm would return before its first launch: ACX_OK, or the refusal's ACX_E_* with the same text in
 * acx_last_error (*out is then route = ACX_GEMM_ROUTE_NONE, ksplit = 1).  ctx == NULL: 256 workgroups and the option values
 * acx_create sets.
 *   route   ACX_GEMM_ROUTE_*, one per route function of csrc/acx_gemm.hip
 *   ksplit  K pieces across workgroups (1: none); X6_TAIL_SPLIT: the pieces of the tail's rows
 *   reduce  0 no split; 1 the pieces are summed by a reduce launch (which applies the epilogue); 2 they meet through the arrival
 *           counters inside the kernel (no second launch)
 *   tiles   output tiles of the launch in the route's own tile size: SK 32 x 32, S64 64 x 64, P256 / W8 / W8_CONV / DMA / DMA_CONV /
 *           GENERIC 128 x 128, X6 / X6_TAIL_SPLIT / RING / P8 256 x 256 (persistent kernels: tiles, not workgroups) */
enum { ACX_GEMM_ROUTE_NONE = 0, ACX_GEMM_ROUTE_X6_TAIL_SPLIT = 1, ACX_GEMM_ROUTE_SK = 2, ACX_GEMM_ROUTE_X6 = 3, ACX_GEMM_ROUTE_S64 = 4,
       ACX_GEMM_ROUTE_P256 = 5, ACX_GEMM_ROUTE_W8 = 6, ACX_GEMM_ROUTE_W8_CONV = 7, ACX_GEMM_ROUTE_RING = 8, ACX_GEMM_ROUTE_P8 = 9,
       ACX_GEMM_ROUTE_DMA_CONV = 10, ACX_GEMM_ROUTE_DMA = 11, ACX_GEMM_ROUTE_GENERIC = 12 };
typedef struct acx_gemm_route_t {
  int32_t route, ksplit, reduce;
  int32_t reserved;
  int64_t tiles;
} acx_gemm_route_t;
int acx_gemm_route(const acx_ctx* ctx, const acx_gemm_desc* d, acx_gemm_route_t* out);

/* acx_gemm_ln: acx_gemm(d) followed by the LayerNorm of ITS OUTPUT rows -- x = d->C ([M, N] f32, ldc == N), y = norm(x) * w + b as
 * acx_layernorm(x, ldc, w, b, y, N, y_dtype, M, N, eps, mode) writes it -- with the same bits as those two calls.  A pairs = 6 product
 * with the f32 residual epilogue (identity rows, N = 768 or 1024, even M, y_dtype = ACX_BF16X3P) whose last round of 256 x 256 tiles
 * fills only part of the chip goes out as (1) its full rounds, (2) its last round -- whole tiles or strips -- on one workgroup per
 * CU, where the workgroups without a tile normalise rows that (1) completed and write their planes, (3) acx_layernorm's kernel on
 * the rows that did not ride.  No workgroup waits for another.  y may be the product's own A planes (the ViT's out-proj reads and
 * ln_2 writes the same buffer): the riders write plane rows no tile of (2) reads.  ACX_OPT_LN_RIDER = 0: always the two calls. */
typedef struct acx_ln_job {
  const float* w;         /* [N] */
  const float* b;         /* [N] */
  void* y;                /* output of y_dtype (K-panel planes: [3][N / 32][M][32] bf16, 16-byte aligned) */
  int32_t y_dtype;
  float eps;
  int32_t mode;           /* ACX_NORM_* */
  float y_scale;          /* y_dtype = ACX_F16X2P (N = 768 or 1024): the planes hold y_scale * y, a power of two; 0 = 1.  Not read otherwise.
                             The struct GREW by this member with ACX_F16X2P jobs (a dtype acx_gemm_ln refused before): a caller built
                             against the earlier header never names that dtype, and the member is read for it alone */
} acx_ln_job;
int acx_gemm_ln(acx_ctx* ctx, const acx_gemm_desc* d, const acx_ln_job* job, void* stream);
/* host-side plan of acx_gemm_ln for an eligible product on `ncu` workgroups (no device needed): returns the rows that ride (even;
 * 0: none -- no partial round, a K split (ksplit > 1), or no workgroup without a tile), *rows_ready (may be NULL) = the rows the
 * full rounds complete.  rate: LayerNorm rows of 768 columns per microsecond and rider workgroup, <= 0: the library's constant. */
int64_t acx_gemm_ln_plan(int32_t M, int32_t N, int32_t K, int32_t ncu, int32_t ksplit, double rate, int64_t* rows_ready);

/* ------------------------------------------------------------------------------------------
 * acx_layernorm: y[r,:] = norm(x[r,:]) * w + b     (HBM-bound; one wavefront per row)
 * replaces clip/model.py:174-180 (LayerNorm), classification_head.py:7,12, axial PreNorm and
 * ChanLayerNorm.  D in {64, 128, 256, 512, 640, 768, 1024, 1280} (1280: every y_dtype but ACX_F16X2P)... rows gathered with stride ldx. */
int acx_layernorm(acx_ctx* ctx, const float* x, int64_t ldx, const float* w, const float* b,
                  void* y, int64_t ldy, int32_t y_dtype, int64_t rows, int32_t D, float eps,
                  int32_t mode, void* stream);
/* y_dtype = ACX_F16X2P (D = 768 or 1024, y dense and 16-byte aligned) with the planes of y_scale * y: y_scale a power of two (0 = 1), the
 * multiply is exact.  The caller keeps |y_scale * y| inside fp16's range */
int acx_layernorm_scaled(acx_ctx* ctx, const float* x, int64_t ldx, const float* w, const float* b, void* y, int64_t rows,
                         int32_t D, float eps, int32_t mode, float y_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * acx_attention: multi-head softmax(q k^T / sqrt(64)) v for head dim 64; causal L <= 224, non-causal L <= 1024
 * (L > 224: out 16-byte aligned with ldo % 4 == 0, and a non-NULL ctx -- a NULL ctx keeps the earlier answer ACX_E_UNSUPPORTED
 * above 224, the contract context-free callers had before longer sequences were supported).  Replaces nn.MultiheadAttention's core as used by clip/model.py:206-212
 * (ViT: L = 50 / 197 / 257 / 577 for B/32, B/16, L/14, L/14@336px, no mask; text: L=77, causal mask clip/model.py:386-392).  qkv: [batch*L, 3*heads*64] packed as
 * in_proj output (q | k | v); out: [batch*L, heads*64]. */
int acx_attention(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo,
                  int32_t batch, int32_t L, int32_t heads, int32_t causal, void* stream);
/* acx_attention_route: which kernel acx_attention (and _x3 / _x3_panel, which take the two streaming routes only) runs a sequence
 * on -- the rule the dispatcher itself switches on.  Arithmetic on the arguments: no device, nothing dereferenced, ctx may be NULL.
 * out_aligned: out is 16-byte aligned and ldo % 4 == 0.  BLOCK32: attn_kernel<NT, NW>, one workgroup per (sequence, head), 32-key
 * blocks, L <= 224; STREAM16: attn16_kernel, 16-key tiles streamed through LDS, 128 < L <= 256 non-causal; STREAM16_QB: the same
 * with several query blocks per (sequence, head), L > 256.  A negative answer is the error code acx_attention gives for the shape. */
enum { ACX_ATTN_ROUTE_BLOCK32 = 1, ACX_ATTN_ROUTE_STREAM16 = 2, ACX_ATTN_ROUTE_STREAM16_QB = 3 };
int acx_attention_route(const acx_ctx* ctx, int32_t L, int32_t causal, int32_t out_aligned);
/* the same (non-causal ViT sequences, 128 < L <= 1024) with the output as three bf16 planes hi | mid | lo (ACX_BF16X3:
 * plane p at (uint16_t*)out_planes + p * batch * L * ldo): the out-projection's A operand in ACX_PREC_F32X6 mode */
int acx_attention_x3(acx_ctx* ctx, const float* qkv, int64_t ldqkv, void* out_planes, int64_t ldo,
                     int32_t batch, int32_t L, int32_t heads, void* stream);
/* The ViT attention on the bf16 matrix cores at f32 accuracy (clip/model.py:206-212 in the ACX_PREC_F32X6 mode): q | k | v as
 * three bf16 planes in K-panel layout (ACX_BF16X3P of the in-projection output [batch * L, 3 heads * 64]: plane p at
 * (uint16_t*)qkv_planes + p * batch * L * 3 * heads * 64), S = Q K^T and O = P V as six-product bf16 x 6 products with f32
 * accumulation, softmax in f32; output = three bf16 planes of [batch * L, heads * 64] in K-panel layout (the out-projection's
 * A operand).  Non-causal, 192 < L <= 208 (seven 32-query tiles: the ViT-B/16 sequence of 197). */
int acx_attention_p3(acx_ctx* ctx, const void* qkv_planes, void* out_planes, int32_t batch, int32_t L, int32_t heads, void* stream);
/* ... with the number of cross products per contraction: 6 (= acx_attention_p3), 3 (the three leading ones: the operands' lo planes
 * are not read, the output's lo plane is not written -- the ACX_PREC_F32X3 mode, not f32-accurate), or 103 = three products on TWO
 * fp16 planes per operand (ACX_F16X2P images of q | k | v in, of the output out: the ACX_PREC_F16X3 mode) */
int acx_attention_p3n(acx_ctx* ctx, const void* qkv_planes, void* out_planes, int32_t batch, int32_t L, int32_t heads, int32_t products,
                      void* stream);
/* acx_attention_p3 fed with the in-projection's f32 rows: qkv [batch * L, 3 heads * 64] f32 (16-byte aligned, ldqkv % 4 == 0); the
 * kernel splits q | k | v into the three planes as it stages them -- the same split, the same products in the same order: the
 * output planes equal acx_attention_p3's on acx_split_bf16x3_panel(qkv) bit for bit.  Six products only; same L gate. */
int acx_attention_p3f(acx_ctx* ctx, const float* qkv, int64_t ldqkv, void* out_planes, int32_t batch, int32_t L, int32_t heads,
                      void* stream);
/* acx_attention_p3f with the output as the TWO fp16 planes of out_scale * o in K-panel layout (ACX_F16X2P): q | k | v, both
 * contractions and the softmax are acx_attention_p3f's six-product bf16 arithmetic, only the epilogue differs -- the planes equal
 * acx_split_f16x2(out_scale * o, panel) of the f32 value o whose three bf16 planes acx_attention_p3f writes, bit for bit.  out_scale: a
 * power of two in [2^-20, 2^20]; the caller keeps |out_scale * o| inside fp16's range (|o| <= max |v|). */
int acx_attention_p3f16(acx_ctx* ctx, const float* qkv, int64_t ldqkv, void* out_planes, float out_scale, int32_t batch, int32_t L,
                        int32_t heads, void* stream);
/* acx_attention_p3n's products = 103 form on scaled planes: qkv_planes = the two fp16 planes (ACX_F16X2P, K-panel layout) of in_scale *
 * (q | k | v), out_planes = those of out_scale * o.  in_scale^2 folds into the exponent's factor, out_scale / in_scale into the
 * normaliser: both exact (powers of two in [2^-20, 2^20], checked).  The planes equal acx_split_f16x2(out_scale * o, panel) of the f32
 * value o the kernel holds, bit for bit.  The caller keeps in_scale * |q, k, v| inside fp16's range.  Same L gate. */
int acx_attention_p3h16(acx_ctx* ctx, const void* qkv_planes, float in_scale, void* out_planes, float out_scale, int32_t batch, int32_t L,
                        int32_t heads, void* stream);
/* acx_attention_p3h16's contract without the L gate -- the streaming kernel.  qkv_planes: the two fp16 planes (ACX_F16X2P, K-panel
 * layout) of in_scale * (q | k | v), [batch * L, 3 * heads * 64]; out_planes: those of out_scale * o, [batch * L, heads * 64].  Products
 * hi.hi, hi.lo, lo.hi in both contractions (v_mfma_f32_*_f16, f32 accumulation), softmax in f32 with a running max and sum over chunks
 * of 64 keys, P split into an fp16 pair as it is consumed.  Non-causal, head dim 64, 1 <= L <= 1024; in_scale / out_scale powers of two
 * in [2^-20, 2^20] (in_scale^2 folds into the exponent's factor, out_scale / in_scale into the normaliser: exact).  64 KB of LDS whatever
 * L; nothing outside the [batch * L] rows of either buffer is read or written.  Refusals, all before any launch: ACX_E_UNSUPPORTED for
 * L outside 1..1024, ACX_E_BADARG for batch < 1, heads < 1, a scale that is no power of two in range, planes not 16-byte aligned. */
int acx_attention_s16(acx_ctx* ctx, const void* qkv_planes, float in_scale, void* out_planes, float out_scale, int32_t batch, int32_t L,
                      int32_t heads, void* stream);
/* ... with the planes in K-panel layout (ACX_BF16X3P: [ldo / 32][batch * L][32] each; ldo == heads * 64) */
int acx_attention_x3_panel(acx_ctx* ctx, const float* qkv, int64_t ldqkv, void* out_planes, int64_t ldo,
                           int32_t batch, int32_t L, int32_t heads, void* stream);

/* ------------------------------------------------------------------------------------------
 * Head dimension 80 (open_clip's ViT-H-14: width 1280 = 16 heads of 80).  Exact f32, non-causal, 1 <= L <= 1024: softmax(q k^T /
 * sqrt(head_dim)) v with the scale head_dim^-0.5 applied to q in f32.  qkv [batch * L, ldqkv] packed q | k | v of heads * head_dim
 * columns each (16-byte aligned, ldqkv % 4 == 0); out [batch * L, ldo], 16-byte aligned with ldo % 4 == 0.  One streaming kernel
 * (f32 MFMAs, K and V through LDS in chunks of 32 keys, online softmax) serves every L.
 * Error codes, all before any launch: null pointer ACX_E_BADARG; head_dim other than 80 ACX_E_UNSUPPORTED with the value in
 * acx_last_error -- 64 is REFUSED, not forwarded: acx_attention and its variants stay the entry points of head dimension 64; L outside
 * 1..1024 or heads <= 0 ACX_E_UNSUPPORTED; a misaligned qkv or a leading dimension too small ACX_E_BADARG; an out that is not 16-byte
 * aligned with ldo % 4 == 0 ACX_E_UNSUPPORTED.  batch <= 0 is ACX_OK (nothing to do). */
int acx_attention_hd(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo, int32_t batch, int32_t L, int32_t heads,
                     int32_t head_dim, void* stream);
/* ... with the output as three bf16 planes hi | mid | lo, plane p at (uint16_t*)out_planes + p * batch * L * ldo.  panel = 0: row-major
 * (ACX_BF16X3); panel != 0: K-panel layout (ACX_BF16X3P: [ldo / 32][batch * L][32] each; ldo % 32 == 0, ldo >= heads * head_dim -- with an
 * odd number of heads the last panel is half used) */
int acx_attention_x3_hd(acx_ctx* ctx, const float* qkv, int64_t ldqkv, void* out_planes, int64_t ldo, int32_t batch, int32_t L,
                        int32_t heads, int32_t head_dim, int32_t panel, void* stream);
/* ... for query row 0 of every sequence only (out [batch, ldo]; no alignment asked of out): the pruned last ViT layer */
int acx_attention_cls_hd(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo, int32_t batch, int32_t L, int32_t heads,
                         int32_t head_dim, void* stream);
/* which kernel route acx_attention_hd / _x3_hd take: STREAM one item per (sequence, head), L <= 128 (up to 8 query tiles, one per wave);
 * STREAM_QB ceil(ceil(L / 16) / 8) query blocks per (sequence, head), L > 128.  Arithmetic on the arguments, ctx may be NULL.  A negative answer is
 * the error code the entry points give: ACX_E_UNSUPPORTED for head_dim != 80, L outside 1..1024, or out_aligned == 0. */
enum { ACX_ATTN_HD_ROUTE_STREAM = 1, ACX_ATTN_HD_ROUTE_STREAM_QB = 2 };
int acx_attention_hd_route(const acx_ctx* ctx, int32_t L, int32_t head_dim, int32_t out_aligned);

/* bf16 variant of acx_attention for the bf16 mode of the ViT (NOT a parity path): qkv [batch*L, ldqkv] and out
 * [batch*L, ldo] are bf16, QK^T and PV run on the bf16 MFMA, softmax in f32.  Non-causal only. */
int acx_attention_bf16(acx_ctx* ctx, const void* qkv, int64_t ldqkv, void* out, int64_t ldo, int32_t batch,
                       int32_t L, int32_t heads, void* stream);
/* acx_attention_cls: same attention, but only for query row 0 of every sequence (out [batch, heads*64]); 0 < L <= 1024.
 * Used for the LAST ViT layer, whose output is consumed at the CLS token only (clip/model.py:285). */
int acx_attention_cls(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo,
                      int32_t batch, int32_t L, int32_t heads, void* stream);
/* acx_attention_cls_fold: what ln_1 -> K | V rows of in_proj -> acx_attention_cls computes, WITHOUT the K | V product.  With one
 * query per (frame, head) the key projection folds into the query (u_h = W_{k,h}^T q_h: q_h . b_k is the same for every key and
 * cancels in the softmax) and the value projection into the output (o_h = W_{v,h} sum_j p_j ln_1(x_j) + b_{v,h}, since sum_j p_j = 1).
 *   x [batch * L, W] f32 (dense, 16-byte aligned): the residual stream;  ln_w, ln_b [W], eps: ln_1;  in_proj_w [3 W, W], in_proj_b
 *   [3 W]: the f32 in-projection (its K and V rows are read);  q [batch, ldq]: the CLS rows' queries (W_q ln_1(x_0) + b_q, unscaled);
 *   out [batch, ldo] f32.  W = 64 heads, W in {64, 128, 256, 512, 640, 768, 1024} (the LayerNorm widths), 0 < L <= 1024.
 * workspace: acx_attention_cls_fold_workspace_bytes(batch, heads) bytes, 16-byte aligned.  A frame's output is a function of that
 * frame's rows alone: bit-identical for every batch size and position. */
size_t acx_attention_cls_fold_workspace_bytes(int32_t batch, int32_t heads);
int acx_attention_cls_fold(acx_ctx* ctx, const float* x, const float* ln_w, const float* ln_b, float eps, const float* in_proj_w,
                           const float* in_proj_b, const float* q, int64_t ldq, float* out, int64_t ldo, int32_t batch, int32_t L,
                           int32_t W, int32_t heads, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * acx_vit_patches: im2col of PxP/P patches, P even and R % P == 0 (P = 14 / 16 / 32: clip/model.py:246-252,267-269).
 * frames [F,3,R,R] f32 -> patches [F*g*g, 3*P*P] (k = c*P*P + ky*P + kx, token = gy*g+gx); out_dtype ACX_F32, ACX_BF16, or
 * ACX_BF16X3P (three bf16 planes of the f32 pixels in K-panel layout: the patch embedding's A operand in ACX_PREC_F32X6; the plane
 * layouts need 3 P P % 32 == 0, which P = 14 does not meet). */
int acx_vit_patches(acx_ctx* ctx, const float* frames, void* patches, int32_t out_dtype,
                    int32_t F, int32_t R, int32_t P, void* stream);
/* acx_vit_embed: x[f,0,:] = cls + pos[0]; x[f,1+t,:] = patch_out[f,t,:] + pos[1+t]; then ln_pre
 * (clip/model.py:270-279).  patch_out [F*T, W] f32 -> x [F*(T+1), W] f32. */
int acx_vit_embed(acx_ctx* ctx, const float* patch_out, const float* cls, const float* pos,
                  const float* ln_w, const float* ln_b, float* x, int32_t F, int32_t T, int32_t W,
                  void* stream);

/* Transformer block weights (clip/model.py:188-217).  All f32 masters; the *_bf16 pointers are
 * the bf16 copies used when prec == ACX_PREC_BF16, or -- prec == ACX_PREC_F32X6 -- the THREE bf16 planes of the f32 weight in
 * K-panel layout (acx_split_bf16x3_panel: plane p at base + p * rows * cols * 2 bytes); may be NULL otherwise. */
typedef struct acx_block_weights {
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
  const float *in_proj_w, *in_proj_b;     /* [3W, W], [3W] */
  const float *out_proj_w, *out_proj_b;   /* [W, W], [W] */
  const float *fc_w, *fc_b;               /* [4W, W], [4W] */
  const float *proj_w, *proj_b;           /* [W, 4W], [W] */
  const void *in_proj_w_bf16, *out_proj_w_bf16, *fc_w_bf16, *proj_w_bf16;
} acx_block_weights;

typedef struct acx_vit_weights {
  const float* conv1_w;       /* [W, 3*P*P]  (conv1.weight viewed 2-D) */
  const void* conv1_w_bf16;
  const float* class_embedding;  /* [W] */
  const float* positional_embedding; /* [T+1, W] */
  const float *ln_pre_w, *ln_pre_b, *ln_post_w, *ln_post_b;
  const float* proj_t;        /* [E, W] = proj^T (proj is [W,E] in the reference, clip/model.py:264) */
  const void* proj_t_bf16;
  const acx_block_weights* blocks; /* [layers] (host array) */
} acx_vit_weights;

typedef struct acx_vit_desc {
  int32_t resolution, patch, width, layers, heads, embed_dim;
  int32_t prec;               /* ACX_PREC_* */
  int32_t act;                /* the MLP's activation: 0 or ACX_ACT_QUICKGELU = QuickGELU (OpenAI's checkpoints), ACX_ACT_GELU = the exact GELU
                                 (open_clip configs without quick_gelu); anything else ACX_E_BADARG, ACX_ACT_GELU with prec = ACX_PREC_BF16
                                 ACX_E_UNSUPPORTED.  The struct GREW by this trailing member (as acx_ln_job did by y_scale): 0 is the
                                 activation every caller of the earlier header got, and such a caller must zero the descriptor's tail --
                                 memset(&desc, 0, sizeof desc) before filling it, as for every descriptor of this header */
} acx_vit_desc;

/* acx_vit_encode: VisionTransformer.forward (clip/model.py:266-290): frames [F,3,R,R] f32 ->
 * features [F, embed_dim] f32.  Workspace from acx_vit_workspace_bytes(desc, F).  Geometry: resolution % patch == 0, patch even,
 * (resolution / patch)^2 + 1 <= 1024 tokens (ACX_E_UNSUPPORTED above), width == 64 heads.  A patch that is not a multiple of 4
 * embeds on the f32 kernels in every precision. */
size_t acx_vit_workspace_bytes(const acx_vit_desc* d, int32_t frames);
int acx_vit_encode(acx_ctx* ctx, const acx_vit_desc* d, const acx_vit_weights* w,
                   const float* frames, int32_t nframes, float* features, void* workspace,
                   size_t workspace_bytes, void* stream);
/* acx_vit_encode with desc->prec = ACX_PREC_F32X6_LN16: ln_scales [2 layers] (HOST array) = the power-of-two plane scales of
 * ln_1 and ln_2 of every block (entries 2 l, 2 l + 1), each with s * max_i(|gamma_i| sqrt(width - 1) + |beta_i|) <= 2^14 and
 * 2^-20 <= s <= 2^20 -- the caller's proof from the weights; the driver checks only that they are such powers of two.
 * acx_vit_encode refuses that precision (it has no scales). */
int acx_vit_encode_ln16(acx_ctx* ctx, const acx_vit_desc* d, const acx_vit_weights* w, const float* ln_scales, const float* frames,
                        int32_t nframes, float* features, void* workspace, size_t workspace_bytes, void* stream);
/* acx_vit_encode with desc->prec = ACX_PREC_F32X6_R16: scales [4 layers] (HOST array), layer l at 4 l: the plane scales of ln_1, ln_2 (as
 * acx_vit_encode_ln16), of the attention output (s_att) and of the MLP hidden (s_hid) -- powers of two in [2^-20, 2^20] with s * bound <=
 * 2^14 for a bound the caller proves from the weights; the driver checks only that they are such powers of two. */
int acx_vit_encode_r16(acx_ctx* ctx, const acx_vit_desc* d, const acx_vit_weights* w, const float* scales, const float* frames,
                       int32_t nframes, float* features, void* workspace, size_t workspace_bytes, void* stream);
/* acx_vit_encode with desc->prec = ACX_PREC_F32X6_QKV16: scales [5 layers] (HOST array), layer l at 5 l: ln_1, ln_2, att, hid as
 * acx_vit_encode_r16 and s_qkv, the scale of the in-projection's output planes -- one power of two in [2^-20, 2^20] for the three thirds,
 * with s_qkv * bound <= 2^14 for a bound on every q, k and v element the caller proves from the weights. */
int acx_vit_encode_qkv16(acx_ctx* ctx, const acx_vit_desc* d, const acx_vit_weights* w, const float* scales, const float* frames,
                         int32_t nframes, float* features, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The CLIP ResNet image encoders (RN50, RN101, RN50x4, RN50x16, RN50x64: ModifiedResNet, clip/model.py:111-171), eval mode.
 * Activations are NHWC rows [frames * H * W][Cp] with Cp = the channel count rounded up to a multiple of 32; the padding
 * channels are zero (their weight rows / columns and biases are zero). */

/* acx_resnet_stem_im2col: the stem's 3x3 stride-2 pad-1 convolution (clip/model.py:123) as im2col: frames [F,3,R,R] f32 ->
 * cols [F * (R/2)^2][32], column k = c * 9 + ky * 3 + kx (conv1.weight.reshape(N, 27)'s order), columns 27..31 zero. */
int acx_resnet_stem_im2col(acx_ctx* ctx, const float* frames, float* cols, int32_t F, int32_t R, void* stream);
/* acx_avgpool2_nhwc: nn.AvgPool2d(2) (clip/model.py:24,37,132) on NHWC rows: in [F][H][W][C] -> out [F][H/2][W/2][C]; H, W even,
 * C % 4 == 0, 16-byte aligned. */
int acx_avgpool2_nhwc(acx_ctx* ctx, const float* in, float* out, int32_t F, int32_t H, int32_t W, int32_t C, void* stream);
/* acx_attnpool_tokens: AttentionPool2d's tokens (clip/model.py:82-84): x [F * HW][E] -> tokens [F * (HW + 1)][E], token 0 = the
 * mean over the HW tokens (f64 sum in token order), every token + positional_embedding[t]. */
int acx_attnpool_tokens(acx_ctx* ctx, const float* x, const float* pos, float* tokens, int32_t F, int32_t HW, int32_t E, void* stream);

/* One convolution with its eval BatchNorm folded in: w' = w * gamma / sqrt(running_var + eps), b' = beta - running_mean * gamma /
 * sqrt(running_var + eps) (folded in f64, stored f32).  1x1: w [Cout_p][Cin_p]; 3x3: w [Cout_p][tap = ky * 3 + kx][Cin_p]; the
 * stem's first conv: [Cout_p][32] over acx_resnet_stem_im2col's columns.  b [Cout_p]. */
typedef struct acx_resnet_conv {
  const float* w;
  const float* b;
  const void* w3;                           /* ACX_PREC_BF16X6: the three bf16 planes of w (acx_split_bf16x3: [3][Cout_p][K], plane stride
                                               Cout_p * K * 2 bytes) for every convolution the driver routes to the plane kernel -- every
                                               3x3, and every 1x1 with K >= 64 (not the stem's first); NULL / not read otherwise */
} acx_resnet_conv;
typedef struct acx_resnet_block {           /* Bottleneck (clip/model.py:10-68) */
  acx_resnet_conv conv1, conv2, conv3;
  acx_resnet_conv downsample;               /* w == NULL: no downsample (identity) */
} acx_resnet_block;
typedef struct acx_resnet_weights {
  acx_resnet_conv stem[3];                  /* conv1/bn1, conv2/bn2, conv3/bn3 */
  const acx_resnet_block* blocks;           /* layers[0] + ... + layers[3] blocks, layer after layer (host array) */
  const float* positional_embedding;        /* [HW + 1, E] (AttentionPool2d, E = 32 width) */
  const float *q_w, *q_b;                   /* q_proj [E, E], [E] */
  const float *kv_w, *kv_b;                 /* k_proj | v_proj stacked: [2E, E], [2E] */
  const float *c_w, *c_b;                   /* c_proj [output_dim, E], [output_dim] */
  const void* kv_w3;                        /* ACX_PREC_BF16X6: the three bf16 planes of kv_w ([3][2E][E]); not read otherwise */
} acx_resnet_weights;
typedef struct acx_resnet_desc {
  int32_t resolution, width;
  int32_t layers[4];
  int32_t heads, output_dim;                /* heads = width * 32 / 64 (clip/model.py:314) */
  int32_t prec;                             /* ACX_PREC_F32 or ACX_PREC_F32X6: both run the f32 MFMA kernels; ACX_PREC_BF16X6: the plane
                                               kernel for every product but the K = 32 stem product and the one-row-per-frame q / c_proj */
} acx_resnet_desc;
/* acx_resnet_encode: ModifiedResNet.forward in eval mode (clip/model.py:156-171): frames [F,3,R,R] f32 -> features
 * [F, output_dim] f32.  The frames run in internal batches whose largest activation stays below 2^31 bytes; workspace from
 * acx_resnet_workspace_bytes(desc, F) (0: the geometry is not supported).  R % 32 == 0, heads * 64 == 32 * width.
 * ACX_PREC_BF16X6: the products run as pairs = 6 products of bf16 planes -- which ones is a rule on (K, N, convolution or not) alone,
 * never on the frame count, so identical frames give bit-identical rows wherever they sit; a product whose only consumer is the next
 * product writes its planes directly, an f32 result that feeds a product is split by acx_split_bf16x3.  The workspace (16-byte
 * aligned) is larger by three plane buffers and a 256-byte zero page, which every call clears on its stream. */
size_t acx_resnet_workspace_bytes(const acx_resnet_desc* d, int32_t frames);
int acx_resnet_encode(acx_ctx* ctx, const acx_resnet_desc* d, const acx_resnet_weights* w, const float* frames, int32_t nframes,
                      float* features, void* workspace, size_t workspace_bytes, void* stream);

/* Training mode (BatchNorm2d.train(): Lightning's model.train() reaches the frozen encoder, anomaly_clip_module.py:68-69,160-166):
 * every BatchNorm normalises with the batch statistics over ALL frames, H and W of the call (biased variance), updates running_mean /
 * running_var with `momentum` (unbiased variance, torch.nn.functional.batch_norm) and increments num_batches_tracked. */
typedef struct acx_resnet_bn {              /* one nn.BatchNorm2d: device pointers to its parameters and buffers ([C]) */
  const float *weight, *bias;
  float *running_mean, *running_var;
  int64_t* num_batches_tracked;             /* may be NULL */
} acx_resnet_bn;
typedef struct acx_resnet_block_bn {
  acx_resnet_bn bn1, bn2, bn3, downsample;  /* downsample: unused without downsample weights */
} acx_resnet_block_bn;
typedef struct acx_resnet_train_bn {
  acx_resnet_bn stem[3];
  const acx_resnet_block_bn* blocks;        /* host array, as acx_resnet_weights.blocks */
  float eps, momentum;                      /* 1e-5, 0.1 (nn.BatchNorm2d's defaults, clip/model.py:18-28) */
} acx_resnet_train_bn;
/* acx_bn_apply_nhwc: y = x * alpha + shift (+ residual), then ReLU when relu != 0, over rows of Cp channels (in place allowed), with
 * alpha = gamma / sqrt(var_biased + eps), shift = beta - mean * alpha for the C real channels and 0 for the padding ones
 * (BatchNorm2d in training mode, clip/model.py:56-64,157-160).  scratch: 2 * Cp floats, 16-byte aligned. */
int acx_bn_apply_nhwc(acx_ctx* ctx, const float* x, const float* mean, const float* var_biased, const float* gamma, const float* beta,
                      const float* residual, float* y, int64_t rows, int32_t C, int32_t Cp, float eps, int32_t relu, float* scratch,
                      void* stream);
/* acx_resnet_encode_train: ModifiedResNet.forward with its BatchNorms in training mode (clip/model.py:156-171), layer by layer over
 * all F frames of the call (acx_bn_stats over each convolution's F * H * W rows).  w: the UNFOLDED convolution weights in the layouts
 * of acx_resnet_conv (the b fields are not read) and the attention pool; bn: every BatchNorm's parameters and buffers, which are
 * updated in place.  Workspace from acx_resnet_train_workspace_bytes(desc, F): every activation of all F frames.
 * A correctness path: it runs the f32 MFMA kernels for EVERY value of desc->prec, ACX_PREC_BF16X6 included (w3 / kv_w3 are not read). */
size_t acx_resnet_train_workspace_bytes(const acx_resnet_desc* d, int32_t frames);
int acx_resnet_encode_train(acx_ctx* ctx, const acx_resnet_desc* d, const acx_resnet_weights* w, const acx_resnet_train_bn* bn,
                            const float* frames, int32_t F, float* features, void* workspace, size_t workspace_bytes, void* stream);

/* acx_transformer_forward: Transformer.forward (clip/model.py:220-230) in place on x
 * [batch*L, W] f32 -- used by the text encoder (text_encoder.py:16-18). */
size_t acx_transformer_workspace_bytes(int32_t width, int32_t rows);
size_t acx_transformer_workspace_bytes_prec(int32_t width, int32_t rows, int32_t prec);   /* ACX_PREC_F32X6 needs room for the planes */
int acx_transformer_forward(acx_ctx* ctx, float* x, int32_t batch, int32_t L, int32_t width,
                            int32_t heads, int32_t layers, int32_t causal, int32_t prec,
                            const acx_block_weights* blocks, void* workspace,
                            size_t workspace_bytes, void* stream);
/* the same with the MLP's activation named: act = 0 / ACX_ACT_QUICKGELU (what acx_transformer_forward passes) or ACX_ACT_GELU; anything
 * else ACX_E_BADARG, ACX_ACT_GELU with prec = ACX_PREC_BF16 ACX_E_UNSUPPORTED. */
int acx_transformer_forward_act(acx_ctx* ctx, float* x, int32_t batch, int32_t L, int32_t width,
                                int32_t heads, int32_t layers, int32_t causal, int32_t prec, int32_t act,
                                const acx_block_weights* blocks, void* workspace,
                                size_t workspace_bytes, void* stream);

/* acx_transformer_plan: what acx_transformer_forward / acx_vit_encode launch for every layer of a geometry -- answered by the plan
 * step the drivers themselves execute (there is no second copy of the gates).  Host arithmetic, no device, nothing launched.
 * prune_last: the last layer is evaluated for the CLS rows only (acx_vit_encode; acx_transformer_forward: 0).  has_weight_planes: the
 * blocks carry their *_w_bf16 pointers (bf16 copies / weight planes; the f32 weights count as present).  workspace_is_prec_sized = 0:
 * the plan of a plane mode that is handed an f32-sized workspace (acx_transformer_forward then runs the f32 kernels).  Returns what
 * the driver returns before its first launch: ACX_OK, or the refusal's ACX_E_* with the same text in acx_last_error (the records are
 * then cleared).  ctx == NULL: the option values acx_create sets.  out[l] is layer l's record:
 *   ln1, ln2       ACX_TF_LN_*: ROWS own launch, f32 / bf16 rows; PLANES own launch, K-panel planes; RIDDEN handed to the previous
 *                  residual product as its acx_ln_job (ln_1: the previous layer's proj; ln_2: out_proj); CLS the CLS rows only
 *                  (pruned layer).  A pruned layer whose in_proj is ACX_TF_GEMM_X6 (the K | V product) adds the CLS rows' f32 launch
 *                  to a PLANES / RIDDEN ln1: Q reads them.  ln1_dtype / ln2_dtype: the output's ACX_F32 / ACX_BF16 / plane dtype
 *   in_proj .. proj  kernel ACX_TF_GEMM_ROWS (acx_gemm picks the kernel by its own routes) or ACX_TF_GEMM_X6 (plane kernel); c_dtype
 *                  of its output (ACX_F32 / ACX_BF16 rows, ACX_BF16X3P / ACX_F16X2P planes); scratch ACX_TF_BUF_*: the buffer that is
 *                  free at this product and serves its K split; ln_job 1: it carries the LayerNorm behind it (acx_gemm_ln).  A
 *                  pruned layer's in_proj is the K | V product of all rows (or none: ACX_TF_ATT_CLS_FOLD); Q, for the CLS rows, is
 *                  always a ROWS product
 *   att            ACX_TF_ATT_*: the attention entry point; att_products: acx_attention_p3n's product count (6 / 3 / 103, else 0);
 *                  att_out_dtype: ACX_F16X2P where ACX_TF_ATT_P3F goes out as acx_attention_p3f16, or (ACX_PREC_F32X6_QKV16: in_proj's
 *                  c_dtype is ACX_F16X2P, att ACX_TF_ATT_P3N, att_products 103) ACX_TF_ATT_P3N as acx_attention_p3h16; else 0.
 *                  ACX_TF_ATT_S16 (ACX_PREC_F16X3S): acx_attention_s16 on in_proj's ACX_F16X2P planes, writing out_proj's (scales 1)
 *   split_att, split_mlp  1: acx_split_bf16x3_panel of the attention output / the MLP hidden is launched
 *   pruned         1: the last layer, CLS rows only
 * The plan does not depend on the MLP's activation (acx_vit_desc.act, acx_transformer_forward_act): QuickGELU and the exact GELU take
 * the same kernels with another template value in c_fc's epilogue, so one query answers for both. */
enum { ACX_TF_LN_ROWS = 0, ACX_TF_LN_PLANES = 1, ACX_TF_LN_RIDDEN = 2, ACX_TF_LN_CLS = 3 };
enum { ACX_TF_GEMM_ROWS = 0, ACX_TF_GEMM_X6 = 1 };
enum { ACX_TF_BUF_NONE = 0, ACX_TF_BUF_SPLITK = 1, ACX_TF_BUF_H = 2, ACX_TF_BUF_QKV = 3, ACX_TF_BUF_MLP = 4 };
enum { ACX_TF_ATT_F32 = 0, ACX_TF_ATT_BF16 = 1, ACX_TF_ATT_X3_PANEL = 2, ACX_TF_ATT_P3N = 3, ACX_TF_ATT_P3F = 4, ACX_TF_ATT_CLS = 5,
       ACX_TF_ATT_CLS_FOLD = 6, ACX_TF_ATT_S16 = 7,
       /* width == 80 heads (non-causal only): acx_attention_hd (f32 rows), acx_attention_x3_hd with panel = 1, acx_attention_cls_hd */
       ACX_TF_ATT_HD_F32 = 8, ACX_TF_ATT_HD_X3_PANEL = 9, ACX_TF_ATT_HD_CLS = 10 };
typedef struct acx_tf_product_t {
  int32_t kernel, c_dtype, scratch, ln_job;
} acx_tf_product_t;
typedef struct acx_tf_layer_plan_t {
  int32_t ln1, ln1_dtype, ln2, ln2_dtype;
  acx_tf_product_t in_proj, out_proj, fc, proj;
  int32_t att, att_products, split_att, split_mlp;
  int32_t pruned;
  int32_t att_out_dtype;  /* the record's last word (the `reserved` word of earlier headers, 0 in every plan they describe):
                             ACX_F16X2P = the attention writes the two fp16 planes of s_att * o (ACX_PREC_F32X6_R16 with out-proj on fp16
                             planes: acx_attention_p3f16); 0 = the planes of the mode */
} acx_tf_layer_plan_t;
int acx_transformer_plan(const acx_ctx* ctx, int32_t batch, int32_t L, int32_t width, int32_t heads, int32_t layers,
                         int32_t causal, int32_t prec, int32_t prune_last, int32_t has_weight_planes,
                         int32_t workspace_is_prec_sized, acx_tf_layer_plan_t* out /* [layers] */);

/* ------------------------------------------------------------------------------------------
 * Head, forward (HBM-bound rows of SURVEY.md 8a). */

/* acx_text_directions: selector_model.py:44-59: drop row normal_id, subtract ncentroid,
 * L2-normalise.  text [C, D] -> dirs [C-1, D]. */
int acx_text_directions(acx_ctx* ctx, const float* text, const float* ncentroid, float* dirs,
                        int32_t C, int32_t D, int32_t normal_id, void* stream);
/* acx_selector_project: raw[r, c] = (x[r,:] - ncentroid) . dirs[c,:]  (selector_model.py:54,62).
 * x [rows, D] (D in {64,128,256,512,640,768,1024}), raw [rows, C1], C1 <= 64. */
int acx_selector_project(acx_ctx* ctx, const float* x, const float* ncentroid, const float* dirs,
                         float* raw, int64_t rows, int32_t D, int32_t C1, void* stream);
/* acx_bn_stats: deterministic per-column batch statistics of raw[rows, C1] (training BatchNorm1d,
 * selector_model.py:30,65: biased variance normalises, unbiased variance feeds running_var).  Two
 * stages (row slabs -> f64 partials in `workspace` -> fixed-order sum); C1 <= 64 -- or, with its own kernels, up to 65536 columns
 * (the ResNet encoders' training-mode BatchNorm2d, clip/model.py:18-28: one lane per column of a row slab, slabs added in order);
 * workspace >= acx_bn_workspace_bytes(rows, C1), 8-byte aligned. */
size_t acx_bn_workspace_bytes(int64_t rows, int32_t C1);
/* SyncBN (configs/trainer/ddp.yaml sync_batchnorm): combine the ranks' statistics.  gathered[ranks][2 * C1 + 1] holds, per rank,
 * mean[C1], biased_var[C1] * rows, rows; outputs the statistics over all rows (Chan et al.) and the total row count (device
 * scalar), one launch; C1 <= 64. */
int acx_bn_combine(acx_ctx* ctx, const float* gathered, int32_t ranks, int32_t C1, float* mean, float* var_biased,
                   float* var_unbiased, float* total_rows, void* stream);
int acx_bn_stats(acx_ctx* ctx, const float* raw, int64_t rows, int32_t C1, float* mean,
                 float* var_biased, float* var_unbiased, void* workspace, size_t workspace_bytes,
                 void* stream);
/* acx_selector_project_stats: acx_selector_project with the batch statistics of its output
 * accumulated in the projection's epilogue (raw is not read again): the training-mode pair
 * selector_model.py:62 + :65's statistics in two launches.  Same workspace rule as acx_bn_stats. */
int acx_selector_project_stats(acx_ctx* ctx, const float* x, const float* ncentroid,
                               const float* dirs, float* raw, int64_t rows, int32_t D, int32_t C1,
                               float* mean, float* var_biased, float* var_unbiased,
                               void* workspace, size_t workspace_bytes, void* stream);
/* acx_selector_bn: logits = (raw - mean) / sqrt(var + eps)  (BatchNorm1d(C-1, affine=False),
 * selector_model.py:30,65).  mean/var [C1] (running stats in eval, batch stats in train). */
int acx_selector_bn(acx_ctx* ctx, const float* raw, const float* mean, const float* var,
                    float* logits, int64_t ldl, int64_t rows, int32_t C1, float eps, void* stream);

/* acx_axial_attention: the softmax(q k^T e^-1/2) v core of axial_attention.SelfAttention along one
 * axis of the (tiles, gn, gl) token grid.  qkv [rows, 3*heads*e] = (q | k | v) per token, out
 * [rows, heads*e].  axis 0: attend along gn (tokens with equal (tile, l)); axis 1: along gl.
 * Domain: 1 <= axis length T <= 128 (either axis, any integer), e in {16, 32, 64}, heads >= 1; anything else is
 * ACX_E_UNSUPPORTED.  T in {16, 32} with e in {16, 32} runs one wave per (line, head) (q, k, v in a wave-private LDS
 * slice); every other shape runs the padded kernel (T rounded up to 16 inside the kernel, K / V of a group staged once
 * per workgroup, one query tile per wave; needs 16-byte aligned qkv / out).  Both on v_mfma_f32_16x16x4_f32. */
int acx_axial_attention(acx_ctx* ctx, const float* qkv, float* out, int32_t tiles, int32_t gn,
                        int32_t gl, int32_t heads, int32_t e, int32_t axis, void* stream);
/* acx_axial_attention_route: which kernel acx_axial_attention runs a shape on -- the rule the dispatcher itself switches on.
 * Arithmetic on the arguments: no device, nothing dereferenced, ctx may be NULL.  aligned: qkv and out are both 16-byte aligned.
 * PADDED_MFMA with aligned == 0 is the shape whose call answers ACX_E_BADARG (that kernel needs the alignment); UNSUPPORTED is
 * the call's ACX_E_UNSUPPORTED.  THREAD_PER_ROW (one thread per (line, head, query), K / V of the block's lines in LDS) is what a
 * misaligned T in {16, 32}, e in {16, 32} call with T * heads | 256 falls back to. */
enum { ACX_AXF_ROUTE_UNSUPPORTED = 0, ACX_AXF_ROUTE_PADDED_MFMA = 1, ACX_AXF_ROUTE_EXACT_MFMA = 2, ACX_AXF_ROUTE_THREAD_PER_ROW = 3 };
int acx_axial_attention_route(const acx_ctx* ctx, int32_t gn, int32_t gl, int32_t heads, int32_t e, int32_t axis, int32_t aligned);

/* acx_cls_head: score = sigmoid(LayerNorm((x1+x2)/2) . w + b) (ReversibleSequence mean +
 * classification_head.py:11-15); out_index maps row ((b s) n l) back to ((b n s l)) when seg > 0
 * (temporal_model.py:69-71). */
int acx_cls_head(acx_ctx* ctx, const float* x1, const float* x2, const float* ln_w,
                 const float* ln_b, const float* lin_w, const float* lin_b, float* scores,
                 int64_t rows, int32_t E, int32_t gn, int32_t gl, int32_t seg, void* stream);

/* acx_class_probs: softmax(similarity, dim=1) * score  (anomaly_clip_module.py:474-477). */
/* acx_cls_head with the scores scattered through a tile table (see acx_gemm_desc.tile_table): row (tile, n, l) is
 * written at base + n * stride + l -- the inverse tiling of temporal_model.py:67-73 for a batch of videos. */
int acx_cls_head_tiles(acx_ctx* ctx, const float* x1, const float* x2, const float* ln_w, const float* ln_b,
                       const float* lin_w, const float* lin_b, float* scores, int64_t rows, int32_t E, int32_t gn,
                       int32_t gl, const int32_t* tile_table, void* stream);
int acx_class_probs(acx_ctx* ctx, const float* sim, const float* scores, float* probs,
                    int64_t rows, int32_t C1, void* stream);

/* acx_prompt_embed: out[c,t,:] = cat(token_prefix, ctx, token_suffix)[c,t,:] + positional_embedding[t,:]
 * (coop.py:74-90 class_token_position "end" + text_encoder.py:15).  ctx is [C,n_ctx,W] or, when
 * shared_ctx != 0, [n_ctx,W] broadcast over classes (coop.py:76-77).  pos may be NULL (no add).  Lout (0 = Lc): only the
 * first Lout <= Lc positions of every class are written, out is [C, Lout, W] (the causal tower runs up to the last EOT). */
int acx_prompt_embed(acx_ctx* ctx, const float* prefix, const float* ctxv, const float* suffix,
                     const float* pos, float* out, int32_t C, int32_t n_ctx, int32_t Lc, int32_t W,
                     int32_t shared_ctx, int32_t Lout, void* stream);
/* acx_gather_rows: out[i,:] = x[idx[i],:]  (EOT-token gather, text_encoder.py:23). idx int64 on device. */
int acx_gather_rows(acx_ctx* ctx, const float* x, const int64_t* idx, float* out, int64_t n,
                    int32_t W, void* stream);

/* acx_add_bcast: out[r,:] = x[r,:] + p[:] over n rows of LW floats (text_encoder.py:15 when the
 * prompts were assembled without the positional embedding). */
int acx_add_bcast(acx_ctx* ctx, const float* x, const float* p, float* out, int64_t n, int64_t LW,
                  void* stream);
/* acx_concat_features: temporal-model input when concat_features is on: [logits | x - ncentroid | 0]
 * padded to Kp columns (anomaly_clip.py:143,201,223-233). */
int acx_concat_features(acx_ctx* ctx, const float* logits, const float* x, const float* ncentroid,
                        float* out, int64_t rows, int32_t C1, int32_t D, int32_t Kp, void* stream);

/* acx_preprocess_frames: decoded uint8 RGB frames [F,H,W,3] -> CLIP input [F,3,orows,ocols] f32:
 * Resize(shorter side, BICUBIC as PIL does it) + CenterCrop + /255 + Normalize (reference
 * src/utils/augmentations.py:21-34 and gtransforms.py GroupScale/GroupCenterCrop/GroupToTensor/GroupNormalize).
 * hbounds/hcoef: for each kept output column (xmin, n) and hksize 22-bit fixed-point coefficients (PIL's
 * precompute_coeffs + normalize_coeffs_8bpc, computed by anomalyclip_amd/preprocess.py); vbounds/vcoef likewise for
 * the kept output rows.  tmp: [F,H,ocols,3] uint8 scratch.  mean3/std3 are HOST pointers. */
int acx_preprocess_frames(acx_ctx* ctx, const unsigned char* frames, float* out, unsigned char* tmp,
                          const int32_t* hbounds, const int32_t* hcoef, int32_t hksize, const int32_t* vbounds,
                          const int32_t* vcoef, int32_t vksize, int32_t F, int32_t H, int32_t W, int32_t orows,
                          int32_t ocols, const float* mean3, const float* std3, void* stream);

/* acx_preprocess_crops: decoded uint8 RGB frames [F,H,W,3] -> [F,ncrops,3,crop,crop] f32, the crop index minor to the
 * frame index: GroupScale (shorter side -> scale_size, BICUBIC as PIL does it; reference gtransforms.py:89-102), then
 * the 1 / 5 / 10 crops of torchvision's CenterCrop / FiveCrop / TenCrop (gtransforms.py:449-477: tl, tr, bl, br, centre,
 * then the same five of the horizontally mirrored image), /255 and Normalize -- all crops of all frames in one launch
 * sequence.  hbounds/hcoef ([ow,2] / [ow,hksize]) and vbounds/vcoef ([oh,2] / [oh,vksize]) are the tables of the WHOLE
 * resized image (oh x ow); windows is a HOST array of ncrops x (top, left, flip): the crop is rows top..top+crop and
 * columns left..left+crop of the resized image, read right to left when flip != 0 (a window (t, l) of the mirrored
 * image is (t, ow - crop - l, 1) here).  tmp: [F,H,ow,3] uint8 scratch.  mean3/std3 are HOST pointers.
 * ACX_E_BADARG: ncrops not 1, 5 or 10; oh or ow below crop (scale_size < crop_size); a window outside the image.
 * F * ncrops beyond a launch's grid limits is split inside the call. */
int acx_preprocess_crops(acx_ctx* ctx, const unsigned char* frames, float* out, unsigned char* tmp,
                         const int32_t* hbounds, const int32_t* hcoef, int32_t hksize, const int32_t* vbounds,
                         const int32_t* vcoef, int32_t vksize, int32_t F, int32_t H, int32_t W, int32_t oh, int32_t ow,
                         int32_t crop, int32_t ncrops, const int32_t* windows, const float* mean3, const float* std3,
                         void* stream);

/* utility: x[rows, cols] (f32, leading dimension ld) -> three dense bf16 planes dst + p * plane_stride_bytes, [rows, cols] each:
 * hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) (each subtraction exact in f32): the operands of
 * acx_gemm_desc.pairs = 6.  cols % 4 == 0, 16-byte aligned src rows / 8-byte aligned planes. */
int acx_split_bf16x3(acx_ctx* ctx, const float* src, int64_t ld, void* dst, int64_t plane_stride_bytes, int64_t rows,
                     int64_t cols, void* stream);
/* the same into K-panel layout (ACX_BF16X3P: plane = [cols / 32][rows][32]; cols % 32 == 0) */
int acx_split_bf16x3_panel(acx_ctx* ctx, const float* src, int64_t ld, void* dst, int64_t plane_bytes, int64_t rows, int64_t cols, void* stream);
/* TWO fp16 planes hi | lo of scale * src (hi = fp16(.), lo = fp16(. - hi); scale a power of two: exact), row-major or K-panel
 * layout: operands of a pairs = 3 product with a_dtype = ACX_F16 (the ACX_PREC_F16X3 arithmetic); the product's acx_gemm_desc.out_scale
 * takes the scales out again */
int acx_split_f16x2(acx_ctx* ctx, const float* src, int64_t ld, void* dst, int64_t plane_stride_bytes, int64_t rows, int64_t cols,
                    float scale, int32_t panel, void* stream);
/* n dense f32 tensors (numel[i] elements each, multiples of 8, 16-byte aligned) -> three row-major bf16 planes each
 * (dst[i]: 3 * numel[i] bf16, plane stride numel[i]) in ONE launch: a training step re-splits every convolution weight of the
 * temporal model after the optimizer has stepped. */
int acx_split_bf16x3_multi(acx_ctx* ctx, int32_t n, const float* const* src, void* const* dst, const int64_t* numel, void* stream);
/* utility: f32 -> bf16 (round-to-nearest-even) copy, used to prepare bf16 weight copies. */
int acx_cast_bf16(acx_ctx* ctx, const float* src, void* dst, int64_t n, void* stream);
/* utility: column sums of x[rows, D] accumulated into acc[D] (ncentroid, anomaly_clip_module.py:145-171). */
int acx_colsum(acx_ctx* ctx, const float* x, float* acc, int64_t rows, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training side (SURVEY.md 8a rows a4, a9, a12 and the backward of a2/a3/a6/a7/a8).  Row reductions
 * are two-stage and fixed-order: kernels emit per-block partials, acx_reduce_rows sums them. */

/* acx_gemm_tn: C[N1,N2] = sum_m A[m,n1] * bmap(B)[m,n2] (exact-f32 MFMA) -- weight gradients
 * dW = dY^T X of every nn.Linear / Conv2d of the temporal model and text_projection.  conv != 0: B column
 * k = tap*cin + ci reads token row shift_tap(m) on the (gn,gl) grid (zero outside) = dW of the 3x3 convs in
 * the [Cout][tap][Cin] layout.  b_sub [N2]: subtracted from every valid B row (selector direction gradient). */
size_t acx_gemm_tn_workspace_bytes(int32_t M, int32_t N1, int32_t N2);
int acx_gemm_tn(acx_ctx* ctx, const float* A, int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc,
                int32_t M, int32_t N1, int32_t N2, const float* b_sub, int32_t conv, int32_t gn, int32_t gl,
                int32_t cin, void* workspace, size_t workspace_bytes, void* stream);
/* Several small weight gradients C_k[N1_k, N2_k] = A_k^T (B_k - b_sub_k) (identity row map, dense C_k) in ONE launch (+ one
 * reduce launch): each problem runs the blocks of its own acx_gemm_tn launch, so results are bit-identical to separate calls.
 * The temporal model's to_out / to_q|to_kv / projection gradients of a step (0.5-1.6 GFLOP each) are issued this way. */
typedef struct acx_tn_problem {
  const void* A; const void* B; void* C; const void* b_sub;
  int32_t M, N1, N2, lda, ldb, reserved;
} acx_tn_problem;
size_t acx_gemm_tn_group_workspace_bytes(int32_t nprob, const acx_tn_problem* probs);
int acx_gemm_tn_group(acx_ctx* ctx, int32_t nprob, const acx_tn_problem* probs, void* workspace, size_t workspace_bytes,
                      void* stream);
/* the same with a caller-owned zero page (>= 1024 bytes of zeros, 16-byte aligned, never written; may be NULL): the
 * 256 x 256 kernel then pads from it instead of clearing the tail of `workspace` with an extra launch per call */
int acx_gemm_tn_zp(acx_ctx* ctx, const float* A, int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc,
                int32_t M, int32_t N1, int32_t N2, const float* b_sub, int32_t conv, int32_t gn, int32_t gl,
                int32_t cin, void* workspace, size_t workspace_bytes, const void* zero_page, void* stream);
/* acx_gemm_tn_zp WITHOUT its reduce launch: *splits_out (host) = number of K-split partial images left in `workspace`
 * ([splits][N1][N2] f32; their sum in image order is what acx_gemm_tn_zp writes to C); 1: C holds the result.  For consumers that
 * add the images themselves (acx_text_directions_bwd_parts). */
int acx_gemm_tn_parts(acx_ctx* ctx, const float* A, int32_t lda, const float* B, int32_t ldb, float* C, int32_t ldc,
                      int32_t M, int32_t N1, int32_t N2, const float* b_sub, int32_t conv, int32_t gn, int32_t gl,
                      int32_t cin, void* workspace, size_t workspace_bytes, const void* zero_page, int32_t* splits_out, void* stream);
/* The same weight gradient as an f32-ACCURATE product on the bf16 matrix cores: A (dY, [M, lda]) and B (the layer input,
 * [M, ldb]) as three bf16 planes each (acx_split_bf16x3: plane p at base + p * plane_stride bytes), the six leading cross
 * products with f32 accumulation -- the TN instantiation of the plane-reuse kernel (acx_gemm_desc.pairs = 6).  N1, N2 multiples
 * of 256; conv: cin % 256 == 0, N2 == 9 cin, power-of-two grid, M % (gn gl) == 0.  zero_page: >= 256 bytes of zeros, 16-byte
 * aligned (rows behind M and taps outside the grid are DMA'd from it).  workspace: acx_gemm_tn_x6_workspace_bytes (the rows are
 * split across workgroups; fixed summation order for a given shape).  Replaces the weight-gradient products of
 * temporal_model.py:32-39's convolutions under autograd (loss.backward() in src/models/anomaly_clip_module.py:173-293). */
size_t acx_gemm_tn_x6_workspace_bytes(int32_t M, int32_t N1, int32_t N2);
int acx_gemm_tn_x6(acx_ctx* ctx, const void* A3, int64_t a_plane_stride, int32_t lda, const void* B3, int64_t b_plane_stride,
                   int32_t ldb, float* C, int32_t ldc, int32_t M, int32_t N1, int32_t N2, int32_t conv, int32_t gn, int32_t gl,
                   int32_t cin, void* workspace, size_t workspace_bytes, const void* zero_page, void* stream);
/* acx_gemm_tn_route / acx_gemm_tn_x6_route: which kernel acx_gemm_tn / _zp / _parts (acx_gemm_tn_x6) runs a problem on and how it
 * splits the rows -- answered by the entry points' own walk, which stops where the first launch would be (there is no second copy
 * of the gates).  Host arithmetic, no device, nothing launched.  The operands stand in as aligned dummy addresses: has_b_sub /
 * has_workspace / has_zero_page say which optional ones the caller brings, want_parts != 0 asks for acx_gemm_tn_parts.  The
 * pointer (and plane stride) alignment refusals are therefore the real calls' alone.  Returns what the call would return before its
 * first launch: ACX_OK, or the refusal's ACX_E_* with the same text in acx_last_error (*out is then kernel = ACX_TN_ROUTE_NONE,
 * splits = 1).  ctx == NULL: 256 CUs and the option values acx_create sets.
 *   kernel            ACX_TN_ROUTE_W8 (gemm_tn_w8_kernel, 128 x 128 tiles), _P256 (gemm_tn_p256_kernel, 256 x 256), _X6_* (the
 *                     plane kernel's three tile geometries, N1 x N2).  The 4-wave gemm_tn_kernel behind a tools build's debug
 *                     switch is not reported: such a build answers W8
 *   splits            row ranges across workgroups (1: none; C is then written by the kernel itself)
 *   rows_per_split    rows of a range (the last takes what is left; under P256 a trailing range can be empty and stores zeros)
 *   tiles             output tiles in the kernel's tile size
 *   reduce            0 no split; 1 a reduce launch sums the images in image order; 2 they stay in the workspace for the caller
 *   clears_zero_page  1: P256 without a caller's zero page clears 1 KB behind the images in the workspace with a launch of its own */
enum { ACX_TN_ROUTE_NONE = 0, ACX_TN_ROUTE_W8 = 1, ACX_TN_ROUTE_P256 = 2, ACX_TN_ROUTE_X6_256x256 = 3, ACX_TN_ROUTE_X6_256x128 = 4,
       ACX_TN_ROUTE_X6_128x256 = 5 };
typedef struct acx_gemm_tn_route_t {
  int32_t kernel, splits, rows_per_split, tiles, reduce, clears_zero_page;
} acx_gemm_tn_route_t;
int acx_gemm_tn_route(const acx_ctx* ctx, int32_t M, int32_t N1, int32_t N2, int32_t lda, int32_t ldb, int32_t ldc, int32_t has_b_sub,
                      int32_t conv, int32_t gn, int32_t gl, int32_t cin, int32_t has_workspace, size_t workspace_bytes,
                      int32_t has_zero_page, int32_t want_parts, acx_gemm_tn_route_t* out);
int acx_gemm_tn_x6_route(const acx_ctx* ctx, int32_t M, int32_t N1, int32_t N2, int32_t lda, int32_t ldb, int32_t ldc, int32_t conv,
                         int32_t gn, int32_t gl, int32_t cin, int32_t has_workspace, size_t workspace_bytes, int32_t has_zero_page,
                         acx_gemm_tn_route_t* out);
int acx_reduce_rows(acx_ctx* ctx, const float* part, float* out, int32_t nparts, int32_t width, void* stream);
/* LayerNorm / ChanLayerNorm backward.  dx (may be NULL) = [add +] dx_scale * dL/dx (add [rows, D] may be NULL: the
 * residual branch of a pre-norm block, clip/model.py:214-216, folded into the same pass); part (may be NULL)
 * receives acx_row_parts(rows) rows of [dw(D) | db(D)] partials. */
int acx_layernorm_bwd(acx_ctx* ctx, const float* x, const float* w, const float* dy, float* dx, float* part,
                      int64_t rows, int32_t D, float eps, int32_t mode, float dx_scale, const float* add, void* stream);
/* backward of acx_cls_head (seg == 0): dx = dL/dx1 = dL/dx2; part: acx_row_parts(rows) rows of
 * [d ln_w (E) | d ln_b (E) | d lin_w (E) | d lin_b (1) | pad 3]. */
int acx_cls_head_bwd(acx_ctx* ctx, const float* x1, const float* x2, const float* ln_w, const float* ln_b,
                     const float* lin_w, const float* scores, const float* dscores, float* dx, float* part,
                     int64_t rows, int32_t E, void* stream);
/* elementwise: mode 0 LeakyReLU' from saved output, 1 QuickGELU' from saved pre-activation (out = d * f'),
 * 2 QuickGELU forward (d ignored), 3 the exact GELU's derivative Phi(x) + x phi(x) from the saved pre-activation (out = d * f'),
 * 4 the exact GELU forward (d ignored).  n % 4 == 0; any other mode ACX_E_BADARG. */
int acx_act(acx_ctx* ctx, const float* saved, const float* d, float* out, int64_t n, int32_t mode, void* stream);
/* LeakyReLU(0.01) backward for the bf16 x 6 path of the temporal model's feed-forward (temporal_model.py:32-39 under autograd):
 * u_hi = the hi bf16 plane of the saved activation (its sign is the activation's), d [n] the upstream gradient; out [n] f32 and
 * planes (three bf16 planes, plane p at (uint16_t*)planes + p * plane_elems) both receive d * (u > 0 ? 1 : 0.01). */
int acx_leaky_grad_planes(acx_ctx* ctx, const void* u_hi, const float* d, float* out, void* planes, int64_t plane_elems, int64_t n,
                          void* stream);
int acx_add(acx_ctx* ctx, const float* a, const float* b, float* out, int64_t n, void* stream);
int acx_transpose(acx_ctx* ctx, const float* in, float* out, int32_t R, int32_t Cn, void* stream);
/* conv weight [Cout,Cin,3,3] -> [Cin][tap'][Cout] with flipped taps: the W operand of the dX implicit GEMM */
int acx_conv_weight_dx(acx_ctx* ctx, const float* w, float* out, int32_t Cout, int32_t Cin, void* stream);
/* backward of acx_axial_attention (axis 0/1 on the (tiles,gn,gl) grid) and of acx_attention (tiles=batch,
 * gn=1, gl=L, axis=1, e=64, causal as in the forward): dqkv [rows, 3*heads*e].
 * Domain: 1 <= sequence length T <= 256, e in {16, 32, 64} (ACX_E_UNSUPPORTED otherwise).  Non-causal T <= 64 with
 * e in {16, 32} runs on the f32 MFMA, one wave per (line, head): T in {16, 32} unpadded, every other T padded to a
 * multiple of 16 inside the kernel.  The text-tower shapes (gn = 1, e = 64) have their own kernels; everything else
 * (T > 64, or e = 64 on a grid, or causal) runs the general thread-per-(group, row) kernel. */
int acx_seq_attention_bwd(acx_ctx* ctx, const float* qkv, const float* dout, float* dqkv, int32_t tiles,
                          int32_t gn, int32_t gl, int32_t heads, int32_t e, int32_t axis, int32_t causal,
                          float* stats_ws /* [rows*heads*3] floats or NULL */, void* stream);
/* acx_seq_attention_bwd_route: which kernel acx_seq_attention_bwd runs a shape on -- the rule the dispatcher itself switches
 * on.  Arithmetic on the arguments: no device, nothing dereferenced, ctx may be NULL.  has_stats: stats_ws is not NULL.
 *   TEXT_MFMA          gn = 1, axis 1, e = 64, T <= 80: one workgroup per (sequence, head) on the f32 MFMA
 *   TEXT_BLOCK         the same shape, T 81..128: operands staged once in LDS, wave per row on the VALU
 *   TEXT_ROWS          the same shape, T 129..256, with stats_ws: wave per row from L2, two launches
 *   AXIAL_MFMA         non-causal T in {16, 32}, e in {16, 32}: one wave per (line, head) on the f32 MFMA
 *   AXIAL_MFMA_PADDED  non-causal every other T <= 64, e in {16, 32}: the same kernel on T rounded up to 16
 *   GENERIC            everything else in the domain: one thread per (group, row)
 *   UNSUPPORTED        the call's ACX_E_UNSUPPORTED */
enum { ACX_SAB_ROUTE_UNSUPPORTED = 0, ACX_SAB_ROUTE_TEXT_MFMA = 1, ACX_SAB_ROUTE_TEXT_BLOCK = 2, ACX_SAB_ROUTE_TEXT_ROWS = 3,
       ACX_SAB_ROUTE_AXIAL_MFMA = 4, ACX_SAB_ROUTE_AXIAL_MFMA_PADDED = 5, ACX_SAB_ROUTE_GENERIC = 6 };
int acx_seq_attention_bwd_route(const acx_ctx* ctx, int32_t tiles, int32_t gn, int32_t gl, int32_t heads, int32_t e, int32_t axis,
                                int32_t causal, int32_t has_stats);
/* gradients of the axial positional embeddings (pos0 [gn,E], pos1 [gl,E]) from dx [(tile,n,l), E]; `part` is a
 * scratch buffer of tiles*gn*E + tiles*ceil(gn/4)*gl*E floats (two-stage fixed-order reduction). */
int acx_pos_grad(acx_ctx* ctx, const float* dx, float* d0, float* d1, float* part, int32_t tiles, int32_t gn,
                 int32_t gl, int32_t E, void* stream);
/* BatchNorm1d(affine=False) training backward in two steps (so data-parallel SyncBN can all-reduce the
 * sums in between): stats -> sums[2*C1] = (sum dl, sum dl*xhat) per column over this rank's rows; apply ->
 * draw[r*ldo + c] with total_rows = rows of ALL ranks. */
int acx_bn_bwd_stats(acx_ctx* ctx, const float* logits, const float* dlogits, float* sums, int64_t rows,
                     int32_t C1, void* workspace /* acx_bn_workspace_bytes */, size_t workspace_bytes, void* stream);
int acx_bn_bwd_apply(acx_ctx* ctx, const float* logits, const float* dlogits, const float* var_biased,
                     const float* sums, float* draw, int32_t ldo, int64_t rows, int64_t total_rows, int32_t C1,
                     float eps, const float* total_rows_dev /* device scalar overriding total_rows, or NULL: SyncBN keeps
                     the all-gathered row count on the device instead of synchronising the host for it */, void* stream);
/* (draw is [rows, ldo], ldo >= C1: the kernel writes the pad columns C1 .. ldo - 1 as zeros itself) */
/* y = a*x + b*y (BatchNorm running-statistics update, selector_model.py:30 momentum 0.1) */
int acx_axpby(acx_ctx* ctx, const float* x, float* y, int32_t n, float a, float b, void* stream);
/* deterministic column sums: part[blk][D] partials over rows_per_block rows each (then acx_reduce_rows) */
int acx_colsum_partials(acx_ctx* ctx, const float* x, int32_t ld, float* part, int64_t rows, int32_t D,
                        int32_t rows_per_block, void* stream);
int acx_text_directions_bwd(acx_ctx* ctx, const float* text, const float* ncentroid, const float* ddirs,
                            float* dtext, int32_t C, int32_t D, int32_t normal_id, void* stream);
/* acx_select_idx: selector_model.py:119-158 / 227-266.  logits [B, N*Lg, C1]; masks [B,N] (1 keep, 0 drop);
 * idx_top [B,ktop] / idx_bot [B,kbot] int64 (first B/2 rows abnormal videos, rest normal).  Ties are broken
 * towards the LOWER segment index (torch.topk leaves tie order unspecified). */
int acx_select_idx(acx_ctx* ctx, const float* logits, const int64_t* labels, const float* mask_top,
                   const float* mask_bot, int64_t* idx_top, int64_t* idx_bot, int32_t B, int32_t N, int32_t Lg,
                   int32_t C1, int32_t normal_id, int32_t ktop, int32_t kbot, void* stream);
int acx_gather_segments(acx_ctx* ctx, const float* logits, const int64_t* idx, float* out, int32_t B, int32_t N,
                        int32_t Lg, int32_t C1, int32_t K, void* stream);
int acx_scatter_segments(acx_ctx* ctx, const float* dout, const int64_t* idx, float* dlogits, int32_t B, int32_t N,
                         int32_t Lg, int32_t C1, int32_t K, void* stream);
/* acx_mil_loss_one: ComputeLoss.__call__ (loss.py:51-195) forward AND backward in ONE launch.  losses[8] = (cost,
 * ldir_abn, ldir_nor, ltopk_abn, lbottomk_abn, ltopk_nor, lsmooth, lsparse); dsim / dsim_topk / dscores are the
 * gradients of gout*cost (gout: device scalar or NULL = 1).  lambdas[7] = (dir_abn, dir_nor, topk_abn, bottomk_abn, topk_nor,
 * smooth, sparse).  workspace: ceil(B*N*Lg/256)*8 + ceil(B*K*Lg/256) floats.  `counter` = one uint32, zero before the first call
 * and left zero by every call (caller-owned; NULL is ACX_E_BADARG).  The block partials are added in a fixed order, in f64. */
int acx_mil_loss_one(acx_ctx* ctx, const float* sim, const float* sim_topk, const int64_t* labels, const float* scores,
                 const int64_t* idx_topk_abn, const int64_t* idx_topk_nor, const int64_t* idx_bottomk_abn,
                 float* dsim, float* dsim_topk, float* dscores, float* losses, float* workspace,
                 size_t workspace_floats, int32_t B, int32_t N, int32_t Lg, int32_t C1, int32_t K, int32_t normal_id,
                 const float* lambdas, const float* gout, uint32_t* counter, void* stream);
/* The loss, its gradients AND the selector BatchNorm's backward statistics as ONE launch (the whole-step graph's middle):
 * acx_mil_loss_one + acx_axpby(meter += losses) + acx_scatter_segments(dsim += dsim_topk at the top-k segments) + acx_bn_bwd_stats in
 * one kernel with the SAME arithmetic in the same order (bit-identical outputs): dlogits [B N Lg, C1] = the gradient wrt the logits
 * incl. the gathered top-k rows' share, bn_sums [2 C1] = (sum dl, sum dl * xhat), meter [8] (may be NULL) += losses.  Needs
 * B N Lg % 256 == 0 and <= 131072 rows (a block of 256 frame rows is a slab of acx_bn_bwd_stats); ACX_E_UNSUPPORTED otherwise.
 * workspace: ceil(B N Lg / 256) * 8 + ceil(B K Lg / 256) floats; bn_workspace: acx_bn_workspace_bytes; counter as acx_mil_loss_one. */
int acx_mil_loss_bn(acx_ctx* ctx, const float* sim, const float* sim_topk, const int64_t* labels, const float* scores,
                    const int64_t* idx_topk_abn, const int64_t* idx_topk_nor, const int64_t* idx_bottomk_abn, float* dlogits,
                    float* dscores, float* losses, float* meter, float* bn_sums, float* workspace, size_t workspace_floats,
                    void* bn_workspace, size_t bn_workspace_bytes, int32_t B, int32_t N, int32_t Lg, int32_t C1, int32_t K,
                    int32_t normal_id, const float* lambdas, const float* gout, uint32_t* counter, void* stream);
/* acx_mil_loss_bn_fits: the code acx_mil_loss_bn's shape checks give a shape -- ACX_OK, ACX_E_BADARG (B odd or < 2, C1 outside
 * 1..64) or ACX_E_UNSUPPORTED (B N Lg no multiple of 256, or more than 131072 rows); the entry point itself calls it.  Arithmetic
 * on the arguments: no device, nothing dereferenced, ctx may be NULL, no error text. */
int acx_mil_loss_bn_fits(const acx_ctx* ctx, int32_t B, int32_t N, int32_t Lg, int32_t C1, int32_t K);
/* The selector's forward tail as ONE launch, one workgroup per video (selector_model.py:60-99,119-225): [SyncBN combine of
 * `gathered` [ranks, 2 C1 + 1] -> stat_out [3 C1 + 1] = mean | biased var | unbiased var | total rows; gathered == NULL: the local
 * statistics mean / var_biased / var_unbiased] -> logits = BatchNorm(raw) [rows, ldl] -> [running statistics, NULL: none] ->
 * top-k / bottom-k segment picks (acx_select_idx) -> logits_topk [B ktop Lg, C1] (acx_gather_segments of idx_top).  The same
 * expressions in the same order as acx_bn_combine / acx_selector_bn / acx_bn_running_update / acx_select_idx /
 * acx_gather_segments: bit-identical results, four or five launches less. */
int acx_selector_tail(acx_ctx* ctx, const float* raw, const float* gathered, int32_t ranks, const float* mean,
                      const float* var_biased, const float* var_unbiased, float* stat_out, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, float momentum, float one_minus, float* logits, int64_t ldl, const int64_t* labels,
                      const float* mask_top, const float* mask_bot, int64_t* idx_top, int64_t* idx_bot, float* logits_topk, int32_t B,
                      int32_t N, int32_t Lg, int32_t C1, int32_t normal_id, int32_t ktop, int32_t kbot, float eps, void* stream);
/* acx_selector_tail_fits: the code acx_selector_tail's shape checks give a shape -- ACX_OK, ACX_E_BADARG (B odd or < 2, a k
 * outside 0..N, C1 outside 1..64) or ACX_E_UNSUPPORTED (a video's (N Lg C1 + N C1 + 2 N + 2 C1 + ktop + kbot) * 4 bytes exceed the
 * 160 KB of LDS); the entry point itself calls it (and checks ldl).  Arithmetic on the arguments, as acx_mil_loss_bn_fits. */
int acx_selector_tail_fits(const acx_ctx* ctx, int32_t B, int32_t N, int32_t Lg, int32_t C1, int32_t ktop, int32_t kbot);
/* acx_text_directions_bwd with d_dirs given as the K-split partial images of the TN product that forms it (acx_gemm_tn_parts:
 * image s at ddirs_parts + s * part_stride floats, rows = direction index, row stride D), summed here in image order. */
int acx_text_directions_bwd_parts(acx_ctx* ctx, const float* text, const float* ncentroid, const float* ddirs_parts, int32_t nparts,
                                  int64_t part_stride, float* dtext, int32_t C, int32_t D, int32_t normal_id, void* stream);
/* acx_adamw: one torch.optim.AdamW step (decoupled weight decay, bias correction; step counts from 1). */
int acx_adamw(acx_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
              float beta2, float eps, float weight_decay, int32_t step, void* stream);
/* acx_multi_axpy: y_i += a * x_i for nseg tensors in ONE launch (HOST arrays of device pointers / sizes): the
 * gradient accumulation autograd performs with one elementwise launch per parameter (AccumulateGrad). */
int acx_multi_axpy(acx_ctx* ctx, int32_t nseg, void* const* y, const void* const* x, const int64_t* n, float a,
                   void* stream);
/* acx_adamw_multi: the same update for nseg parameter tensors in ONE launch (per-tensor lr / weight decay: the
 * reference's four param groups, anomaly_clip_module.py:693-746; common betas / eps / step).  The pointer and size
 * arrays are HOST arrays of length nseg; entries with n[i] <= 0 are skipped.  Hyper-parameters are doubles: the scalar
 * terms (1 - beta, bias corrections, lr / bc1, 1 - lr * wd) are formed in f64 and rounded once, like torch does. */
int acx_adamw_multi(acx_ctx* ctx, int32_t nseg, void* const* p, const void* const* g, void* const* m, void* const* v,
                    const int64_t* n, const double* lr, const double* weight_decay, double beta1, double beta2, double eps,
                    int32_t step, void* stream);
/* ---- whole-step training graph support (anomalyclip_amd/components/step_graph.py; reference: what Lightning's automatic
 * optimisation + DDP + torch.optim.AdamW do around training_step, anomaly_clip_module.py:203-293,693-746,
 * configs/trainer/ddp.yaml:1-9).  Nothing here allocates; every call is capturable in a HIP graph. */
/* number of per-block partial rows acx_layernorm_bwd (part != NULL) and acx_cls_head_bwd write for `rows` rows */
int64_t acx_row_parts(int64_t rows);
/* strided 2-D copies / transposes of f32 blocks, ALL in one launch: dst[r * dst_ld + c] = src[r * src_ld + c], or with
 * `transpose` dst[c * dst_ld + r] = src[r * src_ld + c]; rows / cols are the SOURCE block's extent, leading dimensions
 * in elements.  Builds every derived weight layout of the temporal model (temporal_model.py:18-40 parameters -> kernel
 * operands: q|kv concatenation, W^T for the dX GEMMs, flipped-tap conv weights, padded projection, positional tables). */
typedef struct acx_prep_seg {
  const void* src;
  void* dst;
  int32_t rows, cols, src_ld, dst_ld;
  int32_t transpose, reserved;
} acx_prep_seg;
int acx_prep_multi(acx_ctx* ctx, int32_t nseg, const acx_prep_seg* segs, void* stream);
/* y_i = x_i for nseg contiguous f32 tensors, one launch */
int acx_multi_copy(acx_ctx* ctx, int32_t nseg, void* const* y, const void* const* x, const int64_t* n, void* stream);
/* HOST helper: the f32 scalars of one AdamW step, out[0] = sqrt(1 - beta2^step), out[1 + 2 i] = 1 - lr_i wd_i,
 * out[2 + 2 i] = lr_i / (1 - beta1^step) -- formed in f64 and rounded once, exactly as acx_adamw_multi forms them. */
int acx_adamw_hyper(int32_t nseg, const double* lr, const double* weight_decay, double beta1, double beta2, int32_t step,
                    float* out);
/* acx_adamw_multi with those scalars read from DEVICE memory (`hyper_dev`: 1 + 2 nseg floats, refreshed by the caller
 * before each step), so a captured launch follows the LR schedule and the step count; every gradient is multiplied by
 * `grad_scale` as it is read (1 / world size after a summing all-reduce, 1.0f otherwise).  torch.optim.AdamW semantics
 * (anomaly_clip_module.py:693-746; wd 0.2 in the reference model configs). */
int acx_adamw_multi_dev(acx_ctx* ctx, int32_t nseg, void* const* p, const void* const* g, void* const* m, void* const* v,
                        const int64_t* n, const float* hyper_dev, float grad_scale, double beta1, double beta2, double eps,
                        void* stream);
/* ---- gradient clipping (configs/trainer/default.yaml:1 instantiates pytorch_lightning.Trainer, whose gradient_clip_val /
 * gradient_clip_algorithm run torch.nn.utils.clip_grad_norm_ / clip_grad_value_ between backward and optimizer.step()).
 * acx_grad_norm: global L2 norm of nseg f32 gradient tensors (host arrays of device pointers and element counts; 4-byte
 * alignment suffices; any nseg >= 1, more tensors than one launch's table are several launches).  Every gradient is
 * multiplied by grad_scale in f32 as it is read (1 / world size after a summing all-reduce, 1.0f otherwise); squares and
 * sums are formed in fp64 in a fixed order (tensor order, then chunk order, then a fixed in-block tree; no floating-point
 * atomics), so the result is bit-identical from call to call and the f32-rounded norm is within one ulp of the exact one.
 * Writes the device record out[0] = norm, out[1] = clip coefficient, out[2] += norm (a running sum the caller zeroes).
 * The coefficient is torch's, in f32: c = max_norm / (norm + 1e-6f), then c > 1 ? 1 : c (a NaN norm gives a NaN
 * coefficient, a zero gradient 1).  workspace: acx_grad_norm_workspace_bytes(nseg, total elements) bytes, 16-byte aligned,
 * caller-owned, ZERO before the first call and left reusable by every call (its arrival counter returns to zero).  No
 * allocation, no host read, capturable. */
size_t acx_grad_norm_workspace_bytes(int32_t nseg, int64_t n);
int acx_grad_norm(acx_ctx* ctx, int32_t nseg, const void* const* g, const int64_t* n, float grad_scale, float max_norm,
                  float* out, void* workspace, size_t workspace_bytes, void* stream);
/* acx_adamw_multi_dev on clipped gradients.  clip_dev (may be NULL): the record acx_grad_norm wrote, every gradient becomes
 * (g * grad_scale) * clip_dev[1].  clip_value (<= 0: off): g * grad_scale is clamped to [-clip_value, clip_value], a NaN
 * stays a NaN (clip_grad_value_).  At most one of the two.  The gradient tensors `g` are WRITTEN despite their const type (the
 * signature mirrors acx_adamw_multi_dev's): they are left holding the clipped mean.  With both off this IS acx_adamw_multi_dev. */
int acx_adamw_multi_dev_clip(acx_ctx* ctx, int32_t nseg, void* const* p, const void* const* g, void* const* m, void* const* v,
                             const int64_t* n, const float* hyper_dev, float grad_scale, double beta1, double beta2, double eps,
                             const float* clip_dev, float clip_value, void* stream);
/* the same clipping applied in place to the gradient tensors alone (an optimizer whose step is not libacx's) */
int acx_clip_grads(acx_ctx* ctx, int32_t nseg, void* const* g, const int64_t* n, float grad_scale, const float* clip_dev,
                   float clip_value, void* stream);
/* SyncBatchNorm payload of a rank (configs/trainer/ddp.yaml:9): out[2 C1 + 1] = [mean | biased var * rows | rows] */
int acx_bn_pack(acx_ctx* ctx, const float* mean, const float* var_biased, int64_t rows, int32_t C1, float* out,
                void* stream);
/* nn.BatchNorm1d running statistics (selector_model.py:30,65; and BatchNorm2d, clip/model.py:18-28): r = one_minus * r + momentum *
 * batch; counter += 1.  C1 <= 65536 */
int acx_bn_running_update(acx_ctx* ctx, const float* mean, const float* var_unbiased, float* running_mean,
                          float* running_var, int64_t* num_batches_tracked, int32_t C1, float momentum, float one_minus,
                          void* stream);
int acx_fill_f32(acx_ctx* ctx, float* p, int64_t n, float value, void* stream);
/* out[D] = column sums of x[rows, ld] in ONE launch, fixed summation order (bias gradients: the reference's autograd sums
 * dY over rows for every nn.Linear / nn.Conv2d bias).  part: scratch of acx_colsum_fused_part_bytes(rows, D) bytes;
 * counters: >= ceil(D / 64) uint32, ZERO before the first call and left zero by every call (caller-owned, reusable).
 * out = sums + beta * out (beta = 0: overwrite; 1: the ncentroid accumulation of anomaly_clip_module.py:145-171). */
size_t acx_colsum_fused_part_bytes(int64_t rows, int32_t D);
int acx_colsum_fused(acx_ctx* ctx, const float* x, int32_t ld, int64_t rows, int32_t D, float* out, float* part,
                     size_t part_bytes, uint32_t* counters, float beta, void* stream);
/* nprob column sums in ONE launch (part[i]: acx_colsum_fused_part_bytes(rows[i], D[i]) bytes each; `counters`: ncounters
 * zero-at-rest uint32, at least sum_i ceil(D[i] / 64)); and nprob row-partial tables reduced in one launch
 * (out_i[width_i] = sum_p part_i[p][:], the summation tree of acx_reduce_rows). */
int acx_colsum_fused_group(acx_ctx* ctx, int32_t nprob, const void* const* x, const int32_t* ld, const int64_t* rows,
                           const int32_t* D, void* const* out, void* const* part, uint32_t* counters, int32_t ncounters,
                           void* stream);
int acx_reduce_rows_group(acx_ctx* ctx, int32_t nprob, const void* const* part, void* const* out, const int32_t* nparts,
                          const int32_t* width, void* stream);

int acx_ctx_grad(acx_ctx* ctx, const float* dx, float* dctx, int32_t C, int32_t n_ctx, int32_t Lc, int32_t W,
                 int32_t shared_ctx, void* stream);
int acx_scatter_rows(acx_ctx* ctx, const float* src, const int64_t* idx, float* out, int64_t n, int32_t W,
                     void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Metrics epilogue: anomaly_clip_module.py:501-626 and the torchmetrics==0.11.0
 * curve functions it calls (requirements.txt:6; functional/classification/{precision_recall_curve,roc,auroc,
 * average_precision}.py).  All results are exact-integer or fixed-order f64 -- run-to-run deterministic.
 * --------------------------------------------------------------------------------------------------------- */
/* Stable LSD radix sort (4 passes of 8 bits) of (f32 key, u32 payload) pairs; replaces
 * `torch.argsort(preds, descending=True)` + gathers of _binary_clf_curve.  Not in place.  -0.0 < +0.0. */
int64_t acx_sort_workspace_bytes(int64_t n);
int acx_sort_pairs(acx_ctx* ctx, const float* keys, const uint32_t* vals, float* keys_out, uint32_t* vals_out,
                   int64_t n, int32_t descending, void* workspace, int64_t workspace_bytes, void* stream);
/* `batch` independent sorts of n pairs in one launch sequence (12 launches for any batch).  Problem b reads keys + b * key_stride and
 * vals + b * val_stride (val_stride = 0: all problems carry the SAME payload array); outputs are dense [batch][n].
 * workspace_bytes >= batch * acx_sort_workspace_bytes(n).  Replaces the per-class loop of anomaly_clip_module.py:507-518. */
int acx_sort_pairs_batched(acx_ctx* ctx, const float* keys, int64_t key_stride, const uint32_t* vals, int64_t val_stride,
                           float* keys_out, uint32_t* vals_out, int64_t n, int32_t batch, int32_t descending, void* workspace,
                           int64_t workspace_bytes, void* stream);

typedef struct acx_curve_result {   /* written to DEVICE memory */
  double auroc;          /* trapz(tpr, fpr) over the distinct thresholds; 0 when a class is absent (torchmetrics) */
  double ap;             /* sum (R_k - R_{k-1}) P_k; NaN without positives */
  int64_t n_pos, n_neg, n_distinct;
  int64_t opt_index;     /* sorted index of argmax(tpr - fpr) (first maximum, exact integer compare), -1 = the
                            prepended (0,0) point */
  float opt_threshold;   /* thresholds[argmax(tpr - fpr)] (anomaly_clip_module.py:526-527); 1.0 for the (0,0) point */
  float pad;
} acx_curve_result;
/* From pairs sorted by score DESCENDING: target_i = (label_i == cls) (negate=0) or (label_i != cls) (negate=1,
 * the reference's labels_binary, :520).  Optional curve_* arrays (capacity n) receive the n_distinct points
 * (tps, fps, threshold) of _binary_clf_curve; pass NULL to skip. */
int64_t acx_clf_curve_workspace_bytes(int64_t n);
int acx_clf_curve(acx_ctx* ctx, const float* sorted_scores, const uint32_t* sorted_labels, int64_t n, int32_t cls,
                  int32_t negate, acx_curve_result* result, int32_t* curve_tps, int32_t* curve_fps,
                  float* curve_thresholds, void* workspace, int64_t workspace_bytes, void* stream);
/* `batch` (1..64) curves in one launch sequence (4 launches): problem b reads sorted_scores + b * score_stride and
 * sorted_labels + b * label_stride, target = (label == cls[b]), or (label != cls[b]) where negate[b] != 0; results[b] is its record;
 * cls / negate are HOST arrays.  The optional curve arrays (all three or none) receive the points of problem 0 only.
 * workspace_bytes >= batch * acx_clf_curve_workspace_bytes(n). */
int acx_clf_curve_batched(acx_ctx* ctx, const float* sorted_scores, int64_t score_stride, const uint32_t* sorted_labels,
                          int64_t label_stride, int64_t n, int32_t batch, const int32_t* cls, const int32_t* negate,
                          acx_curve_result* results, int32_t* curve_tps, int32_t* curve_fps, float* curve_thresholds, void* workspace,
                          int64_t workspace_bytes, void* stream);
/* anomaly_clip_module.py:523-530, 628-656 (the ROC and PR figures plot every point of the curve): the curve of acx_clf_curve
 * (curve_tps / curve_fps, capacity entries, the first result->n_distinct valid) reduced to a figure's `columns` (1..4096) pixel
 * columns, on the device.  `result` is the DEVICE record the curve launch wrote: k = n_distinct, P = n_pos and N = n_neg are read
 * there, no host value depends on them.  Column of point j, by integer division: mode 0 (ROC) min(columns - 1, fps_j * columns / N),
 * all 0 when N == 0; mode 1 (PR) min(columns - 1, tps_j * columns / P), and no point at all when P == 0 (recall is NaN).  Height:
 * mode 0 tps_j; mode 1 the precision tps_j / (tps_j + fps_j), two of them compared as tps_a * (tps_b + fps_b) against
 * tps_b * (tps_a + fps_a) in 64 bits.  out (device, int32 [columns][4][3]) receives per column the (index, tps, fps) of the run's
 * first point, last point, lowest point and highest point (ties: the lowest index); an empty column holds (-1, -1, -1) four times.
 * Exact integers, fixed-order joins, no atomics: run-to-run identical.  capacity == 0 and n_distinct == 0 are valid (all empty). */
int64_t acx_curve_decimate_workspace_bytes(int64_t capacity);
int acx_curve_decimate(acx_ctx* ctx, const int32_t* curve_tps, const int32_t* curve_fps, int64_t capacity,
                       const acx_curve_result* result, int32_t mode, int32_t columns, int32_t* out, void* workspace,
                       int64_t workspace_bytes, void* stream);
/* anomaly_clip_module.py:538-581, 621-626, 673: y_pred and the integer counters behind top-1 / top-5 accuracy,
 * the confusion matrix and F1@{0.1..1.0}.  probs [n, C-1] (class_probs without the normal column), labels int64,
 * threshold = DEVICE pointer to the optimal threshold (e.g. &result->opt_threshold).  counts (int64, device,
 * 3C + C*C + 30 entries): top1_hit[C] | top5_hit[C] | class_n[C] | confusion[C][C] (row = true) | f1_tp[10] |
 * f1_fp[10] | f1_fn[10].  Probability ties rank the lower class index first (torch.topk leaves it unspecified). */
int acx_test_counts(acx_ctx* ctx, const float* scores, const float* probs, const int64_t* labels, int64_t n,
                    int32_t C, int32_t normal_idx, const float* threshold, int32_t* y_pred, int64_t* counts,
                    void* stream);
/* Anomaly events of unlabeled videos, on the device: only the event tables need to reach the host.  scores f32 [n]; probs f32
 * [n, C1] (class_probs without the normal column, as acx_test_counts takes them: 5 <= C1 <= 63, 0 <= normal_idx <= C1); row_off
 * int64 [videos + 1]: video v owns rows row_off[v] .. row_off[v + 1] - 1 (empty videos are allowed).  All three are DEVICE arrays.
 * Rules (exact: tests/events_ref.py restates them entry for entry):
 *   hot / warm  frame t is hot when !(s_t < hi), warm when !(s_t < lo) -- the reference's comparison (anomaly_clip_module.py:538),
 *               so a NaN score is hot.
 *   raw event   a maximal run of warm frames of one video that holds at least one hot frame (lo == hi: the maximal runs of the
 *               reference's y_pred != normal_idx).
 *   merging     consecutive raw events of a video are chained into one event while the gap between them is at most max_gap
 *               frames; the gap frames belong to the event; nothing merges across a video boundary.
 *   length      an event is kept when end - start + 1 >= min_len (start, end inclusive, relative to the video's first row);
 *               merging comes first.
 *   per event   over ALL its frames: peak = the largest non-NaN score (NaN when there is none), peak_frame = the first frame
 *               that attains it (start when every score is NaN), mean = f64 sum of the non-NaN scores / their number (NaN when
 *               there is none), hot_frames = the number of hot frames.
 *   class       every hot frame votes for argmax_k probs[t, k] (strict >, from -inf: NaN never wins, ties and an all-NaN row go to
 *               the lowest k); the event's class is the k with the most votes (ties: the lowest k), reported in the full label
 *               space (k + 1 when k >= normal_idx); votes = the winner's count.
 * Outputs (device): count int32 [videos] = ALL kept events of the video, also beyond max_events, or -1 for a video whose range
 * is not 0 <= row_off[v] <= row_off[v + 1] <= n (its rows are not read); events int32 [videos][max_events][6] = start, end,
 * class, votes, hot_frames, peak_frame; stats f64 [videos][max_events][2] = peak, mean.  Events in ascending start; the first
 * min(count, max_events) slots are filled, every other slot holds -1 / NaN.
 * Refused before any launch (ACX_E_BADARG): n or videos outside 0 .. 2^31 - 1, C1 / normal_idx out of domain, lo > hi or a NaN
 * threshold, max_gap < 0, min_len < 1, max_events < 1, videos * max_events >= 2^31.  Two launches, no float atomics, fixed-order
 * joins: run-to-run identical.  acx_score_events_workspace_bytes is host arithmetic (-1 for sizes the launch refuses); the present
 * decomposition keeps its carry in registers and needs 0 bytes, workspace may then be NULL. */
int64_t acx_score_events_workspace_bytes(int64_t n, int64_t videos, int32_t max_events);
int acx_score_events(acx_ctx* ctx, const float* scores, const float* probs, const int64_t* row_off, int64_t n, int64_t videos,
                     int32_t C1, int32_t normal_idx, float hi, float lo, int32_t max_gap, int32_t min_len, int32_t max_events,
                     int32_t* count, int32_t* events, double* stats, void* workspace, int64_t workspace_bytes, void* stream);

/* In-library launch timer used by bench.py's roofline leg: when enabled, every kernel launch is
 * bracketed by HIP events on the caller's stream.  kinds: 0 GEMM, 1 attention, 2 norm rows, 3 other.
 * acx_prof_collect synchronises the recorded events and returns per-kind launch counts and summed
 * durations (ms), then resets the recording. */
#define ACX_PROF_KINDS 4
/* on = 1: every launch kind; on = 2: the GEMM launches only (an event pair costs ~7 us of queue time: 260 launches of a headline
 * step with all kinds armed add 1.9 ms to its 131.5 ms, the ~110 GEMM launches alone 0.8 ms); on = 0: off */
int acx_prof_enable(acx_ctx* ctx, int on);
int acx_prof_collect(acx_ctx* ctx, int32_t* counts, double* total_ms);
/* executed GEMM flops (2*M*N*K of every acx_gemm / acx_gemm_tn launch) since acx_prof_enable(ctx, 1) */
int acx_prof_gemm_flops(acx_ctx* ctx, double* flops);
/* the acx_gemm_tn share of the above: flops since acx_prof_enable(ctx, 1); summed launch time and launch count of the events the
 * LAST acx_prof_collect consumed (call it after acx_prof_collect) */
int acx_prof_gemm_tn(acx_ctx* ctx, double* flops, double* total_ms, int32_t* launches);

/* ------------------------------------------------------------------------------------------
 * Measured roofline denominators (bench.py `peaks_measured`).  Not on the product path.
 * acx_probe_mfma: register-only MFMA loop on every SIMD (bf16 = 0: v_mfma_f32_32x32x2_f32, 1: v_mfma_f32_32x32x16_bf16),
 *   `iters` x 4 MFMAs per wave, waves_per_simd waves per SIMD; *flops_out (host) = flops the launch executes.
 *   bf16 = 2: mode 1 on RANDOM operands (four fragment pairs per lane); bf16 = 3: the same on v_mfma_f32_16x16x32_bf16 (sixteen
 *   16 x 16 accumulators = the same 64 registers, `iters` x 16 MFMAs per wave); bf16 = 4 (32x32x16) / 5 (16x16x32): one wave per SIMD
 *   (waves_per_simd must be 1), 128 x 128 outputs per wave, an iteration = one 32-wide K-step of three products whose operand
 *   fragments are all re-read from random bf16 data in LDS by ds_read_b128 (32 reads per wave: the plane-reuse kernel's half-step
 *   without DMA and barriers).
 * acx_probe_copy: dst = src, 16 bytes per lane, grid-stride: the HBM stream (read + write) ceiling. */
int acx_probe_mfma(acx_ctx* ctx, int32_t bf16, int32_t iters, int32_t waves_per_simd, float* sink, double* flops_out,
                   void* stream);
int acx_probe_copy(acx_ctx* ctx, const void* src, void* dst, int64_t bytes, void* stream);
/* acx_probe_read: reads `bytes` once (16 bytes per lane, grid-stride), writes nothing: the floor of a one-shot launch over an
 * input of that size -- the denominator for the head's skinny reductions (selector projection, column sums). */
int acx_probe_read(acx_ctx* ctx, const void* src, int64_t bytes, float* sink, void* stream);

/* ------------------------------------------------------------------------------------------
 * Collectives (acx_comm_init / acx_allreduce).  The reference exchanges gradients and SyncBatchNorm statistics
 * through Lightning DDP over NCCL (configs/trainer/ddp.yaml:1-9).  The Python host of this repository issues the same exchange through
 * torch.distributed -- backend "nccl" is RCCL on ROCm -- and that remains its default ("collectives"); these entry
 * points are the torch-free form of it for a C / C++ host: thin RCCL calls on the CALLER's stream (so they order with the library's
 * kernels like any launch, and a capturing stream records them into its HIP graph).  RCCL is opened with dlopen on first use
 * (libacx.so has no link-time dependency on it; a process that already loaded an RCCL -- PyTorch-ROCm -- shares that copy);
 * ACX_E_RCCL when it cannot be opened or a call fails.  One communicator per context, bound to the context's device.
 *   acx_comm_unique_id  rank 0: fills ACX_COMM_ID_BYTES opaque bytes (ncclGetUniqueId) that the host transports to every rank
 *   acx_comm_init       every rank, collectively: ncclCommInitRank(world, id, rank)
 *   acx_allreduce       in place over `count` elements of `dtype` (ACX_F32 / ACX_BF16 / ACX_F64 / ACX_I64), op ACX_COMM_SUM / MAX / MIN
 *   acx_allgather       `count` elements from every rank, rank-major, into recv[world * count]
 *   acx_comm_destroy    releases the communicator (acx_destroy does NOT: collective teardown is the caller's to order) */
#define ACX_COMM_ID_BYTES 128
enum { ACX_F64 = 16, ACX_I64 = 17 };                  /* element types of the collectives only */
enum { ACX_COMM_SUM = 0, ACX_COMM_MAX = 1, ACX_COMM_MIN = 2 };
int acx_comm_unique_id(void* id_out, size_t id_bytes);
int acx_comm_init(acx_ctx* ctx, int32_t rank, int32_t world, const void* unique_id);
int acx_comm_destroy(acx_ctx* ctx);
int acx_comm_info(acx_ctx* ctx, int32_t* rank, int32_t* world);   /* world = 0: no communicator */
int acx_allreduce(acx_ctx* ctx, void* buf, int64_t count, int32_t dtype, int32_t op, void* stream);
int acx_allgather(acx_ctx* ctx, const void* send, void* recv, int64_t count, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training batches from a feature set resident in device memory (feature_dataset.py:347-380, train mode).  `bank` is the
 * concatenation of every video's feature file as stored: [T_v * ncrops, D], frame t / crop c in row t * ncrops + c; row_off[v] is
 * video v's first bank row and frames[v] its T_v.  One launch draws a whole batch:
 *   out[b, c, n*L + l, :] = bank[row_off[vid[b]] + ((starts[b*N + n] + l*stride) mod frames[vid[b]]) * ncrops + c, :]
 * with out [B, ncrops, N*L, D].  All five tables are DEVICE pointers (row_off int64 [V], frames int32 [V], vid int32 [B] with
 * values in [0, V), starts int32 [B*N]); the modulus is a true modulus and every element offset is 64-bit.  A pure copy in
 * 16-byte pieces: D % 4 == 0 and 16-byte aligned bank / out, else ACX_E_BADARG; so are null pointers and non-positive
 * N / L / stride / ncrops / D.  B == 0 is ACX_OK without a launch.  The same video may appear several times in a batch. */
int acx_sample_segments(acx_ctx* ctx, const float* bank, const int64_t* row_off, const int32_t* frames, const int32_t* vid,
                        const int32_t* starts, float* out, int32_t B, int32_t N, int32_t L, int32_t stride, int32_t ncrops,
                        int32_t D, void* stream);

/* Test-mode tiles of a group of V videos of such a bank in ONE launch (feature_dataset.py:347-376: start indices k * L * stride,
 * so row r of a video's tile is frame (r * stride) mod T), written video after video, each crop-major -- the tensor
 * AnomalyCLIP.forward_test_many takes:
 *   out[out_off[j] + c * rows[j] + r, :] = bank[row_off[vid[j]] + ((r * stride) mod frames[vid[j]]) * ncrops + c, :]
 * for j < V, c < ncrops, r < rows[j], with rows[j] = N * L * S_j a multiple of N * L, out_off[j] = ncrops * (rows[0] + ... +
 * rows[j-1]) and total_rows = ncrops * (rows[0] + ... + rows[V-1]).  blk[total_rows / (N * L)] maps every block of N * L output
 * rows to its j.  row_off, frames, vid (int32 [V], values inside the bank), out_off (int64 [V]), rows (int32 [V]) and blk (int32) are
 * DEVICE pointers.  The same pure copy: D % 4 == 0 and 16-byte aligned bank / out, else ACX_E_BADARG; so are null pointers,
 * non-positive sizes, a total_rows that is no multiple of N * L, and total_rows or total_rows * stride at or above 2^31.
 * V == 0 is ACX_OK without a launch. */
int acx_tile_videos(acx_ctx* ctx, const float* bank, const int64_t* row_off, const int32_t* frames, const int32_t* vid,
                    const int64_t* out_off, const int32_t* rows, const int32_t* blk, float* out, int32_t V, int64_t total_rows,
                    int32_t N, int32_t L, int32_t stride, int32_t ncrops, int32_t D, void* stream);

/* Half-precision feature files: the same bank with float16 rows (IEEE binary16, numpy's '<f2').  acx_sample_segments_f16 and
 * acx_tile_videos_f16 are the two gathers above on such a bank: the same tables, arguments, limits and formulas, `out` stays
 * float32 (a half widens exactly).  A half row of D % 4 == 0 elements is 8-byte aligned only, so a lane loads 8 bytes and stores
 * 16: D % 4 == 0, an 8-byte aligned bank and a 16-byte aligned out, else ACX_E_BADARG. */
int acx_sample_segments_f16(acx_ctx* ctx, const void* bank, const int64_t* row_off, const int32_t* frames, const int32_t* vid,
                            const int32_t* starts, float* out, int32_t B, int32_t N, int32_t L, int32_t stride, int32_t ncrops,
                            int32_t D, void* stream);
int acx_tile_videos_f16(acx_ctx* ctx, const void* bank, const int64_t* row_off, const int32_t* frames, const int32_t* vid,
                        const int64_t* out_off, const int32_t* rows, const int32_t* blk, float* out, int32_t V, int64_t total_rows,
                        int32_t N, int32_t L, int32_t stride, int32_t ncrops, int32_t D, void* stream);

/* dst[r, c] = half(src[r * ld + c]) for r < rows, c < cols: float32 rows `ld` floats apart -> contiguous float16 rows, rounded to
 * nearest even with subnormal halves (in integer arithmetic: numpy's astype(float16) bit for bit, NaN payloads included, under any
 * denormal mode).  A finite input whose half is not finite (|x| >= 65520) is written as +-inf and counted: *overflow_count (DEVICE
 * int64, the caller zeroes it) is increased by their number, one atomic add per workgroup that met any.  NaN and +-inf pass
 * uncounted.  cols % 4 == 0, ld % 4 == 0, ld >= cols, a 16-byte aligned src and 8-byte aligned dst / overflow_count, else
 * ACX_E_BADARG; rows == 0 is ACX_OK without a launch. */
int acx_cast_rows_f16(acx_ctx* ctx, const float* src, void* dst, int64_t rows, int32_t cols, int64_t ld, int64_t* overflow_count,
                      void* stream);

/* dst[i] = float(src[i]) over rows * D contiguous float16 elements (exact): D % 4 == 0, an 8-byte aligned src and a 16-byte
 * aligned dst, else ACX_E_BADARG; rows == 0 is ACX_OK without a launch. */
int acx_expand_rows_f16(acx_ctx* ctx, const void* src, float* dst, int64_t rows, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG frames (the reference decodes with Pillow: video_dataset.py:204 `Image.open(...).convert("RGB")`): Huffman decoding
 * on the host, everything after it on the device, bit for bit Pillow's RGB (libjpeg-turbo's defaults: the integer "islow" IDCT,
 * "fancy" upsampling, the table-exact colour conversion).
 *
 * The supported set: 8-bit samples, SOF0 / SOF1, ONE interleaved scan with Ss = 0, Se = 63, Ah = Al = 0; one component, or three
 * read as YCbCr with luma sampling 1x1, 2x1 or 2x2 and both chroma components 1x1.  Everything else a decoder may meet
 * (progressive, arithmetic coding, 12 bits, four components, an Adobe segment with transform 0 or 2, other sampling factors,
 * several scans, DNL, a downsampled chroma plane of one or two samples per row -- W <= 4: libjpeg replicates those instead of
 * filtering them) is ACX_E_UNSUPPORTED; a malformed file is ACX_E_BADARG.  The two
 * host functions take untrusted bytes, keep no state and allocate nothing: they may be called from many threads at once. */
typedef struct acx_jpeg_info {
  int32_t width, height, ncomp;
  int32_t hmax, vmax;                      /* the largest sampling factors (the luma's) */
  int32_t mcus_x, mcus_y;
  int32_t restart_interval;                /* MCUs between restart markers, 0: none */
  int32_t comp_h[4], comp_v[4];            /* sampling factors (a single component counts as 1 x 1) */
  int32_t comp_tq[4], comp_td[4], comp_ta[4]; /* quantisation / DC / AC table of each component */
  int32_t comp_width[4], comp_height[4];   /* real samples: ceil(width * h / hmax), ceil(height * v / vmax) */
  int32_t blocks_wide[4], blocks_high[4];  /* MCUs * sampling factor: padded to whole MCUs */
  int64_t coef_offset[4];                  /* first coefficient of each component, in elements */
  int64_t coef_elems;                      /* coefficients of the frame */
  int64_t scan_offset;                     /* offset of the entropy-coded data in the file */
  uint16_t qtab[4][64];                    /* quantisation tables in NATURAL (row-major) order */
  uint8_t qtab_present[4];
  uint8_t huff_present[2][4];              /* [0: DC, 1: AC][table] */
  uint8_t huff_bits[2][4][17];             /* codes of each length 1 .. 16 */
  uint8_t huff_vals[2][4][256];
} acx_jpeg_info;

/* walks the markers up to the scan (SOI, APPn / COM skipped, DQT with 8- or 16-bit entries, DHT, SOF0 / SOF1, DRI, SOS) */
int acx_jpeg_parse(const uint8_t* data, size_t n, acx_jpeg_info* info);
/* every block's 64 coefficients in natural order, NOT dequantised, into the ZEROED buffer coef[coef_elems]: component after
 * component, each [blocks_high][blocks_wide][64].  FF 00 stuffing; a restart marker re-aligns to a byte and resets the DC
 * predictors.  A stream that ends early, a code no table holds, a run past the block's end: ACX_E_BADARG. */
int acx_jpeg_entropy_decode(const uint8_t* data, size_t n, const acx_jpeg_info* info, int16_t* coef, size_t coef_elems);

/* F frames of ONE geometry -> rgb uint8 [F,H,W,3] (the input of acx_preprocess_crops / acx_preprocess_frames).  coef: int16
 * [F][coef_elems] as acx_jpeg_entropy_decode writes them; qtabs: uint16 [F][ncomp][64], each frame's table of each COMPONENT in
 * natural order; ncomp 1 or 3, (hs, vs) the luma sampling factors (1,1), (2,1) or (2,2), W >= 5 where hs = 2.  planes: uint8 [F][coef_elems] scratch (the
 * component planes, padded to whole blocks).  coef, qtabs and rgb 16-byte aligned, planes 8-byte aligned; F * H * W below 2^31.
 * Two launches: dequantisation + inverse DCT into the planes, then upsampling + colour conversion + packing. */
int acx_jpeg_reconstruct(acx_ctx* ctx, const int16_t* coef, const uint16_t* qtabs, int32_t H, int32_t W, int32_t ncomp, int32_t hs,
                         int32_t vs, int32_t F, uint8_t* planes, uint8_t* rgb, void* stream);

/* ---- Huffman decoding on the device: decode="gpu_entropy".  Only the marker walk and the byte un-stuffing stay on the host. */
#define ACX_JPEG_SCAN_ALIGN 4            /* a packed scan is read as 32-bit words: its start and its padded length are multiples */
#define ACX_JPEG_MAX_SUBSEQ 1024         /* subsequences (threads of the one workgroup) per frame */
/* a frame's Huffman tables as they travel to the device: the huff_* fields of acx_jpeg_info and each component's table indices */
typedef struct acx_jpeg_huff {
  uint8_t present[2][4];                   /* [0: DC, 1: AC][table] */
  uint8_t bits[2][4][17];
  uint8_t vals[2][4][256];
  uint8_t td[4], ta[4];                    /* DC / AC table of each component */
} acx_jpeg_huff;                           /* 2200 bytes */

/* Copies the entropy-coded segment at info->scan_offset into dst[cap] with every FF 00 replaced by FF (and fill FFs dropped), up to
 * the first marker or the end of the file; *payload_bytes is the number of bytes copied, and dst is zero-padded up to the next
 * multiple of ACX_JPEG_SCAN_ALIGN.  huff, if not null, receives the tables.  The contract of acx_jpeg_parse: untrusted bytes,
 * every read and write bounded, no state, no allocation.  A file with a restart interval is ACX_E_UNSUPPORTED (the host decoder
 * takes it); a dst too small, or an info the host decoder would refuse, is ACX_E_BADARG. */
int acx_jpeg_scan_pack(const uint8_t* data, size_t n, const acx_jpeg_info* info, uint8_t* dst, size_t cap, int64_t* payload_bytes,
                       acx_jpeg_huff* huff);

/* Huffman-decodes F frames of ONE geometry in one launch, one workgroup of ACX_JPEG_MAX_SUBSEQ threads per frame (the
 * self-synchronising parallel decode: anomalyclip_amd/csrc/acx_jpeg_sync.h).  DEVICE pointers: scans[scans_bytes], the packed
 * scans; scan_off[F] / scan_bits[F], each frame's first bit (a multiple of 32) and number of bits in it; huff[F]; coef int16
 * [F][coef_elems], ZEROED; status int32 [F].  max_scan_bits: the longest scan of the batch, known to the host that packed it.
 * sub_bits: bits per subsequence, a multiple of 32, or 0 for each frame's smallest (ceil(bits / 1024) rounded up to 32); an
 * explicit value with which 1024 subsequences do not cover max_scan_bits is ACX_E_BADARG before any launch, the needed value in
 * acx_last_error.  coef is written exactly as acx_jpeg_entropy_decode writes it for the frames it accepts; status[f] is 0 exactly
 * for those, and ACX_E_BADARG for the others (whose coefficients are unspecified, inside their frame). */
int acx_jpeg_entropy_decode_dev(acx_ctx* ctx, const uint8_t* scans, int64_t scans_bytes, const int64_t* scan_off, const int32_t* scan_bits,
                                const acx_jpeg_huff* huff, int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs, int32_t F,
                                int64_t max_scan_bits, int32_t sub_bits, int16_t* coef, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * Qualitative videos (data.visualize=True; the reference draws a matplotlib figure per frame: src/utils/visualizer.py): the
 * per-frame picture composed on the device, then encoded as baseline JPEG -- the transform on the device, Huffman coding on the
 * host or (acx_jpeg_entropy_encode_dev) on the device.  anomalyclip_amd/visualizer.py lays the picture out and writes the
 * Motion-JPEG file. */
typedef struct acx_viz_geom {
  int32_t Hc, Wc;                          /* the canvas */
  int32_t H, W;                            /* the source frames */
  int32_t fx, fy, fw, fh;                  /* the inner frame rectangle: the source resized to fw x fh */
  int32_t border;                          /* width of the border around it */
  int32_t bx, by, bh;                      /* bars: left edge of bar 0, top row of the panel, its height PH; a bar of height h
                                              covers rows by + bh - h ... by + bh - 1 */
  int32_t bar_pitch, bar_w;                /* bar k covers columns bx + k * bar_pitch ... + bar_w - 1 */
  int32_t C1;                              /* bars: 1 .. 64 */
  int32_t sx, sy, sw, sh;                  /* the score panel; sw is PW of the cursor's x = sx + (i * (sw - 1)) / T */
  int32_t cursor_w;
  int32_t T;                               /* frames of the video */
  float threshold;
} acx_viz_geom;

/* acx_viz_compose: B canvases [B,Hc,Wc,3] uint8 in one launch sequence.  Every canvas starts as static_layer [Hc,Wc,3]; then, later
 * items over earlier ones: frame b of frames [B,H,W,3] resized to the inner rectangle bit for bit as Pillow's
 * Image.resize((fw, fh), BILINEAR) (hbounds/hcoef [fw,2] / [fw,hksize], vbounds/vcoef [fh,2] / [fh,vksize]: the tables of
 * anomalyclip_amd/resample.py for the triangle filter; tmp: [B,H,fw,3] uint8 scratch), a border around it, (0,0,255) where
 * scores[b] < threshold and (255,0,0) otherwise; C1 bars of height floor(softmax[b,k] * PH + 0.5) (float32, product and sum rounded
 * separately; clipped to 0 .. PH) in (128,128,128), the three largest softmax[b,:] (the lower index wins a tie) in (255,0,0) where
 * scores[b] >= threshold; a cursor of cursor_w columns in (255,0,0) over the score panel's height at frame_idx[b] (none for an
 * index outside 0 .. T - 1).  All pointers but geom are DEVICE pointers.  ACX_E_BADARG: C1 outside 1 .. 64, or a rectangle that
 * does not lie strictly inside the canvas (nothing is clipped). */
int acx_viz_compose(acx_ctx* ctx, const uint8_t* static_layer, const uint8_t* frames, const float* scores, const float* softmax,
                    const int32_t* frame_idx, const int32_t* hbounds, const int32_t* hcoef, int32_t hksize, const int32_t* vbounds,
                    const int32_t* vcoef, int32_t vksize, const acx_viz_geom* geom, int32_t B, uint8_t* tmp, uint8_t* canvases,
                    void* stream);

/* acx_jpeg_forward: B canvases [B,Hc,Wc,3] uint8 -> the quantised coefficients of baseline JPEG, YCbCr 4:2:0, int16
 * [B][Hc * Wc * 3 / 2] in the layout acx_jpeg_entropy_decode writes and acx_jpeg_reconstruct reads (luma sampling 2x2).  Integer
 * arithmetic throughout ("Qualitative videos"): JFIF colour conversion in 16-bit fixed point, 2x2 chroma
 * mean, level shift, samples with 6 fraction bits, the 8x8 orthonormal DCT as two passes of a 14-bit matrix, division by the
 * table rounded half away from zero, clamped to +-1023 (what the Annex K tables code: AC category 10, DC differences category 11).
 * qtabs: DEVICE uint16 [2][64], luma then chroma, natural order.  Hc and Wc multiples of 16 (ACX_E_BADARG otherwise); canvases,
 * qtabs and coef 16-byte aligned. */
int acx_jpeg_forward(acx_ctx* ctx, const uint8_t* canvases, const uint16_t* qtabs, int32_t Hc, int32_t Wc, int32_t B, int16_t* coef,
                     void* stream);

/* Host only, like acx_jpeg_parse: no context, no GPU call, no state, no allocation -- callable from many threads at once.
 * One frame's coefficients (coef[coef_elems], the layout above for an H x W frame: blocks padded to whole 16 x 16 MCUs) and its
 * tables (qtabs: HOST uint16 [2][64], natural order, entries 1 .. 255) -> a complete JFIF file in dst[cap]: APP0, two DQT, SOF0
 * with luma sampling 2x2, four DHT with the Annex K tables, one interleaved scan with FF 00 stuffing, EOI.  Returns the number of
 * bytes, or a negative code: ACX_E_WORKSPACE when cap is too small (nothing is written past dst + cap), ACX_E_BADARG for a
 * coefficient those tables cannot code or a coef_elems that is not the frame's.  acx_jpeg_encode_bound(H, W) is always enough. */
int64_t acx_jpeg_entropy_encode(const int16_t* coef, size_t coef_elems, const uint16_t* qtabs, int32_t H, int32_t W, uint8_t* dst,
                                size_t cap);
int64_t acx_jpeg_encode_bound(int32_t H, int32_t W);

/* Host only, like acx_jpeg_entropy_encode: the 623 bytes that function writes before the scan of an H x W frame with the tables
 * qtabs (HOST uint16 [2][64], natural order, entries 1 .. 255) -- APP0, two DQT, SOF0, four DHT, SOS -- into dst[cap].  Returns
 * 623, or ACX_E_WORKSPACE when cap is smaller (nothing is written past dst + cap), or ACX_E_BADARG (null pointer, a size outside
 * 1 .. 65535, a table entry outside 1 .. 255). */
int64_t acx_jpeg_encode_header(const uint16_t* qtabs, int32_t H, int32_t W, uint8_t* dst, size_t cap);

/* The Huffman coder of acx_jpeg_entropy_encode on the device, for B frames of one size in one launch sequence on `stream`
 * (Visualizer(entropy="gpu"); the phases: anomalyclip_amd/csrc/acx_jpeg_enc_dev.h).  All pointers are DEVICE pointers.
 * coef: int16 [B][coef_elems] as acx_jpeg_forward writes them (an H x W frame padded to whole 16 x 16 MCUs), 16-byte aligned; header: the
 * header_bytes bytes every file begins with (acx_jpeg_encode_header).  Frame f's file -- byte for byte the one
 * acx_jpeg_entropy_encode writes -- goes to files + f * cap; nbytes[f] is the size it needs, also when it does not fit;
 * status[f] is that function's code for the frame: 0, ACX_E_WORKSPACE when nbytes[f] > cap (the slot then holds the file's first
 * cap bytes), or ACX_E_BADARG for a coefficient the Annex K tables cannot code (a DC difference beyond category 11, |AC| > 1023;
 * nbytes[f] is 0 and the slot is left as it was).  Nothing is written at or past files + (f + 1) * cap, and one frame's refusal
 * leaves the other frames of the batch as they are without it.  The workspace (16-byte aligned, at least
 * acx_jpeg_entropy_encode_dev_workspace_bytes(H, W, B) bytes) need not be cleared: the call zeroes what it merges into on the
 * stream, so a workspace may be used again by the next call on the same stream.  Before any launch: ACX_E_BADARG for a null
 * pointer or one not aligned, B < 1, B, H or W outside 1 .. 65535, header_bytes outside 1 .. 65535, cap < 0, or a size whose blocks x 1,658 bits (a
 * block's longest code) reach 2^31 -- bit offsets are 32-bit; ACX_E_WORKSPACE for a workspace that is too small.
 * acx_jpeg_entropy_encode_dev_workspace_bytes returns 0 for the arguments the call refuses. */
size_t acx_jpeg_entropy_encode_dev_workspace_bytes(int32_t H, int32_t W, int32_t B);
int acx_jpeg_entropy_encode_dev(acx_ctx* ctx, const int16_t* coef, const uint8_t* header, int32_t header_bytes, int32_t H, int32_t W,
                                int32_t B, uint8_t* files, int64_t cap, int32_t* nbytes, int32_t* status, void* workspace,
                                size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACX_H_ */
