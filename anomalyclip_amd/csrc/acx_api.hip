// libacx context management and the whole-encoder drivers (host code only: they sequence the
// kernels of acx_gemm / acx_norm / acx_attn / acx_head on the caller's stream; no allocation,
// no synchronisation, safe to capture in a hipGraph).
#include "acx_internal.h"

#include <new>
#include <stdlib.h>

#ifndef ACX_ATTN_F32IN_DEFAULT
#define ACX_ATTN_F32IN_DEFAULT 1   // ACX_OPT_ATTN_F32IN as acx_create sets it (A/B builds of the other default: -DACX_ATTN_F32IN_DEFAULT=0)
#endif

#ifndef ACX_LN16_FC_DEFAULT
#define ACX_LN16_FC_DEFAULT 1      // ACX_PREC_F32X6_LN16: c_fc on fp16 planes as well as the in-projection (the A/B build that measures the in-projection alone: 0)
#endif

#ifndef ACX_R16_OUT_DEFAULT
#define ACX_R16_OUT_DEFAULT 1      // ACX_PREC_F32X6_R16: out-proj on fp16 planes (the A/B build that measures c_proj alone: 0)
#endif
#ifndef ACX_R16_PROJ_DEFAULT
#define ACX_R16_PROJ_DEFAULT 1     // ACX_PREC_F32X6_R16: c_proj on fp16 planes (the A/B build that measures out-proj alone: 0)
#endif

#ifndef ACX_QKV16_DEFAULT
#define ACX_QKV16_DEFAULT 1        // ACX_PREC_F32X6_QKV16: q | k | v as fp16 planes into the three-product attention (the A/B build that keeps ACX_PREC_F32X6_R16's records: 0)
#endif

#ifndef ACX_CLS_FOLD_DEFAULT
#define ACX_CLS_FOLD_DEFAULT 1     // ACX_OPT_CLS_FOLD as acx_create sets it
#endif

thread_local char acx_tls_err[512] = {0};

namespace {
// The options the transformer driver's plan reads.  Filled in one place (tf_opts); acx_create takes its defaults from kCreateOpts.
struct TfOpts {
  int x6_min_tiles;                              // ACX_OPT_X6_MIN_TILES
  bool attn_f32in, cls_fold;                     // ACX_OPT_ATTN_F32IN, ACX_OPT_CLS_FOLD
  bool ln16_fc;                                  // ACX_LN16_FC_DEFAULT (a build constant)
  bool r16_out, r16_proj;                        // ACX_R16_OUT_DEFAULT, ACX_R16_PROJ_DEFAULT (build constants)
  bool qkv16;                                    // ACX_QKV16_DEFAULT (a build constant)
};
constexpr TfOpts kCreateOpts = {18, ACX_ATTN_F32IN_DEFAULT != 0, ACX_CLS_FOLD_DEFAULT != 0, ACX_LN16_FC_DEFAULT != 0, ACX_R16_OUT_DEFAULT != 0,
                                ACX_R16_PROJ_DEFAULT != 0, ACX_QKV16_DEFAULT != 0};
constexpr TfOpts kNoCtxOpts = {512, false, false, ACX_LN16_FC_DEFAULT != 0, ACX_R16_OUT_DEFAULT != 0, ACX_R16_PROJ_DEFAULT != 0,
                              ACX_QKV16_DEFAULT != 0};   // a driver called with ctx == NULL
// query: acx_transformer_plan, which answers for a context as acx_create leaves it when it has none (like the other route queries)
inline TfOpts tf_opts(const acx_ctx* ctx, bool query) {
  if (!ctx) return query ? kCreateOpts : kNoCtxOpts;
  return {ctx->opt_x6_min_tiles, ctx->opt_attn_f32in != 0, ctx->opt_cls_fold != 0, kCreateOpts.ln16_fc, kCreateOpts.r16_out, kCreateOpts.r16_proj,
          kCreateOpts.qkv16};
}
}  // namespace

extern "C" int acx_attention_cls(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo, int32_t batch,
                                 int32_t L, int32_t heads, void* stream);

extern "C" int acx_version(void) { return ACX_VERSION; }

extern "C" int acx_create(acx_ctx** out, int device) {
  if (!out) return acx_fail(nullptr, ACX_E_BADARG, "acx_create: null out%s");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || device < 0 || device >= n) {
    snprintf(acx_tls_err, 512, "acx_create: device %d not available (%s, %d devices)", device,
             e == hipSuccess ? "ok" : hipGetErrorString(e), n);
    return ACX_E_HIP;
  }
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) {
    snprintf(acx_tls_err, 512, "acx_create: hipGetDeviceProperties: %s", hipGetErrorString(e));
    return ACX_E_HIP;
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    snprintf(acx_tls_err, 512, "acx_create: libacx is built for gfx950 only, device %d is %s", device, prop.gcnArchName);
    return ACX_E_UNSUPPORTED;
  }
  acx_ctx* c = new (std::nothrow) acx_ctx;
  if (!c) return acx_fail(nullptr, ACX_E_HIP, "acx_create: out of host memory%s");
  c->device = device;
  c->multiprocessors = prop.multiProcessorCount;
  c->opt_ring_min_tiles = 512;
  c->opt_sk_max_m = 320;
  c->opt_tn_p256_min_rows = 4096;
  c->opt_x6_cus = 0;
  c->opt_x6_tail = 0;
  c->opt_x6_strip = 1;
  c->opt_ln_rider = 1;
  c->opt_attn_f32in = kCreateOpts.attn_f32in;
  c->opt_cls_fold = kCreateOpts.cls_fold;
  c->comm = nullptr; c->comm_rank = 0; c->comm_world = 0;
  c->opt_x6_min_tiles = kCreateOpts.x6_min_tiles;
  c->err[0] = 0;
  c->prof_on = false;
  c->prof_gemm_only = false;
  c->prof_n = c->prof_created = 0;
  c->prof_gemm_flops = 0.0;
  c->prof_tn_flops = c->prof_tn_ms = 0.0; c->prof_tn_count = 0;
  c->prof_ev = new (std::nothrow) hipEvent_t[2 * ACX_PROF_MAX];
  c->prof_kind = new (std::nothrow) unsigned char[ACX_PROF_MAX];
  *out = c;
  return ACX_OK;
}

extern "C" void acx_destroy(acx_ctx* ctx) {
  if (!ctx) return;
  for (int i = 0; i < 2 * ctx->prof_created; ++i) (void)hipEventDestroy(ctx->prof_ev[i]);
  delete[] ctx->prof_ev;
  delete[] ctx->prof_kind;
  delete ctx;
}

extern "C" int acx_prof_enable(acx_ctx* ctx, int on) {
  if (!ctx || !ctx->prof_ev || !ctx->prof_kind) return acx_fail(ctx, ACX_E_BADARG, "acx_prof_enable: no context%s");
  ctx->prof_on = on != 0;
  ctx->prof_gemm_only = on == 2;
  if (on) { ctx->prof_n = 0; ctx->prof_gemm_flops = 0.0; ctx->prof_tn_flops = 0.0; }
  return ACX_OK;
}

extern "C" int acx_prof_gemm_flops(acx_ctx* ctx, double* flops) {
  if (!ctx || !flops) return acx_fail(ctx, ACX_E_BADARG, "acx_prof_gemm_flops: null pointer%s");
  *flops = ctx->prof_gemm_flops;
  return ACX_OK;
}

extern "C" int acx_prof_gemm_tn(acx_ctx* ctx, double* flops, double* total_ms, int32_t* launches) {
  if (!ctx || !flops || !total_ms || !launches) return acx_fail(ctx, ACX_E_BADARG, "acx_prof_gemm_tn: null pointer%s");
  *flops = ctx->prof_tn_flops; *total_ms = ctx->prof_tn_ms; *launches = ctx->prof_tn_count;
  return ACX_OK;
}

extern "C" int acx_prof_collect(acx_ctx* ctx, int32_t* counts, double* total_ms) {
  if (!ctx || !counts || !total_ms) return acx_fail(ctx, ACX_E_BADARG, "acx_prof_collect: null pointer%s");
  for (int k = 0; k < ACX_K_COUNT; ++k) { counts[k] = 0; total_ms[k] = 0.0; }
  ctx->prof_tn_ms = 0.0; ctx->prof_tn_count = 0;
  for (int i = 0; i < ctx->prof_n; ++i) {
    hipError_t e = hipEventSynchronize(ctx->prof_ev[2 * i + 1]);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]);
    if (e != hipSuccess) {
      snprintf(ctx->err, 512, "acx_prof_collect: %s", hipGetErrorString(e));
      return ACX_E_HIP;
    }
    int kind = ctx->prof_kind[i];
    if (kind == ACX_K_GEMM_TN) { ctx->prof_tn_ms += ms; ctx->prof_tn_count++; kind = ACX_K_GEMM; }
    counts[kind]++;
    total_ms[kind] += ms;
  }
  ctx->prof_n = 0;
  return ACX_OK;
}

extern "C" int acx_set_option(acx_ctx* ctx, int32_t option, int64_t value) {
  if (!ctx) return acx_fail(ctx, ACX_E_BADARG, "acx_set_option: no context%s");
  switch (option) {
    case ACX_OPT_RING_MIN_TILES:
      if (value < 1) return acx_fail(ctx, ACX_E_BADARG, "acx_set_option: ring_min_tiles must be >= 1%s");
      ctx->opt_ring_min_tiles = (int)value;
      return ACX_OK;
    case ACX_OPT_TN_P256_MIN_ROWS:
      if (value < 1) return acx_fail(ctx, ACX_E_BADARG, "acx_set_option: tn_p256_min_rows must be >= 1%s");
      ctx->opt_tn_p256_min_rows = (int)(value > 0x7fffffff ? 0x7fffffff : value);
      return ACX_OK;
    case ACX_OPT_X6_TAIL_SPLIT:
      ctx->opt_x6_tail = value != 0;
      return ACX_OK;
    case ACX_OPT_X6_STRIP_TAIL:
      if (value < 0 || value > 3) return acx_fail(ctx, ACX_E_BADARG, "acx_set_option: x6_strip_tail is 0 (off), 1 (cost model), 2 or 3 (forced strip width)%s");
      ctx->opt_x6_strip = (int)value;
      return ACX_OK;
    case ACX_OPT_LN_RIDER:
      if (value < 0) return acx_fail(ctx, ACX_E_BADARG, "acx_set_option: ln_rider is 0 (off), 1 (cost model) or a row count%s");
      ctx->opt_ln_rider = (long long)value;
      return ACX_OK;
    case ACX_OPT_ATTN_F32IN:
      ctx->opt_attn_f32in = value != 0;
      return ACX_OK;
    case ACX_OPT_CLS_FOLD:
      ctx->opt_cls_fold = value != 0;
      return ACX_OK;
    case ACX_OPT_X6_MIN_TILES:
      if (value < 1) return acx_fail(ctx, ACX_E_BADARG, "acx_set_option: x6_min_tiles must be >= 1%s");
      ctx->opt_x6_min_tiles = (int)(value > 0x7fffffff ? 0x7fffffff : value);
      return ACX_OK;
    case ACX_OPT_X6_CUS:
      if (value < 0) return acx_fail(ctx, ACX_E_BADARG, "acx_set_option: x6_cus must be >= 0%s");
      ctx->opt_x6_cus = (int)(value > 4096 ? 4096 : value);
      return ACX_OK;
    case ACX_OPT_SK_MAX_M:
      if (value < 0) return acx_fail(ctx, ACX_E_BADARG, "acx_set_option: sk_max_m must be >= 0%s");
      ctx->opt_sk_max_m = (int)value;
      return ACX_OK;
    default:
      return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_set_option: unknown option %s%ld", "", (long)option);
  }
}

extern "C" int acx_get_option(acx_ctx* ctx, int32_t option, int64_t* value) {
  if (!ctx || !value) return acx_fail(ctx, ACX_E_BADARG, "acx_get_option: no context or no result pointer%s");
  switch (option) {
    case ACX_OPT_RING_MIN_TILES: *value = ctx->opt_ring_min_tiles; return ACX_OK;
    case ACX_OPT_SK_MAX_M: *value = ctx->opt_sk_max_m; return ACX_OK;
    case ACX_OPT_TN_P256_MIN_ROWS: *value = ctx->opt_tn_p256_min_rows; return ACX_OK;
    case ACX_OPT_X6_CUS: *value = ctx->opt_x6_cus; return ACX_OK;
    case ACX_OPT_X6_TAIL_SPLIT: *value = ctx->opt_x6_tail; return ACX_OK;
    case ACX_OPT_X6_STRIP_TAIL: *value = ctx->opt_x6_strip; return ACX_OK;
    case ACX_OPT_X6_MIN_TILES: *value = ctx->opt_x6_min_tiles; return ACX_OK;
    case ACX_OPT_LN_RIDER: *value = ctx->opt_ln_rider; return ACX_OK;
    case ACX_OPT_ATTN_F32IN: *value = ctx->opt_attn_f32in; return ACX_OK;
    case ACX_OPT_CLS_FOLD: *value = ctx->opt_cls_fold; return ACX_OK;
    default:
      return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_get_option: unknown option %s%ld", "", (long)option);
  }
}

extern "C" const char* acx_last_error(acx_ctx* ctx) { return ctx ? ctx->err : acx_tls_err; }

namespace {

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

struct TfWs {   // transformer scratch carved from the caller's workspace
  char *h, *qkv, *att, *mlp, *splitk;
  char *hp, *mp;  // ACX_PREC_F32X6: three bf16 planes of a [rows, W] / [rows, 4W] GEMM input (nullptr otherwise)
  char* qkv3;     // ACX_PREC_F32X6: three bf16 planes of q | k | v [rows, 3W] (the plane attention's operands)
  size_t splitk_bytes, total;
};

// the plane modes of the drivers: ACX_PREC_F32X6 (six products: f32-accurate) and ACX_PREC_F32X3 (the three leading products)
static inline bool is_xmode(int prec) {
  return prec == ACX_PREC_F32X6 || prec == ACX_PREC_F32X3 || prec == ACX_PREC_F16X3 || prec == ACX_PREC_F32X6_LN16 ||
         prec == ACX_PREC_F32X6_R16 || prec == ACX_PREC_F32X6_QKV16 || prec == ACX_PREC_F16X3S;
}
// the six-product modes whose LayerNorm-fed products read fp16 planes (ACX_PREC_F32X6_R16: the residual products too)
static inline bool is_r16(int prec) { return prec == ACX_PREC_F32X6_R16 || prec == ACX_PREC_F32X6_QKV16; }
static inline bool is_ln16(int prec) { return prec == ACX_PREC_F32X6_LN16 || is_r16(prec); }
// the plane scales a driver call brings per layer: ln_1, ln_2 | att, hid | qkv
static inline int scales_per_layer(int prec) { return prec == ACX_PREC_F32X6_QKV16 ? 5 : prec == ACX_PREC_F32X6_R16 ? 4 : 2; }
static inline const char* ln16_name(int prec) {
  return prec == ACX_PREC_F32X6_QKV16 ? "ACX_PREC_F32X6_QKV16" : prec == ACX_PREC_F32X6_R16 ? "ACX_PREC_F32X6_R16" : "ACX_PREC_F32X6_LN16";
}
struct XMode {
  int pairs;                                     // acx_gemm_desc.pairs of the driver's plane products (and the attention's products)
  bool f16;                                      // ACX_PREC_F16X3: two fp16 planes per operand (weights scaled by ACX_F16X3_WSCALE)
};
// ACX_PREC_F16X3S: ACX_PREC_F16X3 in everything but the attention rule (tf_plan)
static inline bool is_f16x3(int prec) { return prec == ACX_PREC_F16X3 || prec == ACX_PREC_F16X3S; }
static inline XMode xmode_of(int prec) { return {(prec == ACX_PREC_F32X3 || is_f16x3(prec)) ? 3 : 6, is_f16x3(prec)}; }
// what LayerNorm / acx_vit_patches write for the plane products of a mode
static inline int plane_dtype_of(int prec) { return is_f16x3(prec) ? ACX_F16X2P : prec == ACX_PREC_F32X3 ? ACX_BF16X2P : ACX_BF16X3P; }

TfWs carve_tf(char* base, int64_t rows, int W, int prec = ACX_PREC_F32) {
  TfWs w;
  size_t off = 0;
  w.h = base + off;   off += al((size_t)rows * W * 4);
  w.qkv = base + off; off += al((size_t)rows * 3 * W * 4);
  w.att = base + off; off += al((size_t)rows * W * 4);
  w.mlp = base + off; off += al((size_t)rows * 4 * W * 4);
  // split-K scratch for skinny problems (text tower: 14 x 77 rows): 8 partial copies of the widest output
  // ... and for the partial last wave of big problems: <= 256 tiles of 128x128 outputs, 4 splits
  w.splitk_bytes = rows <= 4096 ? (size_t)8 * rows * 4 * W * 4 : (size_t)4 * 256 * 128 * 128 * 4;
  w.splitk = base + off; off += al(w.splitk_bytes);
  w.hp = w.mp = w.qkv3 = nullptr;
  if (is_xmode(prec)) {
    w.hp = base + off; off += al((size_t)3 * rows * W * 2);
    w.mp = base + off; off += al((size_t)3 * rows * 4 * W * 2);
    w.qkv3 = base + off; off += al((size_t)3 * rows * 3 * W * 2);
  }
  w.total = off;
  return w;
}

// The pruned last layer's scratch (acx_vit_encode's cls_ws): everything of that layer that exists for the CLS rows only.
struct ClsWs {
  float *xc, *attc, *x1;   // [batch, W] each: the final CLS residual stream, the attention output, the stream after out_proj
  char *hc, *mc;           // [batch, W] LayerNorm output, [batch, 4W] MLP hidden (f32 or bf16; the fold's Q sits in mc before c_fc)
};
inline size_t cls_ws_bytes(int batch, int W) { return (size_t)8 * batch * W * 4; }   // xc, attc, x1, hc: W floats a row; mc: 4W
ClsWs carve_cls(float* base, int batch, int W) {
  const size_t n = (size_t)batch * W;
  return {base, base + n, base + 2 * n, (char*)(base + 3 * n), (char*)(base + 4 * n)};
}

// ACX_PREC_F32X6: the large GEMMs of the ViT as f32-accurate products on the bf16 matrix cores (acx_gemm_desc.pairs = 6): the
// f32 input is split into three bf16 planes (acx_split_bf16x3), the weights come as three planes from the caller.  A problem
// the persistent 256x256 kernel does not take (few rows) stays on the f32 MFMA kernels.  planes_ws: the workspace has the planes.
bool x6_takes(const TfOpts& o, bool planes_ws, int64_t M, int N, int K, int lda) {
  if (!planes_ws || !ACX_DBG_SWITCH("X6", true)) return false;
  const int64_t rtiles = ((M + 255) / 256) * ((N + 255) / 256);
  return rtiles >= o.x6_min_tiles && K % 256 == 0 && N % 8 == 0 && (size_t)M * lda * 2 < ((size_t)1 << 32) &&
         (size_t)N * K * 2 < ((size_t)1 << 32);
}

// One y = act(A W^T + bias) [+ residual] of the drivers.
struct Product {
  int kernel;                  // ACX_TF_GEMM_ROWS: A is rows of a_dtype, acx_gemm picks the kernel; ACX_TF_GEMM_X6: A and Wb are K-panel planes
  const void* A; int a_dtype, lda;
  const float* Wf;             // f32 weight [N, K]
  const void* Wb;              // its bf16 copy (ACX_PREC_BF16) or its planes (plane modes)
  int64_t w_plane_bytes;       // 0: N * K * 2 (a row range of a taller weight: that weight's)
  int ldw, M, N, K;
  const float* bias; int act;
  const float* residual; int ldr;   // ldr 0: ldc
  void* C; int c_dtype, ldc;
  void* scratch; size_t scratch_bytes;   // for a K split, free while the product runs
  const acx_ln_job* ln;        // plane kernel: the LayerNorm of the output rows follows (acx_gemm_ln: part of it rides in the last round)
  float a_scale;               // plane kernel, ACX_PREC_F32X6_LN16: > 0 = A is the fp16 pair planes of a_scale * (LayerNorm output), Wb the fp16
                               // pair planes of 2^10 w: three products, the accumulator leaves multiplied by 2^-10 / a_scale.  0: the mode's planes
                               // (ACX_PREC_F32X6_R16: the same for the planes of a_scale * (attention output) / a_scale * (MLP hidden))
  float c_scale;               // plane kernel, ACX_PREC_F32X6_R16's c_fc: > 0 = C is the fp16 pair planes of c_scale * value (acx_gemm_desc.c_scale)
};

struct TfMode {
  int prec;                    // acx_gemm_desc.prec of the row products and everything small (plane modes: f32)
  int hdt, pdt;                // what LayerNorm writes: rows of hdt (c_fc's hidden too), planes of pdt
  XMode xm;
};

int missing_weights(acx_ctx* ctx, bool planes, int prec) {
  if (planes) return acx_fail(ctx, ACX_E_BADARG, "driver: missing bf16 x 3 weight planes for ACX_PREC_F32X6%s");
  return acx_fail(ctx, ACX_E_BADARG, "driver: missing %s weight copy for the requested precision", prec == ACX_PREC_BF16 ? "bf16" : "f32");
}

acx_gemm_desc desc_of(const Product& p) {        // all of a descriptor but the weight, the arithmetic and the scratch
  acx_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.A = p.A; d.C = p.C;
  d.M = p.M; d.N = p.N; d.K = p.K; d.lda = p.lda; d.ldw = p.ldw; d.ldc = p.ldc;
  d.a_dtype = p.a_dtype; d.c_dtype = p.c_dtype;
  d.bias = p.bias; d.act = p.act; d.residual = p.residual; d.ldr = p.ldr ? p.ldr : p.ldc;
  return d;
}

// Both operands' planes are in K-PANEL layout (ACX_BF16X3P: the driver's producers -- LayerNorm, the attention, c_fc's epilogue,
// acx_split_bf16x3_panel -- write it, the caller's weight planes come in it): a 256-row x 32-column unit of the plane-reuse
// kernel is then ONE contiguous 16 KB block (+5-6 % on the ViT products against row-major planes, profiles/r05_gemm_x6_notes.txt).
int run_x6(acx_ctx* ctx, XMode xm, const Product& p, hipStream_t s) {
  acx_gemm_desc d = desc_of(p);
  d.W = p.Wb;
  if (p.a_scale > 0.f) xm = {3, true};
  d.a_dtype = xm.f16 ? ACX_F16 : ACX_BF16; d.prec = ACX_PREC_BF16; d.pairs = xm.pairs; d.panels = 3;
  d.out_scale = p.a_scale > 0.f ? 1.f / (ACX_F16X3_WSCALE * p.a_scale) : xm.f16 ? 1.f / ACX_F16X3_WSCALE : 0.f;
  d.c_scale = p.c_scale;
  d.a_plane_stride = (int64_t)p.M * p.lda * 2;
  d.w_plane_stride = p.w_plane_bytes ? p.w_plane_bytes : (int64_t)p.N * p.K * 2;
  // scratch for the K split of a partly filled last round of tiles (acx_gemm: row-major outputs only)
  d.workspace = p.scratch; d.workspace_bytes = p.scratch ? p.scratch_bytes : 0;
  return p.ln ? acx_gemm_ln(ctx, &d, p.ln, s) : acx_gemm(ctx, &d, s);
}

int run_rows1(acx_ctx* ctx, int prec, const Product& p, hipStream_t s) {
  acx_gemm_desc d = desc_of(p);
  d.W = prec == ACX_PREC_BF16 ? p.Wb : (const void*)p.Wf;
  if (!d.W) return missing_weights(ctx, false, prec);
  d.prec = prec;
  d.workspace = p.scratch_bytes ? p.scratch : nullptr; d.workspace_bytes = p.scratch_bytes;
  return acx_gemm(ctx, &d, s);
}

// Row product with tail handling: a grid of T tiles runs in ceil(T/512) waves of 128x128 tiles (2 per CU); when
// the last wave would be mostly empty (e.g. N=768: 9.23 waves -> 10), the rows of that partial wave are issued as a
// second launch that fills the chip (9 waves + ~1/3 wave): acx_gemm runs it on 64x64 tiles (f32, four blocks per CU)
// or splits K over the scratch handed in here (other precisions).  The f32 tail gets no scratch: the 64x64 kernel would
// split a K >= 1024 over it (ViT-L/14: 512 tail rows, K = 1024 / 4096), and the tail rows would then sum K in another order
// than the head rows -- identical frames would no longer give identical rows across the launch.
int run_rows(acx_ctx* ctx, int prec, const Product& p, hipStream_t s) {
  bool tail_split = ACX_DBG_SWITCH("TAIL_SPLIT", true);
  if (tail_split && !p.ldr) {   // the persistent strip-stream kernel balances its own tail
    acx_gemm_desc d = desc_of(p);
    d.prec = prec;
    if (acx_gemm_takes_strip_stream(&d)) tail_split = false;
  }
  const int tiles_n = (p.N + 127) / 128, tiles_m = (p.M + 127) / 128;
  const long tiles = (long)tiles_m * tiles_n;
  const long full = tiles / 512;
  const long rem = tiles - full * 512;
  if (tail_split && p.scratch && full >= 2 && rem > 0 && rem <= 256 && !p.ldr) {
    const int head_rows = (int)((full * 512) / tiles_n) * 128;
    const int tail_rows = p.M - head_rows;
    if (head_rows > 0 && tail_rows > 0 && (size_t)4 * tail_rows * p.N * sizeof(float) <= p.scratch_bytes) {
      const size_t asz = p.a_dtype == ACX_BF16 ? 2 : 4, csz = p.c_dtype == ACX_BF16 ? 2 : 4;
      Product head = p, tail = p;
      head.M = head_rows; head.scratch = nullptr; head.scratch_bytes = 0;
      tail.M = tail_rows;
      tail.A = (const char*)p.A + (size_t)head_rows * p.lda * asz;
      tail.C = (char*)p.C + (size_t)head_rows * p.ldc * csz;
      if (p.residual) tail.residual = p.residual + (size_t)head_rows * p.ldc;
      if (prec == ACX_PREC_F32) { tail.scratch = nullptr; tail.scratch_bytes = 0; }
      const int rc = run_rows1(ctx, prec, head, s);
      return rc ? rc : run_rows1(ctx, prec, tail, s);
    }
  }
  return run_rows1(ctx, prec, p, s);
}

int run(acx_ctx* ctx, const TfMode& m, const Product& p, hipStream_t s) {
  return p.kernel == ACX_TF_GEMM_X6 ? run_x6(ctx, m.xm, p, s) : run_rows(ctx, m.prec, p, s);
}

// ---- the layer plan: every decision of the transformer drivers, taken once, before the first launch ----------------------------
struct TfGeom {
  int batch, L, W, heads, layers, causal, prec;
  bool prune;                  // the LAST layer is evaluated only where its output is consumed: token 0 of every sequence (clip/model.py:285)
  bool planes_ws;              // the workspace holds the planes of a plane mode (TfWs.hp)
  int act;                     // c_fc's activation, ACX_ACT_QUICKGELU or ACX_ACT_GELU (the executor's alone: tf_plan never reads it)
};

// the MLP activation a driver was handed: 0 means QuickGELU (callers of the headers before ACX_ACT_GELU); *act = the epilogue's value
int tf_act(acx_ctx* ctx, const char* who, int32_t given, int prec, int* act) {
  if (given != 0 && given != ACX_ACT_QUICKGELU && given != ACX_ACT_GELU)
    return acx_fail(ctx, ACX_E_BADARG, "%s: act must be 0 / ACX_ACT_QUICKGELU or ACX_ACT_GELU", who);
  if (given == ACX_ACT_GELU && prec == ACX_PREC_BF16)
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "%s: ACX_ACT_GELU with ACX_PREC_BF16 (the bf16 MFMA routes are no parity path)", who);
  *act = given == ACX_ACT_GELU ? ACX_ACT_GELU : ACX_ACT_QUICKGELU;
  return ACX_OK;
}
// the head dimension of a driver geometry: 64, 80, or 0 (neither)
inline int tf_head_dim(int width, int heads) { return heads <= 0 ? 0 : width == heads * 64 ? 64 : width == heads * 80 ? 80 : 0; }
struct TfHave { bool f32[4], alt[4]; };   // in_proj, out_proj, fc, proj of every block: the f32 weight, the *_w_bf16 copy / planes
struct TfPlan {
  TfMode mode;
  bool ln16_qkv, ln16_fc;      // ACX_PREC_F32X6_LN16: the in-projection / c_fc of the body layers run on fp16 planes (ln_1 / ln_2 write them)
  bool r16_out, r16_proj;      // ACX_PREC_F32X6_R16: out-proj / c_proj of the body layers run on fp16 planes (the attention / c_fc write them)
  bool qkv16;                  // ACX_PREC_F32X6_QKV16: q | k | v of the body layers leave the in-projection as fp16 planes (the fp16 planes attention)
  acx_tf_layer_plan_t body, before_pruned, pruned;   // the three layer shapes (before_pruned: body with the pruned layer's ln_1 job)
  bool prune;
};

// layer l's record: one of the three shapes; the first layer's ln_1 has no product before it, the last layer's proj no ln_1 behind it
acx_tf_layer_plan_t tf_layer(const TfPlan& p, int l, int layers) {
  acx_tf_layer_plan_t r = p.prune && l == layers - 1 ? p.pruned : p.prune && l == layers - 2 ? p.before_pruned : p.body;
  if (l == 0 && r.ln1 == ACX_TF_LN_RIDDEN) r.ln1 = ACX_TF_LN_PLANES;
  if (l == layers - 1) r.proj.ln_job = 0;
  return r;
}

inline acx_tf_product_t tf_rows(int c_dtype, int scratch) { return {ACX_TF_GEMM_ROWS, c_dtype, scratch, 0}; }
inline acx_tf_product_t tf_x6(int c_dtype, int scratch, bool ln_job) { return {ACX_TF_GEMM_X6, c_dtype, scratch, ln_job ? 1 : 0}; }

// Whether a body layer's ACX_PREC_F32X6_R16 in-projection (fp16 A planes, f32 rows out) is a launch whose K acx_gemm may split across
// workgroups: fewer tiles than workgroups, the small launches -- the dispatcher's own answers, its split model's scratch query
// (acx_gemm_scratch: bytes > 0 = a split is possible for this shape) and its route with the scratch the driver hands it (acx_gemm_route;
// no operand is dereferenced, any aligned address does).  Such a launch keeps its f32 rows: fp16 plane outputs never split K.
bool in_proj_splits(acx_ctx* ctx, const TfGeom& g, int64_t rows) {
  acx_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.A = d.W = d.C = d.workspace = (void*)(uintptr_t)256;
  d.M = (int)rows; d.N = 3 * g.W; d.K = g.W; d.lda = d.ldw = g.W; d.ldc = 3 * g.W; d.ldr = d.ldc;
  d.a_dtype = ACX_F16; d.c_dtype = ACX_F32; d.prec = ACX_PREC_BF16; d.pairs = 3; d.panels = 3;
  d.out_scale = 1.f / ACX_F16X3_WSCALE;
  d.a_plane_stride = rows * g.W * 2; d.w_plane_stride = (int64_t)3 * g.W * g.W * 2;
  d.workspace_bytes = (size_t)rows * g.W * 4;
  acx_gemm_scratch_t sc;
  if (acx_gemm_scratch(ctx, &d, 1, &sc) != ACX_OK || sc.workspace_bytes > 0) return true;
  acx_gemm_route_t r;
  return acx_gemm_route(ctx, &d, &r) != ACX_OK || r.ksplit > 1;
}

// Pure host arithmetic on its arguments.  err: where a refusal's text goes; ACX_PREC_F32X6_QKV16 also hands it to acx_gemm's dry queries
// (in_proj_splits), which read its workgroup count and options as acx_gemm itself would and launch nothing.
int tf_plan(acx_ctx* err, const TfGeom& g, const TfHave& have, const TfOpts& o, TfPlan* p) {
  memset(p, 0, sizeof(*p));
  const int W = g.W, L = g.L;
  const int64_t rows = (int64_t)g.batch * L;
  const bool xmode = is_xmode(g.prec);
  TfMode& m = p->mode;
  m.xm = xmode_of(g.prec);
  m.pdt = plane_dtype_of(g.prec);
  m.prec = xmode ? ACX_PREC_F32 : g.prec;         // everything that is not one of the four large GEMMs runs as in f32 mode
  m.hdt = m.prec == ACX_PREC_BF16 ? ACX_BF16 : ACX_F32;
  p->prune = g.prune;
  // head dimension 80 (width == 80 heads: ViT-H-14's image tower): the f32 attentions of acx_attn_hd.h, non-causal, under ACX_PREC_F32 and
  // the six bf16-plane products only; no planes attention, no fold of the pruned layer, no LayerNorm rider.  Every other geometry keeps
  // head dimension 64's rules below, record for record.
  const bool hd80 = tf_head_dim(W, g.heads) == 80;
  if (hd80 && (g.causal || (g.prec != ACX_PREC_F32 && g.prec != ACX_PREC_F32X6)))
    return acx_fail(err, ACX_E_UNSUPPORTED, "driver: head dimension 80 runs non-causal under ACX_PREC_F32 or ACX_PREC_F32X6 only%s");
  const int cpl = m.xm.f16 ? ACX_F16X2P : ACX_BF16X3P;   // a plane product's plane output
  auto x6 = [&](int N, int K) { return xmode && x6_takes(o, g.planes_ws, rows, N, K, K); };
  const bool x6_qkv = x6(3 * W, W), x6_out = x6(W, W), x6_fc = x6(4 * W, W), x6_proj = x6(W, 4 * W), x6_kv = x6(2 * W, W);
  // ACX_PREC_F32X6: the LayerNorm behind a residual product (out-proj -> ln_2, c_proj -> the next layer's ln_1, K | V LayerNorm of the
  // pruned last layer included) is handed to the product (acx_gemm_ln: the idle workgroups of its last round of tiles run part of it)
  const bool ln_ride = m.pdt == ACX_BF16X3P && !hd80;
  // ACX_PREC_F32X6_LN16: the plane-kernel in-projection and (ACX_LN16_FC_DEFAULT) c_fc read fp16 pair planes -- their weights come in that
  // format, so the rule is per product and holds for every geometry; everything else is the six-product plan below, record for record
  const bool ln16 = is_ln16(g.prec), r16 = is_r16(g.prec);
  if (ln16 && W != 768 && W != 1024)
    return acx_fail(err, ACX_E_UNSUPPORTED, "driver: %s is built for widths 768 and 1024", ln16_name(g.prec));
  p->ln16_qkv = ln16 && x6_qkv;
  p->ln16_fc = ln16 && x6_fc && o.ln16_fc;
  // bf16 mode, non-causal (the ViT): q/k/v, the attention and its output stay bf16 end to end -- half the
  // QKV store traffic, bf16-MFMA attention, and a bf16 A operand (LDS-DMA kernels) for the out-projection
  const bool ab = m.prec == ACX_PREC_BF16 && !g.causal && L <= 224 && ACX_DBG_SWITCH("ATTN_BF16", true);
  // the attention on the bf16 matrix cores (acx_attention_p3): q | k | v leave the in-projection as three bf16 planes
  const bool att_p3 = x6_qkv && x6_out && !g.causal && !hd80 && L > 192 && L <= 208 && ACX_DBG_SWITCH("ATTN_P3", true);
  // ACX_PREC_F16X3S: every other non-causal sequence takes the streaming fp16 planes attention (acx_attention_s16)
  const bool att_s16 = g.prec == ACX_PREC_F16X3S && x6_qkv && x6_out && !g.causal && L <= 1024 && !att_p3;
  // ... or, six products (ACX_OPT_ATTN_F32IN), as f32 rows the attention splits itself (acx_attention_p3f): no plane round trip
  // ACX_PREC_F32X6_R16: a residual product goes fp16 only where it AND its producer take the plane kernels -- out-proj behind the planes
  // attention (whose f32-rows arm writes the fp16 planes: taken whatever ACX_OPT_ATTN_F32IN says, out-proj's weights come as fp16 planes
  // for this sequence length), c_proj behind a c_fc that itself reads fp16 planes.  The rule depends on the geometry's L and W and the
  // build constants alone wherever the product is a plane product, so the caller binds the weights by one plan query.
  p->r16_out = r16 && o.r16_out && att_p3;
  p->r16_proj = r16 && o.r16_proj && p->ln16_fc && x6_proj;
  const bool att_p3f = att_p3 && ln_ride && (o.attn_f32in || p->r16_out);
  // ACX_PREC_F32X6_QKV16: behind an in-projection that reads fp16 planes, in front of an out-projection that reads them, q | k | v go
  // as fp16 planes too and the attention is its three-product fp16 form.  An fp16 plane output never takes a K split, so a layer whose
  // ACX_PREC_F32X6_R16 in-projection acx_gemm would split (few tiles: small launches) keeps that record.
  p->qkv16 = g.prec == ACX_PREC_F32X6_QKV16 && o.qkv16 && p->r16_out && p->ln16_qkv && att_p3f && !in_proj_splits(err, g, rows);
  const bool qkv_planes = (att_p3 && !att_p3f) || att_s16;
  // ... or on f32 rows, writing the out-projection's three planes itself
  // (head dimension 80: acx_attention_x3_hd, at every L)
  const bool att_x3 = hd80 ? x6_out : x6_out && !g.causal && L > 128 && L <= 1024 && (L > 224 || ACX_DBG_SWITCH("ATTN16", true));
  // ACX_OPT_CLS_FOLD (every precision but bf16): the pruned layer without K and V -- ln_1 and Q for the CLS rows, then
  // acx_attention_cls_fold reads the residual stream itself.  Its u | z scratch (2 heads W floats per frame) lives in the f32 q | k | v
  // buffer (3 L W floats per frame): a geometry with 2 heads > 3 L tokens (fewer than 11 tokens at 16 heads; no CLIP backbone) keeps
  // the K | V path, whatever the option says.
  const bool cls_fold = g.prune && m.prec != ACX_PREC_BF16 && o.cls_fold && !hd80 && L <= 1024 &&
                        acx_attention_cls_fold_workspace_bytes(g.batch, g.heads) <= (size_t)rows * 3 * W * 4;
  const bool kv_planes = g.prune && !cls_fold && x6_kv;   // the pruned layer's K | V product runs on the plane kernel

  // refusals, in the order the walk meets them: in-projection, the fp16 gate, the other products, the pruned layer
  auto need = [&](bool planes, int i) { return (planes || m.prec == ACX_PREC_BF16 ? have.alt[i] : have.f32[i]) ? 0 : missing_weights(err, planes, m.prec); };
  int rc;
  if (g.layers > (g.prune ? 1 : 0)) {
    if ((rc = need(x6_qkv, 0))) return rc;
    if (m.xm.f16 && (x6_qkv || x6_out || x6_fc || x6_proj) && !((att_p3 || att_s16) && x6_fc && x6_proj))
      return acx_fail(err, ACX_E_UNSUPPORTED, "driver: ACX_PREC_F16X3 needs the planes attention (192 < L <= 208) and all four products on the plane kernel%s");
    if ((rc = need(x6_out, 1)) || (rc = need(x6_fc, 2)) || (rc = need(x6_proj, 3))) return rc;
  }
  if (g.prune && g.layers > 0) {
    if (kv_planes && (rc = need(true, 0))) return rc;
    for (int i = 0; i < 4; ++i) if ((rc = need(false, i))) return rc;
  }

  // x = x + attn(ln_1(x)); x = x + mlp(ln_2(x))                      clip/model.py:215-216
  // (plane modes: the producers of the four large GEMMs' inputs write the planes themselves -- LayerNorm, the plane attentions and
  // the QuickGELU epilogue of c_fc; an f32 attention output or MLP hidden in front of a plane product goes through acx_split_bf16x3_panel.
  // Scratch: a free f32 buffer -- ws.h at every plane product, LayerNorm's output went to the planes or has been consumed; ws.qkv /
  // ws.mlp where the product writes the planes of that buffer's contents)
  acx_tf_layer_plan_t& b = p->body;
  b.ln1 = !x6_qkv ? ACX_TF_LN_ROWS : ln_ride && x6_proj ? ACX_TF_LN_RIDDEN : ACX_TF_LN_PLANES;
  b.ln1_dtype = p->ln16_qkv ? ACX_F16X2P : x6_qkv ? m.pdt : m.hdt;
  b.in_proj = !x6_qkv ? tf_rows(ab ? ACX_BF16 : ACX_F32, ACX_TF_BUF_SPLITK)
                      : qkv_planes ? tf_x6(cpl, ACX_TF_BUF_QKV, false) : tf_x6(ACX_F32, ACX_TF_BUF_H, false);
  b.att = ab ? ACX_TF_ATT_BF16 : att_p3f ? ACX_TF_ATT_P3F : att_p3 ? ACX_TF_ATT_P3N : att_s16 ? ACX_TF_ATT_S16
          : att_x3 ? (hd80 ? ACX_TF_ATT_HD_X3_PANEL : ACX_TF_ATT_X3_PANEL) : hd80 ? ACX_TF_ATT_HD_F32 : ACX_TF_ATT_F32;
  b.att_products = b.att == ACX_TF_ATT_P3N ? (m.xm.f16 ? 103 : m.xm.pairs) : 0;
  b.att_out_dtype = p->r16_out ? ACX_F16X2P : 0;
  if (p->qkv16) {
    b.in_proj = tf_x6(ACX_F16X2P, ACX_TF_BUF_QKV, false);
    b.att = ACX_TF_ATT_P3N;
    b.att_products = 103;
  }
  b.split_att = x6_out && !att_x3 && !att_p3 && !att_s16;
  b.out_proj = x6_out ? tf_x6(ACX_F32, ACX_TF_BUF_H, ln_ride && x6_fc) : tf_rows(ACX_F32, ACX_TF_BUF_SPLITK);
  b.ln2 = !x6_fc ? ACX_TF_LN_ROWS : b.out_proj.ln_job ? ACX_TF_LN_RIDDEN : ACX_TF_LN_PLANES;
  b.ln2_dtype = p->ln16_fc ? ACX_F16X2P : x6_fc ? m.pdt : m.hdt;
  // QuickGELU(c_fc) straight into the planes of c_proj's input when c_proj takes the plane kernel too
  b.fc = !x6_fc ? tf_rows(m.hdt, ACX_TF_BUF_SPLITK) : x6_proj ? tf_x6(p->r16_proj ? ACX_F16X2P : cpl, ACX_TF_BUF_MLP, false) : tf_x6(ACX_F32, ACX_TF_BUF_H, false);
  b.split_mlp = x6_proj && !x6_fc;
  // c_proj carries the next layer's ln_1 where that writes planes: a whole layer with its in-projection on the plane kernel ...
  b.proj = x6_proj ? tf_x6(ACX_F32, ACX_TF_BUF_H, ln_ride && x6_qkv) : tf_rows(ACX_F32, ACX_TF_BUF_SPLITK);
  // ... or the pruned last layer's K | V product (none under ACX_OPT_CLS_FOLD: that layer reads x itself)
  p->before_pruned = b;
  p->before_pruned.proj.ln_job = x6_proj && ln_ride && kv_planes;

  // the pruned layer: K | V for all tokens (rows [W, 3W) of in_proj) or the fold; everything else for `batch` rows, on the row kernels
  acx_tf_layer_plan_t& c = p->pruned;
  c.pruned = 1;
  c.ln1 = cls_fold ? ACX_TF_LN_CLS : !kv_planes ? ACX_TF_LN_ROWS : p->before_pruned.proj.ln_job ? ACX_TF_LN_RIDDEN : ACX_TF_LN_PLANES;
  c.ln1_dtype = kv_planes ? (p->ln16_qkv ? ACX_F16X2P : m.pdt) : m.hdt;
  c.in_proj = kv_planes ? tf_x6(ACX_F32, ACX_TF_BUF_NONE, false) : tf_rows(ACX_F32, ACX_TF_BUF_NONE);
  c.att = cls_fold ? ACX_TF_ATT_CLS_FOLD : hd80 ? ACX_TF_ATT_HD_CLS : ACX_TF_ATT_CLS;
  c.out_proj = c.proj = tf_rows(ACX_F32, ACX_TF_BUF_NONE);
  c.ln2 = ACX_TF_LN_CLS;
  c.ln2_dtype = m.hdt;
  c.fc = tf_rows(m.hdt, ACX_TF_BUF_NONE);
  return ACX_OK;
}

// the plan of a driver call: the options of its context, the weights its blocks carry
int tf_plan_call(acx_ctx* ctx, const TfGeom& g, const acx_block_weights* blk, TfPlan* p) {
  TfHave have;
  for (int i = 0; i < 4; ++i) have.f32[i] = have.alt[i] = true;
  for (int l = 0; l < g.layers; ++l) {
    const void* f32[4] = {blk[l].in_proj_w, blk[l].out_proj_w, blk[l].fc_w, blk[l].proj_w};
    const void* alt[4] = {blk[l].in_proj_w_bf16, blk[l].out_proj_w_bf16, blk[l].fc_w_bf16, blk[l].proj_w_bf16};
    for (int i = 0; i < 4; ++i) { have.f32[i] &= f32[i] != nullptr; have.alt[i] &= alt[i] != nullptr; }
  }
  return tf_plan(ctx, g, have, tf_opts(ctx, false), p);
}

// ---- the executor: walks the layers and launches what the records say ----------------------------------------------------------
struct TfRun {
  acx_ctx* ctx; const TfGeom& g; const TfMode& m; const TfWs& ws; hipStream_t s;
  const float* ln_scales;      // ACX_PREC_F32X6_LN16: [2 layers] plane scales of ln_1, ln_2; ACX_PREC_F32X6_R16: [4 layers] ln_1, ln_2, att, hid;
                               // ACX_PREC_F32X6_QKV16: [5 layers] ... and qkv (host)
  int64_t rows() const { return (int64_t)g.batch * g.L; }
  bool r16() const { return is_r16(g.prec); }
  int nsc() const { return scales_per_layer(g.prec); }
  // the scale of LayerNorm `which` (0 ln_1, 1 ln_2) of layer l where it writes ACX_PREC_F32X6_LN16's fp16 planes, else 0
  float lnsc(int dtype, int l, int which) const { return is_ln16(g.prec) && dtype == ACX_F16X2P ? ln_scales[nsc() * l + which] : 0.f; }
  // ACX_PREC_F32X6_R16: the scale of layer l's attention output (which = 2) / MLP hidden (3) where `dtype` says it leaves as fp16 planes, else 0
  // (ACX_PREC_F32X6_QKV16: which = 4, the in-projection's output planes)
  float r16sc(int dtype, int l, int which) const { return r16() && dtype == ACX_F16X2P ? ln_scales[nsc() * l + which] : 0.f; }

  // product i (0 in_proj, 1 out_proj, 2 fc, 3 proj) of block b on M rows, run as r says; A, C and residual are the caller's to set
  Product product(const acx_block_weights& b, int i, const acx_tf_product_t& r, int64_t M) const {
    const int W = g.W;
    Product p;
    memset(&p, 0, sizeof(p));
    p.kernel = r.kernel; p.c_dtype = r.c_dtype; p.M = (int)M;
    switch (i) {
      case 0: p.Wf = b.in_proj_w; p.Wb = b.in_proj_w_bf16; p.bias = b.in_proj_b; p.N = 3 * W; p.K = W; break;
      case 1: p.Wf = b.out_proj_w; p.Wb = b.out_proj_w_bf16; p.bias = b.out_proj_b; p.N = W; p.K = W; break;
      case 2: p.Wf = b.fc_w; p.Wb = b.fc_w_bf16; p.bias = b.fc_b; p.N = 4 * W; p.K = W; p.act = g.act; break;
      default: p.Wf = b.proj_w; p.Wb = b.proj_w_bf16; p.bias = b.proj_b; p.N = W; p.K = 4 * W; break;
    }
    p.lda = p.ldw = p.K; p.ldc = p.N; p.a_dtype = m.hdt;
    const size_t f = (size_t)rows() * W * 4;
    switch (r.scratch) {
      case ACX_TF_BUF_SPLITK: p.scratch = ws.splitk; p.scratch_bytes = ws.splitk_bytes; break;
      case ACX_TF_BUF_H: p.scratch = ws.h; p.scratch_bytes = f; break;
      case ACX_TF_BUF_QKV: p.scratch = ws.qkv; p.scratch_bytes = 3 * f; break;
      case ACX_TF_BUF_MLP: p.scratch = ws.mlp; p.scratch_bytes = 4 * f; break;
      default: break;
    }
    return p;
  }
  int norm(const float* x, int64_t ldx, const float* w, const float* b, void* y, int64_t ldy, int dtype, int64_t n, float sc = 0.f) const {
    if (sc > 0.f) return acx_layernorm_rows(ctx, x, ldx, w, b, y, dtype, sc, n, 0, g.W, 1e-5f, ACX_NORM_LAYER, s);   // fp16 planes of sc * y
    return acx_layernorm(ctx, x, ldx, w, b, y, ldy, dtype, n, g.W, 1e-5f, ACX_NORM_LAYER, s);
  }
  // ln_1 / ln_2 of all rows: to ws.h, to the planes of ws.hp, or already run behind the previous residual product
  int norm_all(int kind, int dtype, const float* x, const float* w, const float* b, float sc) const {
    if (kind == ACX_TF_LN_RIDDEN) return ACX_OK;
    return norm(x, g.W, w, b, kind == ACX_TF_LN_PLANES ? ws.hp : ws.h, g.W, dtype, rows(), kind == ACX_TF_LN_PLANES ? sc : 0.f);
  }
  // the LayerNorm a residual product carries: the planes of the mode, or (sc > 0) ACX_PREC_F32X6_LN16's fp16 planes of sc * y
  acx_ln_job job(const float* w, const float* b, float sc = 0.f) const {
    return {w, b, ws.hp, sc > 0.f ? ACX_F16X2P : m.pdt, 1e-5f, ACX_NORM_LAYER, sc};
  }
  int go(const Product& p) const { return run(ctx, m, p, s); }

  // l: the layer; next_ln1_dtype: what the NEXT layer's ln_1 writes (the job c_proj carries)
  int body(const acx_tf_layer_plan_t& r, const acx_block_weights& b, const acx_block_weights* next, float* x, int l, int next_ln1_dtype) const {
    const int W = g.W, batch = g.batch, L = g.L, heads = g.heads;
    auto planes = [](const acx_tf_product_t& q) { return q.c_dtype != ACX_F32 && q.c_dtype != ACX_BF16; };
    const float sc1 = lnsc(r.ln1_dtype, l, 0), sc2 = lnsc(r.ln2_dtype, l, 1);
    const float s_att = r16sc(r.att_out_dtype, l, 2), s_hid = r16sc(r.fc.c_dtype, l, 3);
    const float s_qkv = g.prec == ACX_PREC_F32X6_QKV16 ? r16sc(r.in_proj.c_dtype, l, 4) : 0.f;
    int rc;
    if ((rc = norm_all(r.ln1, r.ln1_dtype, x, b.ln1_w, b.ln1_b, sc1))) return rc;
    Product p = product(b, 0, r.in_proj, rows());
    p.a_scale = r.in_proj.kernel == ACX_TF_GEMM_X6 ? sc1 : 0.f;
    p.A = r.in_proj.kernel == ACX_TF_GEMM_X6 ? ws.hp : ws.h;
    p.C = planes(r.in_proj) ? ws.qkv3 : ws.qkv;
    if (s_qkv > 0.f) {           // the two fp16 planes of s_qkv * (q | k | v) where the f32 rows would go: the same bytes; no K split, no scratch
      p.C = ws.qkv; p.c_scale = s_qkv;
      p.scratch = nullptr; p.scratch_bytes = 0;
    }
    if ((rc = go(p))) return rc;
    switch (r.att) {
      case ACX_TF_ATT_BF16: rc = acx_attention_bf16(ctx, ws.qkv, 3 * W, ws.att, W, batch, L, heads, s); break;
      case ACX_TF_ATT_P3F:                                                                                               // f32 rows in, planes out
        rc = s_att > 0.f ? acx_attention_p3f16(ctx, (const float*)ws.qkv, 3 * W, ws.hp, s_att, batch, L, heads, s)
                         : acx_attention_p3f(ctx, (const float*)ws.qkv, 3 * W, ws.hp, batch, L, heads, s);
        break;
      case ACX_TF_ATT_P3N:                                                                                               // planes in, planes out
        rc = s_qkv > 0.f ? acx_attention_p3h16(ctx, ws.qkv, s_qkv, ws.hp, s_att, batch, L, heads, s)
                         : acx_attention_p3n(ctx, ws.qkv3, ws.hp, batch, L, heads, r.att_products, s);
        break;
      case ACX_TF_ATT_S16: rc = acx_attention_s16(ctx, ws.qkv3, 1.f, ws.hp, 1.f, batch, L, heads, s); break;                  // fp16 planes in, fp16 planes out
      case ACX_TF_ATT_X3_PANEL: rc = acx_attention_x3_panel(ctx, (const float*)ws.qkv, 3 * W, ws.hp, W, batch, L, heads, s); break;
      case ACX_TF_ATT_HD_X3_PANEL: rc = acx_attention_x3_hd(ctx, (const float*)ws.qkv, 3 * W, ws.hp, W, batch, L, heads, W / heads, 1, s); break;
      case ACX_TF_ATT_HD_F32: rc = acx_attention_hd(ctx, (const float*)ws.qkv, 3 * W, (float*)ws.att, W, batch, L, heads, W / heads, s); break;
      default: rc = acx_attention(ctx, (const float*)ws.qkv, 3 * W, (float*)ws.att, W, batch, L, heads, g.causal, s); break;
    }
    if (rc) return rc;
    if (r.split_att && (rc = acx_split_bf16x3_panel(ctx, (const float*)ws.att, W, ws.hp, rows() * W * 2, rows(), W, s))) return rc;
    // ws.hp: out-proj's A planes AND ln_2's output -- disjoint rows, acx_gemm_ln.  ACX_PREC_F32X6_R16 (s_att > 0): A is TWO fp16 planes
    // with the geometry of the two ln_2 writes (plane = [W / 32][rows][32] u16, N == K), so a rider's plane row r is exactly A's plane row
    // r: the riders write rows below `ride` <= the rows the full rounds completed, the tiles of the last round read rows at or above
    // them, and the full rounds -- which read every row -- are an earlier launch on the same stream.  The argument never used the
    // planes' number format or count, only that row r of y and row r of A are the same bytes.
    const acx_ln_job ln2 = job(b.ln2_w, b.ln2_b, sc2);
    p = product(b, 1, r.out_proj, rows());
    p.a_scale = r.out_proj.kernel == ACX_TF_GEMM_X6 ? s_att : 0.f;
    p.A = r.out_proj.kernel == ACX_TF_GEMM_X6 ? ws.hp : ws.att;
    p.a_dtype = r.att == ACX_TF_ATT_BF16 ? ACX_BF16 : ACX_F32;
    p.C = x; p.residual = x;
    p.ln = r.out_proj.ln_job ? &ln2 : nullptr;
    if ((rc = go(p))) return rc;
    if ((rc = norm_all(r.ln2, r.ln2_dtype, x, b.ln2_w, b.ln2_b, sc2))) return rc;
    p = product(b, 2, r.fc, rows());
    p.a_scale = r.fc.kernel == ACX_TF_GEMM_X6 ? sc2 : 0.f;
    p.c_scale = s_hid;
    p.A = r.fc.kernel == ACX_TF_GEMM_X6 ? ws.hp : ws.h;
    p.C = planes(r.fc) ? ws.mp : ws.mlp;
    if ((rc = go(p))) return rc;
    if (r.split_mlp && (rc = acx_split_bf16x3_panel(ctx, (const float*)ws.mlp, 4 * W, ws.mp, rows() * 4 * W * 2, rows(), 4 * W, s))) return rc;
    const acx_ln_job ln1 = r.proj.ln_job ? job(next->ln1_w, next->ln1_b, lnsc(next_ln1_dtype, l + 1, 0)) : job(nullptr, nullptr);
    p = product(b, 3, r.proj, rows());
    p.a_scale = r.proj.kernel == ACX_TF_GEMM_X6 ? s_hid : 0.f;
    p.A = r.proj.kernel == ACX_TF_GEMM_X6 ? ws.mp : ws.mlp;
    p.C = x; p.residual = x;
    p.ln = r.proj.ln_job ? &ln1 : nullptr;
    return go(p);
  }

  // the final residual stream of the CLS tokens is left COMPACT in c.xc instead of x
  int pruned(const acx_tf_layer_plan_t& r, const acx_block_weights& b, const float* x, const ClsWs& c, int l) const {
    const int W = g.W, batch = g.batch, L = g.L;
    const float sc1 = lnsc(r.ln1_dtype, l, 0);     // (the K | V product on the plane kernel reads the in-projection's fp16 planes)
    int rc;
    Product p = product(b, 0, r.in_proj, rows());
    if (r.att == ACX_TF_ATT_CLS_FOLD) {
      // ln_1 and Q for the CLS rows (hc and mc are free until ln_2 / c_fc), then the folded attention over the rows of x
      if ((rc = norm(x, (int64_t)L * W, b.ln1_w, b.ln1_b, c.hc, W, r.ln1_dtype, batch))) return rc;
      p.M = batch; p.N = W;
      p.A = c.hc;
      p.C = c.mc; p.ldc = W;
      if ((rc = go(p))) return rc;
      if ((rc = acx_attention_cls_fold(ctx, x, b.ln1_w, b.ln1_b, 1e-5f, b.in_proj_w, b.in_proj_b, (const float*)c.mc, W, c.attc, W, batch, L, W,
                                       g.heads, ws.qkv, (size_t)rows() * 3 * W * 4, s))) return rc;
    } else {
      // K | V for every token: rows [W, 3W) of in_proj.  On the plane kernel LayerNorm writes the product's planes (all rows) and the
      // f32 rows of the CLS tokens (Q below reads only those)
      if ((rc = norm_all(r.ln1, r.ln1_dtype, x, b.ln1_w, b.ln1_b, sc1))) return rc;
      p.N = 2 * W; p.bias = b.in_proj_b + W;
      p.C = (float*)ws.qkv + W; p.ldc = 3 * W;
      if (r.in_proj.kernel == ACX_TF_GEMM_X6) {
        if ((rc = norm(x, (int64_t)L * W, b.ln1_w, b.ln1_b, ws.h, (int64_t)L * W, m.hdt, batch))) return rc;
        p.A = ws.hp; p.a_scale = sc1;
        p.Wb = (const char*)b.in_proj_w_bf16 + (size_t)W * 64;   // row W of every K-panel
        p.w_plane_bytes = (int64_t)3 * W * W * 2;
      } else {
        p.A = ws.h;
        p.Wf = b.in_proj_w + (size_t)W * W;
        p.Wb = b.in_proj_w_bf16 ? (const char*)b.in_proj_w_bf16 + (size_t)W * W * 2 : nullptr;
      }
      if ((rc = go(p))) return rc;
      // Q for the CLS rows only (A rows strided by one sequence)
      Product q = product(b, 0, tf_rows(ACX_F32, ACX_TF_BUF_NONE), batch);
      q.N = W;
      q.A = ws.h; q.lda = L * W;
      q.C = ws.qkv; q.ldc = L * 3 * W;
      if ((rc = go(q))) return rc;
      if ((rc = r.att == ACX_TF_ATT_HD_CLS ? acx_attention_cls_hd(ctx, (const float*)ws.qkv, 3 * W, c.attc, W, batch, L, g.heads, W / g.heads, s)
                                           : acx_attention_cls(ctx, (const float*)ws.qkv, 3 * W, c.attc, W, batch, L, g.heads, s))) return rc;
    }
    p = product(b, 1, r.out_proj, batch);
    p.A = c.attc; p.a_dtype = ACX_F32;
    p.C = c.x1; p.residual = x; p.ldr = L * W;
    if ((rc = go(p))) return rc;
    if ((rc = norm(c.x1, W, b.ln2_w, b.ln2_b, c.hc, W, r.ln2_dtype, batch))) return rc;
    p = product(b, 2, r.fc, batch);
    p.A = c.hc;
    p.C = c.mc;
    if ((rc = go(p))) return rc;
    p = product(b, 3, r.proj, batch);
    p.A = c.mc;
    p.C = c.xc; p.residual = c.x1;
    return go(p);
  }
};

int transformer_layers(acx_ctx* ctx, float* x, const TfGeom& g, const TfPlan& plan, const acx_block_weights* blk, const TfWs& ws,
                       hipStream_t s, float* cls_ws = nullptr, const float* ln_scales = nullptr) {
  if (g.prec == ACX_PREC_F32X6_LN16) {
    if (!ln_scales) return acx_fail(ctx, ACX_E_BADARG, "driver: ACX_PREC_F32X6_LN16 needs the LayerNorm plane scales (acx_vit_encode_ln16)%s");
    for (int i = 0; i < 2 * g.layers; ++i) {
      int e = 0;
      const float sc = ln_scales[i];
      if (!(sc >= 0x1p-20f && sc <= 0x1p20f) || frexpf(sc, &e) != 0.5f)
        return acx_fail(ctx, ACX_E_BADARG, "driver: ACX_PREC_F32X6_LN16: a LayerNorm plane scale is not a power of two in [2^-20, 2^20]%s");
    }
  }
  if (is_r16(g.prec)) {
    const bool q = g.prec == ACX_PREC_F32X6_QKV16;
    if (!ln_scales)
      return acx_fail(ctx, ACX_E_BADARG, q ? "driver: ACX_PREC_F32X6_QKV16 needs the plane scales (acx_vit_encode_qkv16)%s"
                                           : "driver: ACX_PREC_F32X6_R16 needs the plane scales (acx_vit_encode_r16)%s");
    for (int i = 0; i < scales_per_layer(g.prec) * g.layers; ++i) {
      int e = 0;
      const float sc = ln_scales[i];
      if (!(sc >= 0x1p-20f && sc <= 0x1p20f) || frexpf(sc, &e) != 0.5f)
        return acx_fail(ctx, ACX_E_BADARG, "driver: %s: a plane scale is not a power of two in [2^-20, 2^20]", ln16_name(g.prec));
    }
  }
  const TfRun exec = {ctx, g, plan.mode, ws, s, ln_scales};
  for (int l = 0; l < g.layers; ++l) {
    const acx_tf_layer_plan_t r = tf_layer(plan, l, g.layers);
    const int next_ln1 = l + 1 < g.layers ? tf_layer(plan, l + 1, g.layers).ln1_dtype : 0;
    const int rc = r.pruned ? exec.pruned(r, blk[l], x, carve_cls(cls_ws, g.batch, g.W), l)
                            : exec.body(r, blk[l], l + 1 < g.layers ? &blk[l + 1] : nullptr, x, l, next_ln1);
    if (rc) return rc;
  }
  return ACX_OK;
}

}  // namespace

extern "C" size_t acx_transformer_workspace_bytes(int32_t width, int32_t rows) {
  return carve_tf(nullptr, rows, width).total;
}
extern "C" size_t acx_transformer_workspace_bytes_prec(int32_t width, int32_t rows, int32_t prec) {
  return carve_tf(nullptr, rows, width, prec).total;
}

extern "C" int acx_transformer_plan(const acx_ctx* ctx, int32_t batch, int32_t L, int32_t width, int32_t heads, int32_t layers,
                                    int32_t causal, int32_t prec, int32_t prune_last, int32_t has_weight_planes,
                                    int32_t workspace_is_prec_sized, acx_tf_layer_plan_t* out) {
  acx_ctx* err = const_cast<acx_ctx*>(ctx);      // (the refusal's text)
  if (!out || batch <= 0 || L <= 0 || layers < 0) return acx_fail(err, ACX_E_BADARG, "acx_transformer_plan: no result array or an empty geometry%s");
  memset(out, 0, sizeof(*out) * layers);
  const TfGeom g = {batch, L, width, heads, layers, causal, prec, prune_last != 0, is_xmode(prec) && workspace_is_prec_sized, ACX_ACT_QUICKGELU};
  const bool alt = has_weight_planes != 0;
  const TfHave have = {{true, true, true, true}, {alt, alt, alt, alt}};
  TfPlan plan;
  const int rc = tf_plan(err, g, have, tf_opts(ctx, true), &plan);
  for (int l = 0; !rc && l < layers; ++l) out[l] = tf_layer(plan, l, layers);
  return rc;
}

extern "C" int acx_transformer_forward(acx_ctx* ctx, float* x, int32_t batch, int32_t L, int32_t width, int32_t heads,
                                       int32_t layers, int32_t causal, int32_t prec, const acx_block_weights* blocks,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  return acx_transformer_forward_act(ctx, x, batch, L, width, heads, layers, causal, prec, ACX_ACT_QUICKGELU, blocks, workspace, workspace_bytes, stream);
}

extern "C" int acx_transformer_forward_act(acx_ctx* ctx, float* x, int32_t batch, int32_t L, int32_t width, int32_t heads,
                                           int32_t layers, int32_t causal, int32_t prec, int32_t act, const acx_block_weights* blocks,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !blocks || !workspace) return acx_fail(ctx, ACX_E_BADARG, "acx_transformer_forward: null pointer%s");
  int mlp_act = 0, rc0;
  if ((rc0 = tf_act(ctx, "acx_transformer_forward", act, prec, &mlp_act))) return rc0;
  if (tf_head_dim(width, heads) != 64 && !(tf_head_dim(width, heads) == 80 && !causal))
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_transformer_forward: head dim must be 64 (or 80, non-causal)%s");
  // ACX_PREC_F32X6 with a workspace sized for it (acx_transformer_workspace_bytes_prec); a smaller (f32-sized) workspace runs
  // the f32 kernels
  TfWs ws = carve_tf((char*)workspace, (int64_t)batch * L, width, prec);
  if (ws.total > workspace_bytes && is_xmode(prec)) ws = carve_tf((char*)workspace, (int64_t)batch * L, width);
  if (ws.total > workspace_bytes) return acx_fail(ctx, ACX_E_WORKSPACE, "acx_transformer_forward: workspace too small%s");
  const TfGeom g = {batch, L, width, heads, layers, causal, prec, false, ws.hp != nullptr, mlp_act};
  TfPlan plan;
  const int rc = tf_plan_call(ctx, g, blocks, &plan);
  return rc ? rc : transformer_layers(ctx, x, g, plan, blocks, ws, (hipStream_t)stream);
}

namespace {
struct VitWs {
  char *patches, *patch_out, *x, *cls, *cls_ws;
  size_t tf_off, total;
};
VitWs carve_vit(char* base, const acx_vit_desc* d, int F) {
  const int g = d->resolution / d->patch, T = g * g, W = d->width;
  const int K = 3 * d->patch * d->patch;
  VitWs w;
  size_t off = 0;
  w.patches = base + off;   off += al((size_t)F * T * K * (is_xmode(d->prec) ? 6 : 4));   // (plane modes: three bf16 planes)
  w.patch_out = base + off; off += al((size_t)F * T * W * 4);
  w.x = base + off;         off += al((size_t)F * (T + 1) * W * 4);
  w.cls = base + off;       off += al((size_t)F * W * 4);
  w.cls_ws = base + off;    off += al(cls_ws_bytes(F, W));
  w.tf_off = off;
  off += carve_tf(nullptr, (int64_t)F * (T + 1), W, d->prec).total;
  w.total = off;
  return w;
}
}  // namespace

extern "C" size_t acx_vit_workspace_bytes(const acx_vit_desc* d, int32_t frames) {
  if (!d || frames <= 0) return 0;
  return carve_vit(nullptr, d, frames).total;
}

static int vit_encode(acx_ctx* ctx, const acx_vit_desc* d, const acx_vit_weights* w, const float* ln_scales, const float* frames,
                      int32_t nframes, float* features, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !w || !frames || !features || !workspace) return acx_fail(ctx, ACX_E_BADARG, "acx_vit_encode: null pointer%s");
  if (d->prec == ACX_PREC_F32X6_LN16 && !ln_scales)
    return acx_fail(ctx, ACX_E_BADARG, "acx_vit_encode: ACX_PREC_F32X6_LN16 needs the LayerNorm plane scales (acx_vit_encode_ln16)%s");
  if (d->prec == ACX_PREC_F32X6_R16 && !ln_scales)
    return acx_fail(ctx, ACX_E_BADARG, "acx_vit_encode: ACX_PREC_F32X6_R16 needs the plane scales (acx_vit_encode_r16)%s");
  if (d->prec == ACX_PREC_F32X6_QKV16 && !ln_scales)
    return acx_fail(ctx, ACX_E_BADARG, "acx_vit_encode: ACX_PREC_F32X6_QKV16 needs the plane scales (acx_vit_encode_qkv16)%s");
  int mlp_act = 0, rc0;
  if ((rc0 = tf_act(ctx, "acx_vit_encode", d->act, d->prec, &mlp_act))) return rc0;
  if (nframes <= 0) return ACX_OK;
  if (!tf_head_dim(d->width, d->heads)) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_vit_encode: head dim must be 64 or 80%s");
  if (d->patch <= 0 || d->resolution % d->patch || d->patch % 2)
    return acx_fail(ctx, ACX_E_BADARG, "acx_vit_encode: bad patch geometry (need resolution %% patch == 0 and an even patch)%s");
  const int g = d->resolution / d->patch, T = g * g, W = d->width, F = nframes;
  const int K = 3 * d->patch * d->patch;
  if (T + 1 > 1024)
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_vit_encode: %s%ld tokens per frame, the attention kernels take at most 1024", "", (long)(T + 1));
  const VitWs ws = carve_vit((char*)workspace, d, F);
  if (ws.total > workspace_bytes) return acx_fail(ctx, ACX_E_WORKSPACE, "acx_vit_encode: workspace too small%s");
  hipStream_t s = (hipStream_t)stream;
  const TfWs tf = carve_tf((char*)workspace + ws.tf_off, (int64_t)F * (T + 1), W, d->prec);
  const bool prune = ACX_DBG_SWITCH("VIT_PRUNE", true);
  const TfGeom geom = {F, T + 1, W, d->heads, d->layers, 0, d->prec, prune, tf.hp != nullptr, mlp_act};
  TfPlan plan;
  int rc;
  if ((rc = tf_plan_call(ctx, geom, w->blocks, &plan))) return rc;
  const TfMode& m = plan.mode;                   // final projection (and small launches): f32 kernels in the plane modes
  // conv1 as GEMM over im2col'ed patches                               clip/model.py:267-269
  Product p;
  memset(&p, 0, sizeof(p));
  p.A = ws.patches; p.lda = K;
  p.Wf = w->conv1_w; p.Wb = w->conv1_w_bf16; p.ldw = K;
  p.M = F * T; p.N = W; p.K = K;
  p.C = ws.patch_out; p.c_dtype = ACX_F32; p.ldc = W;
  if (is_xmode(d->prec) && w->conv1_w_bf16 && K % 32 == 0 && x6_takes(tf_opts(ctx, false), tf.hp != nullptr, (int64_t)F * T, W, K, K)) {
    // plane modes: im2col writes the planes of the pixels (K-panel layout), the embedding is a plane product like the layers' GEMMs
    // (conv1_w_bf16: the weight's K-panel planes); scratch for a K-split tail: the f32 q | k | v buffer
    p.kernel = ACX_TF_GEMM_X6;
    p.a_dtype = m.pdt;
    p.scratch = tf.qkv; p.scratch_bytes = (size_t)F * (T + 1) * 3 * W * 4;
  } else {
    // a patch of 14 (K = 588: not a multiple of the bf16 kernels' 8) embeds on the f32 kernels in every mode: ~0.2 % of the MACs
    p.kernel = ACX_TF_GEMM_ROWS;
    p.a_dtype = d->patch % 4 ? ACX_F32 : m.hdt;
  }
  if ((rc = acx_vit_patches(ctx, frames, ws.patches, p.a_dtype, F, d->resolution, d->patch, s))) return rc;
  if ((rc = p.kernel == ACX_TF_GEMM_X6 ? run_x6(ctx, m.xm, p, s) : run_rows(ctx, p.a_dtype == ACX_BF16 ? ACX_PREC_BF16 : ACX_PREC_F32, p, s))) return rc;
  // CLS + positional embedding + ln_pre                                :270-279
  if ((rc = acx_vit_embed(ctx, (const float*)ws.patch_out, w->class_embedding, w->positional_embedding, w->ln_pre_w,
                          w->ln_pre_b, (float*)ws.x, F, T, W, s))) return rc;
  if ((rc = transformer_layers(ctx, (float*)ws.x, geom, plan, w->blocks, tf, s, (float*)ws.cls_ws, ln_scales))) return rc;
  // ln_post on the CLS rows, then @ proj                                :285-288
  if ((rc = acx_layernorm(ctx, prune ? (const float*)ws.cls_ws : (const float*)ws.x, prune ? (int64_t)W : (int64_t)(T + 1) * W,
                          w->ln_post_w, w->ln_post_b, ws.cls, W, ACX_F32, F, W, 1e-5f, ACX_NORM_LAYER, s))) return rc;
  memset(&p, 0, sizeof(p));
  p.A = ws.cls; p.a_dtype = ACX_F32; p.lda = W;
  p.Wf = w->proj_t; p.Wb = w->proj_t_bf16; p.ldw = W;
  p.M = F; p.N = d->embed_dim; p.K = W;
  p.C = features; p.c_dtype = ACX_F32; p.ldc = d->embed_dim;
  return run_rows(ctx, m.prec, p, s);
}


extern "C" int acx_vit_encode(acx_ctx* ctx, const acx_vit_desc* d, const acx_vit_weights* w, const float* frames,
                              int32_t nframes, float* features, void* workspace, size_t workspace_bytes, void* stream) {
  return vit_encode(ctx, d, w, nullptr, frames, nframes, features, workspace, workspace_bytes, stream);
}

extern "C" int acx_vit_encode_ln16(acx_ctx* ctx, const acx_vit_desc* d, const acx_vit_weights* w, const float* ln_scales, const float* frames,
                                   int32_t nframes, float* features, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || d->prec != ACX_PREC_F32X6_LN16 || !ln_scales)
    return acx_fail(ctx, ACX_E_BADARG, "acx_vit_encode_ln16: needs desc->prec = ACX_PREC_F32X6_LN16 and the LayerNorm plane scales%s");
  return vit_encode(ctx, d, w, ln_scales, frames, nframes, features, workspace, workspace_bytes, stream);
}

extern "C" int acx_vit_encode_r16(acx_ctx* ctx, const acx_vit_desc* d, const acx_vit_weights* w, const float* scales, const float* frames,
                                  int32_t nframes, float* features, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || d->prec != ACX_PREC_F32X6_R16 || !scales)
    return acx_fail(ctx, ACX_E_BADARG, "acx_vit_encode_r16: needs desc->prec = ACX_PREC_F32X6_R16 and the plane scales%s");
  return vit_encode(ctx, d, w, scales, frames, nframes, features, workspace, workspace_bytes, stream);
}

extern "C" int acx_vit_encode_qkv16(acx_ctx* ctx, const acx_vit_desc* d, const acx_vit_weights* w, const float* scales, const float* frames,
                                    int32_t nframes, float* features, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || d->prec != ACX_PREC_F32X6_QKV16 || !scales)
    return acx_fail(ctx, ACX_E_BADARG, "acx_vit_encode_qkv16: needs desc->prec = ACX_PREC_F32X6_QKV16 and the plane scales%s");
  return vit_encode(ctx, d, w, scales, frames, nframes, features, workspace, workspace_bytes, stream);
}
