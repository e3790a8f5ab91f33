// acx_attention* -- multi-head attention for head dim 64: the CLIP vision transformers (non-causal, L = 197 for ViT-B/16, up to
// 1024) and the CLIP text transformer (L = 77, causal).  Replaces the core of nn.MultiheadAttention as called from
// clip/model.py:206-212; the reference materialises (batch*heads, L, L) score tensors in HBM, here scores never leave registers.
//
// One header per kernel family, included below; this file holds the C entry points: argument checks, kernel choice, launches.
#include "acx_internal.h"

#include <stdlib.h>

namespace {
#include "acx_attn_f32.h"    // attn_kernel, attn16_kernel: f32 MFMAs
#include "acx_attn_p3.h"     // attn_p3_kernel: bf16 / fp16 operand planes (or f32 rows split in the kernel), f32-accurate products
#include "acx_attn_s16.h"    // attn_s16_kernel: two fp16 planes per operand, streaming over the keys (any L <= 1024)
#include "acx_attn_bf16.h"   // attn_bf16_kernel: bf16 operands, the bf16 mode of the ViT
#include "acx_attn_cls.h"    // attn_cls_kernel, cls_fold_u_kernel, cls_fold_kernel, cls_fold_o_kernel: the CLS row only
#include "acx_attn_hd.h"     // attn_hd_kernel, attn_cls_hd_kernel: f32 MFMAs at head dimension 80
}  // namespace

// The kernel choice of acx_attention / _x3 / _x3_panel: one rule, asked by the dispatcher below and by acx_attention_route.  *why: the
// refusal's message; *late: the refusal comes after the argument checks of attention_impl (it depends on out, not on the shape alone)
static int attn_route(const acx_ctx* ctx, int32_t L, int32_t causal, int32_t out_aligned, const char** why, bool* late) {
  *late = false;
  *why = "acx_attention: need 0 < L <= 224 (causal) or 0 < L <= 1024 (non-causal)%s";
  if (L <= 0 || L > (causal ? 224 : 1024)) return ACX_E_UNSUPPORTED;
  // Calls without a context keep the answer the ABI gave before sequences above 224 were supported (ACX_E_UNSUPPORTED, checked
  // before any launch: tests/test_cpu_host.py pins it with a NULL context and a host buffer).  Nothing in the kernel needs the
  // context -- it falls back to 256 CUs below -- this only keeps that earlier contract for context-free callers.
  *why = "acx_attention: L > 224 needs a context%s";
  if (L > 224 && !ctx) return ACX_E_UNSUPPORTED;
  if (!causal && L > 128 && out_aligned && (L > 224 || ACX_DBG_SWITCH("ATTN16", true)))
    return L > 256 ? ACX_ATTN_ROUTE_STREAM16_QB : ACX_ATTN_ROUTE_STREAM16;
  *late = true;
  *why = "acx_attention: L > 224 needs the streaming kernel (out 16-byte aligned, ldo %% 4 == 0)%s";
  if (L > 224) return ACX_E_UNSUPPORTED;
  return ACX_ATTN_ROUTE_BLOCK32;
}

extern "C" int acx_attention_route(const acx_ctx* ctx, int32_t L, int32_t causal, int32_t out_aligned) {
  const char* why;
  bool late;
  return attn_route(ctx, L, causal, out_aligned, &why, &late);
}

static int attention_impl(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo,
                          int32_t batch, int32_t L, int32_t heads, int32_t causal, void* stream, int x3) {
  if (!qkv || !out) return acx_fail(ctx, ACX_E_BADARG, "acx_attention: null pointer%s");
  if (batch <= 0) return ACX_OK;
  const char* why;
  bool late;
  const int route = attn_route(ctx, L, causal, ldo % 4 == 0 && !((uintptr_t)out & 15), &why, &late);
  if (heads <= 0) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention: need 0 < L <= 224 (causal) or 0 < L <= 1024 (non-causal)%s");
  if (route < 0 && !late) return acx_fail(ctx, route, why);
  if (ldqkv % 4 || ((uintptr_t)qkv & 15)) return acx_fail(ctx, ACX_E_BADARG, "acx_attention: qkv must be 16-byte aligned, ld%%4==0%s");
  const int nt = (L + 31) / 32;
  const bool nw4 = ACX_DBG_SWITCH("ATTN_NW4", false);
  const dim3 grid((unsigned)(batch * heads));
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_ATTN, (hipStream_t)stream);
  if (route == ACX_ATTN_ROUTE_STREAM16 || route == ACX_ATTN_ROUTE_STREAM16_QB) {
    // ViT sequence: 16-wide tiles (one or two query tiles per wave), chunked LDS-DMA staging, two workgroups per CU;
    // L > 256: several query blocks per (sequence, head)
    const int nqb = route == ACX_ATTN_ROUTE_STREAM16_QB ? ((L + 15) / 16 + 15) / 16 : 1;
    const int nitems = batch * heads * nqb;
    const int ncu = ctx && ctx->multiprocessors > 0 ? ctx->multiprocessors : 256;
    const int slots = 2 * ncu;                                            // two workgroups per CU
    const dim3 grid16((unsigned)(nitems < slots ? nitems : slots));
    const int64_t x3plane = x3 ? (int64_t)batch * L * ldo : (int64_t)0, prows = x3 == 2 ? (int64_t)batch * L : (int64_t)0;
    if (nqb == 1)
      hipLaunchKernelGGL(attn16_kernel<false>, grid16, dim3(512), 2 * A16_STAGE_B, s, qkv, ldqkv, out, ldo, L, heads, nitems, x3plane, prows);
    else
      hipLaunchKernelGGL(attn16_kernel<true>, grid16, dim3(512), 2 * A16_STAGE_B, s, qkv, ldqkv, out, ldo, L, heads, nitems, x3plane, prows);
    ACX_CHECK_LAUNCH(ctx, "acx_attention");
    return ACX_OK;
  }
  if (x3) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_x3: the ViT kernel only (non-causal, 128 < L <= 1024, out 16-byte aligned)%s");
  if (route != ACX_ATTN_ROUTE_BLOCK32) return acx_fail(ctx, route, why);
  const int dev_slot = (ctx ? ctx->device : 0) & 63;
#define ACX_ATTN(NT, NW)                                                                           \
  acx_launch_lds<attn_kernel<NT, NW>>(dev_slot, grid, dim3(NW * 64), (size_t)NT * 32 * (KROW + VROW) * 4 + NW * 32 * 4 + 16, s, \
                                      qkv, ldqkv, out, ldo, L, heads, causal)
  switch (nt) {
    // one wave per 32-query block where it fits; >4 blocks -> 8 waves (2 per SIMD: one wave's softmax and
    // LDS phases overlap the other's MFMAs)
    case 1: ACX_ATTN(1, 4); break;
    case 2: ACX_ATTN(2, 4); break;
    case 3: ACX_ATTN(3, 4); break;
    case 4: ACX_ATTN(4, 4); break;
    case 5: ACX_ATTN(5, 8); break;
    case 6: ACX_ATTN(6, 8); break;
    default:
      if (nw4) ACX_ATTN(7, 4); else ACX_ATTN(7, 8);
      break;
  }
#undef ACX_ATTN
  ACX_CHECK_LAUNCH(ctx, "acx_attention");
  return ACX_OK;
}

extern "C" int acx_attention(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo,
                             int32_t batch, int32_t L, int32_t heads, int32_t causal, void* stream) {
  return attention_impl(ctx, qkv, ldqkv, out, ldo, batch, L, heads, causal, stream, 0);
}

// The launch of attn_p3_kernel for acx_attention_p3n (form 6 / 3: products on bf16 planes, 103: three products on fp16 planes) and
// acx_attention_p3f (form 0: `src` is the f32 matrix, ldqkv its leading dimension; form 16: acx_attention_p3f16, the same with the two
// fp16 planes of oscale * o out; form 116: acx_attention_p3h16, form 103 on scaled planes with a scaled output): persistent, one
// workgroup per CU; `name` is the entry point's, for the launch check
static int ap3_launch(acx_ctx* ctx, int form, const void* src, int64_t ldqkv, void* out_planes, int32_t batch, int32_t L, int32_t heads,
                      void* stream, const char* name, float oscale = 1.f, float sscale = 1.f) {
  const int64_t rows = (int64_t)batch * L;
  const int nitems = batch * heads;
  const int ncu = ctx && ctx->multiprocessors > 0 ? ctx->multiprocessors : 256;
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_ATTN, s);
  const int dev_slot = (ctx ? ctx->device : 0) & 63;
#if AP3_TRACE
  long long* trace_ = getenv("ACX_TRACE_PTR") ? (long long*)strtoull(getenv("ACX_TRACE_PTR"), nullptr, 0) : nullptr;
#else
  long long* trace_ = nullptr;
#endif
  const dim3 grid((unsigned)(nitems < ncu ? nitems : ncu));
#define ACX_AP3(LD, ...)                                                                                                        \
  acx_launch_lds<attn_p3_kernel<__VA_ARGS__>>(dev_slot, grid, dim3(512), (size_t)AP3_LDS_B, s, (const u16*)src, (int64_t)(LD), rows, \
                                              (u16*)out_planes, rows * heads * 64, L, heads, nitems, trace_)
  if (form == 103) ACX_AP3(rows * 3 * heads * 64, 3, 1);
  else if (form == 3) ACX_AP3(rows * 3 * heads * 64, 3);
  else if (form == 6) ACX_AP3(rows * 3 * heads * 64, 6);
  else if (form == 16)
    acx_launch_lds<attn_p3_o16_kernel>(dev_slot, grid, dim3(512), (size_t)AP3_LDS_B, s, (const u16*)src, ldqkv, rows, (u16*)out_planes,
                                       rows * heads * 64, L, heads, nitems, trace_, oscale);
  else if (form == 116)
    acx_launch_lds<attn_p3_h16_kernel>(dev_slot, grid, dim3(512), (size_t)AP3_LDS_B, s, (const u16*)src, rows * 3 * heads * 64, rows,
                                       (u16*)out_planes, rows * heads * 64, L, heads, nitems, trace_, oscale, sscale);
  else ACX_AP3(ldqkv, 6, 0, 1);
#undef ACX_AP3
  ACX_CHECK_LAUNCH(ctx, name);
  return ACX_OK;
}

// q | k | v as three bf16 planes in K-panel layout (ACX_BF16X3P of the [batch * L, 3 heads * 64] in-projection output) ->
// attention output as three bf16 planes in K-panel layout ([heads * 64 / 32][batch * L][32]); 128 < L <= 208, non-causal
extern "C" int acx_attention_p3(acx_ctx* ctx, const void* qkv_planes, void* out_planes, int32_t batch, int32_t L, int32_t heads,
                                void* stream) {
  return acx_attention_p3n(ctx, qkv_planes, out_planes, batch, L, heads, 6, stream);
}
// products = 6: the f32-accurate form; 3: the three leading products of both contractions (ACX_PREC_F32X3: the lo planes of the
// operands are not read, the output's lo plane is not written)
extern "C" int acx_attention_p3n(acx_ctx* ctx, const void* qkv_planes, void* out_planes, int32_t batch, int32_t L, int32_t heads,
                                 int32_t products, void* stream) {
  if (!qkv_planes || !out_planes) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_p3: null pointer%s");
  const bool f16 = products == 103;                     // 103: three products on TWO fp16 planes (ACX_PREC_F16X3)
  if (f16) products = 3;
  if (products != 6 && products != 3) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_p3n: products must be 6, 3 or 103 (3 on fp16 planes)%s");
  if (batch <= 0) return ACX_OK;
  if (L <= 192 || L > AP3_ROWS || heads <= 0 || (((uintptr_t)qkv_planes | (uintptr_t)out_planes) & 15))
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_p3: 192 < L <= 208, 16-byte aligned planes%s");
  return ap3_launch(ctx, f16 ? 103 : products, qkv_planes, 0, out_planes, batch, L, heads, stream, "acx_attention_p3");
}

// the six-product form fed with the in-projection's f32 rows: qkv [batch * L, 3 heads * 64] f32 (leading dimension ldqkv) -> the same
// three output planes, bit for bit what acx_attention_p3 gives on acx_split_bf16x3_panel(qkv); same L gate
extern "C" int acx_attention_p3f(acx_ctx* ctx, const float* qkv, int64_t ldqkv, void* out_planes, int32_t batch, int32_t L, int32_t heads,
                                 void* stream) {
  if (!qkv || !out_planes) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_p3f: null pointer%s");
  if (batch <= 0) return ACX_OK;
  if (L <= 192 || L > AP3_ROWS || heads <= 0 || ldqkv < (int64_t)3 * heads * 64 || (ldqkv & 3) || (((uintptr_t)qkv | (uintptr_t)out_planes) & 15))
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_p3f: 192 < L <= 208, 16-byte aligned qkv and planes, ldqkv %% 4 == 0 and >= 3 heads * 64%s");
  return ap3_launch(ctx, 0, qkv, ldqkv, out_planes, batch, L, heads, stream, "acx_attention_p3f");
}

// ... with the epilogue writing the two fp16 planes of out_scale * o (ACX_F16X2P): the out-projection's A operand in ACX_PREC_F32X6_R16
extern "C" int acx_attention_p3f16(acx_ctx* ctx, const float* qkv, int64_t ldqkv, void* out_planes, float out_scale, int32_t batch, int32_t L,
                                   int32_t heads, void* stream) {
  if (!qkv || !out_planes) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_p3f16: null pointer%s");
  int e = 0;
  if (!(out_scale >= 0x1p-20f && out_scale <= 0x1p20f) || frexpf(out_scale, &e) != 0.5f)
    return acx_fail(ctx, ACX_E_BADARG, "acx_attention_p3f16: out_scale must be a power of two in [2^-20, 2^20]%s");
  if (batch <= 0) return ACX_OK;
  if (L <= 192 || L > AP3_ROWS || heads <= 0 || ldqkv < (int64_t)3 * heads * 64 || (ldqkv & 3) || (((uintptr_t)qkv | (uintptr_t)out_planes) & 15))
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_p3f16: 192 < L <= 208, 16-byte aligned qkv and planes, ldqkv %% 4 == 0 and >= 3 heads * 64%s");
  return ap3_launch(ctx, 16, qkv, ldqkv, out_planes, batch, L, heads, stream, "acx_attention_p3f16", out_scale);
}

// the fp16 planes form (acx_attention_p3n, products = 103) on the planes of in_scale * (q | k | v), writing those of out_scale * o: the
// attention of ACX_PREC_F32X6_QKV16 between an in-projection and an out-projection that both run on fp16 planes
extern "C" int acx_attention_p3h16(acx_ctx* ctx, const void* qkv_planes, float in_scale, void* out_planes, float out_scale, int32_t batch,
                                   int32_t L, int32_t heads, void* stream) {
  if (!qkv_planes || !out_planes) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_p3h16: null pointer%s");
  int e = 0;
  if (!(in_scale >= 0x1p-20f && in_scale <= 0x1p20f) || frexpf(in_scale, &e) != 0.5f || !(out_scale >= 0x1p-20f && out_scale <= 0x1p20f) ||
      frexpf(out_scale, &e) != 0.5f)
    return acx_fail(ctx, ACX_E_BADARG, "acx_attention_p3h16: in_scale and out_scale must be powers of two in [2^-20, 2^20]%s");
  if (batch <= 0) return ACX_OK;
  if (L <= 192 || L > AP3_ROWS || heads <= 0 || (((uintptr_t)qkv_planes | (uintptr_t)out_planes) & 15))
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_p3h16: 192 < L <= 208, 16-byte aligned planes%s");
  return ap3_launch(ctx, 116, qkv_planes, 0, out_planes, batch, L, heads, stream, "acx_attention_p3h16", out_scale / in_scale,
                    1.f / (in_scale * in_scale));
}

// the same contract without the L gate: the streaming kernel (attn_s16_kernel), 1 <= L <= 1024.  Every refusal comes before the launch.
extern "C" int acx_attention_s16(acx_ctx* ctx, const void* qkv_planes, float in_scale, void* out_planes, float out_scale, int32_t batch,
                                 int32_t L, int32_t heads, void* stream) {
  if (!qkv_planes || !out_planes) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_s16: null pointer%s");
  int e = 0;
  if (!(in_scale >= 0x1p-20f && in_scale <= 0x1p20f) || frexpf(in_scale, &e) != 0.5f || !(out_scale >= 0x1p-20f && out_scale <= 0x1p20f) ||
      frexpf(out_scale, &e) != 0.5f)
    return acx_fail(ctx, ACX_E_BADARG, "acx_attention_s16: in_scale and out_scale must be powers of two in [2^-20, 2^20]%s");
  if (batch < 1 || heads < 1) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_s16: need batch >= 1 and heads >= 1%s");
  if (L < 1 || L > 1024) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_s16: need 1 <= L <= 1024%s");
  if (((uintptr_t)qkv_planes | (uintptr_t)out_planes) & 15) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_s16: planes must be 16-byte aligned%s");
  const int nt = (L + 31) / 32, nqb = (nt + AS16_NW - 1) / AS16_NW;
  const int64_t rows = (int64_t)batch * L, items = (int64_t)batch * heads * nqb;
  if (items > INT32_MAX || rows * 3 * heads * 64 > ((int64_t)1 << 40))
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_s16: batch * heads too large%s");
  const int ncu = ctx && ctx->multiprocessors > 0 ? ctx->multiprocessors : 256;
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_ATTN, s);
  const dim3 grid((unsigned)(items < 2 * ncu ? items : 2 * ncu));   // two workgroups per CU
  hipLaunchKernelGGL(attn_s16_kernel, grid, dim3(AS16_NW * 64), (size_t)AS16_LDS_B, s, (const u16*)qkv_planes, rows * 3 * heads * 64, rows,
                     (u16*)out_planes, rows * heads * 64, L, heads, batch * heads, (int)items, out_scale / in_scale, 1.f / (in_scale * in_scale));
  ACX_CHECK_LAUNCH(ctx, "acx_attention_s16");
  return ACX_OK;
}

extern "C" int acx_attention_x3(acx_ctx* ctx, const float* qkv, int64_t ldqkv, void* out_planes, int64_t ldo,
                                int32_t batch, int32_t L, int32_t heads, void* stream) {
  return attention_impl(ctx, qkv, ldqkv, (float*)out_planes, ldo, batch, L, heads, 0, stream, 1);
}
extern "C" int acx_attention_x3_panel(acx_ctx* ctx, const float* qkv, int64_t ldqkv, void* out_planes, int64_t ldo,
                                      int32_t batch, int32_t L, int32_t heads, void* stream) {
  if (ldo != (int64_t)heads * 64) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_x3_panel: dense planes (ldo == heads * 64)%s");
  return attention_impl(ctx, qkv, ldqkv, (float*)out_planes, ldo, batch, L, heads, 0, stream, 2);
}

extern "C" int acx_attention_bf16(acx_ctx* ctx, const void* qkv, int64_t ldqkv, void* out, int64_t ldo, int32_t batch,
                                  int32_t L, int32_t heads, void* stream) {
  if (!qkv || !out) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_bf16: null pointer%s");
  if (batch <= 0) return ACX_OK;
  if (L <= 0 || L > 224 || heads <= 0) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_bf16: need 0 < L <= 224%s");
  if (ldqkv % 8 || ldo % 4 || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 7))
    return acx_fail(ctx, ACX_E_BADARG, "acx_attention_bf16: qkv 16-byte aligned with ld%%8==0, out 8-byte aligned with ld%%4==0%s");
  const int nt = (L + 31) / 32;
  const dim3 grid((unsigned)(batch * heads));
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_ATTN, s);
  const int dev_slot = (ctx ? ctx->device : 0) & 63;
#define ACX_ATTNB(NT)                                                                              \
  acx_launch_lds<attn_bf16_kernel<NT>>(dev_slot, grid, dim3(256), (size_t)NT * 32 * BK_ROWB + 2 * BV_PANEL_B, s, (const u16*)qkv, ldqkv, \
                                       (u16*)out, ldo, L, heads)
  switch (nt) {
    case 1: ACX_ATTNB(1); break;
    case 2: ACX_ATTNB(2); break;
    case 3: ACX_ATTNB(3); break;
    case 4: ACX_ATTNB(4); break;
    case 5: ACX_ATTNB(5); break;
    case 6: ACX_ATTNB(6); break;
    default: ACX_ATTNB(7); break;
  }
#undef ACX_ATTNB
  ACX_CHECK_LAUNCH(ctx, "acx_attention_bf16");
  return ACX_OK;
}

extern "C" int acx_attention_cls(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo, int32_t batch,
                                 int32_t L, int32_t heads, void* stream) {
  if (!qkv || !out) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_cls: null pointer%s");
  if (batch <= 0) return ACX_OK;
  if (L <= 0 || L > 1024 || heads <= 0) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_cls: need 0 < L <= 1024%s");
  if (ldqkv % 4 || ((uintptr_t)qkv & 15)) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_cls: alignment%s");
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_ATTN, s);
  const int64_t n = (int64_t)batch * heads;
  hipLaunchKernelGGL(attn_cls_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, qkv, ldqkv, out, ldo, batch, L, heads);
  ACX_CHECK_LAUNCH(ctx, "acx_attention_cls");
  return ACX_OK;
}

extern "C" size_t acx_attention_cls_fold_workspace_bytes(int32_t batch, int32_t heads) {
  if (batch <= 0 || heads <= 0) return 0;
  return (size_t)2 * batch * heads * heads * 64 * sizeof(float);                 // u | z, [batch, heads, 64 heads] each
}

extern "C" int acx_attention_cls_fold(acx_ctx* ctx, const float* x, const float* ln_w, const float* ln_b, float eps,
                                      const float* in_proj_w, const float* in_proj_b, const float* q, int64_t ldq, float* out,
                                      int64_t ldo, int32_t batch, int32_t L, int32_t W, int32_t heads, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (!x || !ln_w || !ln_b || !in_proj_w || !in_proj_b || !q || !out || !workspace)
    return acx_fail(ctx, ACX_E_BADARG, "acx_attention_cls_fold: null pointer%s");
  if (batch <= 0) return ACX_OK;
  if (L <= 0 || L > 1024) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_cls_fold: need 0 < L <= 1024%s");
  if (heads <= 0 || W != heads * 64) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_cls_fold: head dim must be 64%s");
  switch (heads) {   // the LayerNorm widths
    case 1: case 2: case 4: case 8: case 10: case 12: case 16: break;
    default: return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_cls_fold: width %s%ld not in {64,128,256,512,640,768,1024}", "", (long)W);
  }
  if (((uintptr_t)x & 15) || ((uintptr_t)workspace & 15)) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_cls_fold: x and workspace must be 16-byte aligned%s");
  if (workspace_bytes < acx_attention_cls_fold_workspace_bytes(batch, heads))
    return acx_fail(ctx, ACX_E_WORKSPACE, "acx_attention_cls_fold: workspace too small%s");
  hipStream_t s = (hipStream_t)stream;
  const int dev_slot = (ctx ? ctx->device : 0) & 63;
  float* u = (float*)workspace;
  float* z = u + (size_t)batch * heads * W;
  const float* wk = in_proj_w + (size_t)W * W;
  const float* wv = in_proj_w + (size_t)2 * W * W;
  const int HP = (heads + 3) & ~3;
  const size_t lds = ((size_t)heads * W + (size_t)L * HP) * 4 + (size_t)L * 8;   // <= 136 KB (W = 1024, L = 1024)
  AcxProfScope prof__(ctx, ACX_K_ATTN, s);
#define ACX_CLS_FOLD(V) \
  acx_launch_lds<cls_fold_kernel<V>>(dev_slot, dim3((unsigned)batch), dim3(256), lds, s, x, (const float*)u, ln_w, ln_b, z, (int)L, eps)
  hipLaunchKernelGGL(cls_fold_u_kernel, dim3((unsigned)heads, (unsigned)((batch + CF_UF - 1) / CF_UF)), dim3(256), 0, s, q, ldq, wk,
                     ln_w, u, (int)batch, (int)W);
  switch (heads) {
    case 1: ACX_CLS_FOLD(1); break;
    case 2: ACX_CLS_FOLD(2); break;
    case 4: ACX_CLS_FOLD(4); break;
    case 8: ACX_CLS_FOLD(8); break;
    case 10: ACX_CLS_FOLD(10); break;
    case 12: ACX_CLS_FOLD(12); break;
    default: ACX_CLS_FOLD(16); break;
  }
#undef ACX_CLS_FOLD
  hipLaunchKernelGGL(cls_fold_o_kernel, dim3((unsigned)heads, (unsigned)((batch + CF_OF - 1) / CF_OF)), dim3(256), 0, s, (const float*)z,
                     wv, in_proj_b + 2 * W, out, ldo, (int)batch, (int)W);
  ACX_CHECK_LAUNCH(ctx, "acx_attention_cls_fold");
  return ACX_OK;
}

// ---- head dimension 80 (acx_attn_hd.h).  64 is refused, not forwarded: acx_attention and its variants are the entry points of that
// head dimension, with their own routes and error codes, and one meaning per entry point keeps both contracts short.
static int attn_hd_dim(acx_ctx* ctx, const char* who, int32_t head_dim) {
  if (head_dim == 80) return ACX_OK;
  return acx_fail(ctx, ACX_E_UNSUPPORTED, "%s: head_dim %ld is not supported (80; head dimension 64 is acx_attention's)", who, (long)head_dim);
}

extern "C" int acx_attention_hd_route(const acx_ctx* ctx, int32_t L, int32_t head_dim, int32_t out_aligned) {
  (void)ctx;                                                             // (no device property enters the rule)
  if (head_dim != 80 || L <= 0 || L > 1024 || !out_aligned) return ACX_E_UNSUPPORTED;
  return L > 128 ? ACX_ATTN_HD_ROUTE_STREAM_QB : ACX_ATTN_HD_ROUTE_STREAM;
}

// x3: 0 f32 rows, 1 three row-major bf16 planes, 2 three K-panel planes
static int attention_hd_impl(acx_ctx* ctx, const char* who, const float* qkv, int64_t ldqkv, void* out, int64_t ldo, int32_t batch, int32_t L,
                             int32_t heads, int32_t head_dim, void* stream, int x3) {
  if (!qkv || !out) return acx_fail(ctx, ACX_E_BADARG, "%s: null pointer", who);
  int rc = attn_hd_dim(ctx, who, head_dim);
  if (rc) return rc;
  if (L <= 0 || L > 1024 || heads <= 0) return acx_fail(ctx, ACX_E_UNSUPPORTED, "%s: need 1 <= L <= 1024 and heads >= 1", who);
  if (batch <= 0) return ACX_OK;
  const int64_t W = (int64_t)heads * head_dim;
  if (ldqkv % 4 || ldqkv < 3 * W || ((uintptr_t)qkv & 15)) return acx_fail(ctx, ACX_E_BADARG, "%s: qkv must be 16-byte aligned, ldqkv %% 4 == 0 and >= 3 heads head_dim", who);
  if (ldo < W) return acx_fail(ctx, ACX_E_BADARG, "%s: ldo < heads head_dim", who);
  if (x3 == 2 && ldo % 32) return acx_fail(ctx, ACX_E_BADARG, "%s: K-panel planes need ldo %% 32 == 0", who);
  const int route = acx_attention_hd_route(ctx, L, head_dim, ldo % 4 == 0 && !((uintptr_t)out & 15));
  if (route < 0) return acx_fail(ctx, route, "%s: out must be 16-byte aligned with ldo %% 4 == 0", who);
  const int nqb = route == ACX_ATTN_HD_ROUTE_STREAM_QB ? ((L + 15) / 16 + 7) / 8 : 1;
  const int64_t items = (int64_t)batch * heads * nqb;
  if (items > INT32_MAX || (int64_t)batch * L > INT32_MAX) return acx_fail(ctx, ACX_E_UNSUPPORTED, "%s: batch * heads too large", who);
  const int nitems = (int)items;
  const int ncu = ctx && ctx->multiprocessors > 0 ? ctx->multiprocessors : 256;
  const int slots = 2 * ncu;                                              // two workgroups per CU
  const dim3 grid((unsigned)(nitems < slots ? nitems : slots));
  const int64_t x3plane = x3 ? (int64_t)batch * L * ldo : (int64_t)0, prows = x3 == 2 ? (int64_t)batch * L : (int64_t)0;
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_ATTN, s);
  hipLaunchKernelGGL(attn_hd_kernel<80>, grid, dim3(512), AhdGeom<80>::LDS_B, s, qkv, ldqkv, (float*)out, ldo, L, heads, nitems, nqb, x3plane, prows);
  ACX_CHECK_LAUNCH(ctx, who);
  return ACX_OK;
}

extern "C" int acx_attention_hd(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo, int32_t batch, int32_t L,
                                int32_t heads, int32_t head_dim, void* stream) {
  return attention_hd_impl(ctx, "acx_attention_hd", qkv, ldqkv, out, ldo, batch, L, heads, head_dim, stream, 0);
}

extern "C" int acx_attention_x3_hd(acx_ctx* ctx, const float* qkv, int64_t ldqkv, void* out_planes, int64_t ldo, int32_t batch, int32_t L,
                                   int32_t heads, int32_t head_dim, int32_t panel, void* stream) {
  return attention_hd_impl(ctx, "acx_attention_x3_hd", qkv, ldqkv, out_planes, ldo, batch, L, heads, head_dim, stream, panel ? 2 : 1);
}

extern "C" int acx_attention_cls_hd(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo, int32_t batch, int32_t L,
                                    int32_t heads, int32_t head_dim, void* stream) {
  if (!qkv || !out) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_cls_hd: null pointer%s");
  int rc = attn_hd_dim(ctx, "acx_attention_cls_hd", head_dim);
  if (rc) return rc;
  if (L <= 0 || L > 1024 || heads <= 0) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_cls_hd: need 1 <= L <= 1024 and heads >= 1%s");
  if (batch <= 0) return ACX_OK;
  const int64_t W = (int64_t)heads * head_dim;
  if (ldqkv % 4 || ldqkv < 3 * W || ((uintptr_t)qkv & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_attention_cls_hd: qkv must be 16-byte aligned, ldqkv %% 4 == 0 and >= 3 heads head_dim%s");
  if (ldo < W) return acx_fail(ctx, ACX_E_BADARG, "acx_attention_cls_hd: ldo < heads head_dim%s");
  if ((int64_t)batch * heads > INT32_MAX || (int64_t)batch * L > INT32_MAX)
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_attention_cls_hd: batch * heads too large%s");
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_ATTN, s);
  const int64_t n = (int64_t)batch * heads;
  hipLaunchKernelGGL(attn_cls_hd_kernel<80>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, qkv, ldqkv, out, ldo, batch, L, heads);
  ACX_CHECK_LAUNCH(ctx, "acx_attention_cls_hd");
  return ACX_OK;
}
