// Row-wise normalisation kernels (HBM-bound): one 64-lane wavefront per row, values kept in
// registers between the two reduction passes, 16-byte loads/stores when the row allows.
//   acx_layernorm  : nn.LayerNorm (clip/model.py:174-180, classification_head.py:7) and the
//                    axial_attention ChanLayerNorm variant (eps added to the std)
//   acx_vit_embed  : CLS concat + positional embedding + ln_pre (clip/model.py:270-279)
//   acx_cls_head   : mean of the two reversible streams + LayerNorm + Linear(E,1) + sigmoid
//                    (classification_head.py:11-15), with the inverse test-mode tiling on store
#include "acx_internal.h"
#include "acx_ln_rows.h"     // normalize, ln_panel2_store: shared with the LayerNorm rider of the plane-reuse GEMM

namespace {

// OUT_BF16 == 2: the row as THREE bf16 planes hi | mid | lo (x = hi + mid + lo to 24 bits: the A operand of acx_gemm_desc.pairs =
// 6), plane p at y + p * plane elements
// OUT_BF16 == 3: the same planes in K-panel layout (ACX_BF16X3P): y = plane base, element e of row `prow` of `prows` rows at
// ((e / 32) * prows + prow) * 32 + e % 32
template <int VPL, int OUT_BF16>
__device__ __forceinline__ void store_row_affine(void* y, int lane, const float (&v)[VPL],
                                                 const float* __restrict__ w, const float* __restrict__ b, int64_t plane = 0,
                                                 int64_t prow = 0, int64_t prows = 0) {
  if constexpr (VPL % 4 == 0) {
#pragma unroll
    for (int i = 0; i < VPL / 4; ++i) {
      const int e = 4 * lane + 256 * i;
      const float4 ww = *reinterpret_cast<const float4*>(w + e);
      const float4 bb = *reinterpret_cast<const float4*>(b + e);
      float4 o;
      o.x = v[4 * i] * ww.x + bb.x; o.y = v[4 * i + 1] * ww.y + bb.y;
      o.z = v[4 * i + 2] * ww.z + bb.z; o.w = v[4 * i + 3] * ww.w + bb.w;
      if constexpr (OUT_BF16 == 2 || OUT_BF16 == 3) {
        const float ov[4] = {o.x, o.y, o.z, o.w};
        u16 hh[4], mm[4], ll[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          hh[k] = f2bf(ov[k]);
          const float r1 = ov[k] - bf2f(hh[k]);
          mm[k] = f2bf(r1);
          ll[k] = f2bf(r1 - bf2f(mm[k]));
        }
        const int64_t eo = OUT_BF16 == 3 ? ((int64_t)(e >> 5) * prows + prow) * 32 + (e & 31) : (int64_t)e;
        uint2 pk;
        pk.x = (uint32_t)hh[0] | ((uint32_t)hh[1] << 16); pk.y = (uint32_t)hh[2] | ((uint32_t)hh[3] << 16);
        *reinterpret_cast<uint2*>((u16*)y + eo) = pk;
        pk.x = (uint32_t)mm[0] | ((uint32_t)mm[1] << 16); pk.y = (uint32_t)mm[2] | ((uint32_t)mm[3] << 16);
        *reinterpret_cast<uint2*>((u16*)y + plane + eo) = pk;
        pk.x = (uint32_t)ll[0] | ((uint32_t)ll[1] << 16); pk.y = (uint32_t)ll[2] | ((uint32_t)ll[3] << 16);
        *reinterpret_cast<uint2*>((u16*)y + 2 * plane + eo) = pk;
      } else if constexpr (OUT_BF16 == 1) {
        uint2 pk;
        pk.x = (uint32_t)f2bf(o.x) | ((uint32_t)f2bf(o.y) << 16);
        pk.y = (uint32_t)f2bf(o.z) | ((uint32_t)f2bf(o.w) << 16);
        *reinterpret_cast<uint2*>((u16*)y + e) = pk;
      } else {
        *reinterpret_cast<float4*>((float*)y + e) = o;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int e = lane + 64 * i;
      const float o = v[i] * w[e] + b[e];
      if constexpr (OUT_BF16 == 2 || OUT_BF16 == 3) {
        const u16 h1 = f2bf(o);
        const float r1 = o - bf2f(h1);
        const u16 m1 = f2bf(r1);
        const int64_t eo = OUT_BF16 == 3 ? ((int64_t)(e >> 5) * prows + prow) * 32 + (e & 31) : (int64_t)e;
        ((u16*)y)[eo] = h1; ((u16*)y)[plane + eo] = m1; ((u16*)y)[2 * plane + eo] = f2bf(r1 - bf2f(m1));
      } else if constexpr (OUT_BF16 == 1) ((u16*)y)[e] = f2bf(o); else ((float*)y)[e] = o;
    }
  }
}

template <int VPL, int OUT_BF16>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, int64_t ldx,
                                                        const float* __restrict__ w, const float* __restrict__ b,
                                                        void* __restrict__ y, int64_t ldy, int64_t rows,
                                                        float eps, int mode) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[VPL];
  load_row<VPL>(x + row * ldx, lane, v);
  normalize<VPL>(v, eps, mode);
  void* yr = OUT_BF16 == 3 ? y : OUT_BF16 ? (void*)((u16*)y + row * ldy) : (void*)((float*)y + row * ldy);
  store_row_affine<VPL, OUT_BF16>(yr, lane, v, w, b, rows * ldy, row, rows);
}

// K-panel planes (ACX_BF16X3P), TWO rows per wave: with one row per wave a store instruction writes eight separate 64-byte pieces
// (one per 32-column panel: half lines; 0.157 ms per ViT LayerNorm against 0.12 for row-major planes).  Here lane pairs trade
// halves -- the even lane of a pair ends up with eight consecutive elements of row r, the odd lane with the same eight of row r + 1
// -- so that eight lanes write the 128 contiguous bytes rows r, r + 1 occupy in a panel with 16-byte stores.  Same arithmetic.
// TWO (ACX_BF16X2P): the hi and mid planes only (the lo plane is left untouched: a pairs = 3 product does not read it)
// F16 (ACX_F16X2P): two fp16 planes hi | lo (hi = fp16(sc y), lo = fp16(sc y - hi)) instead of bf16 planes; sc: a power of two
template <int VPL, bool TWO = false, bool F16 = false>
__global__ __launch_bounds__(256) void layernorm_panel2_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                               const float* __restrict__ b, u16* __restrict__ y, int64_t rows,
                                                               float eps, int mode, int64_t row0, float sc) {
  static_assert(VPL % 4 == 0, "16-byte row loads");
  // row0 (even): the launch covers rows row0 .. rows of the planes (acx_gemm_ln: the rows before it rode in the product's last round)
  const int lane = threadIdx.x & 63;
  const int64_t r0 = row0 + ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 2;  // even: rows r0, r0 + 1 share a line in every panel
  if (r0 >= rows) return;
  const bool two = r0 + 1 < rows;
  float va[VPL], vb[VPL];
  load_row<VPL>(x + r0 * ldx, lane, va);
  load_row<VPL>(x + (two ? r0 + 1 : r0) * ldx, lane, vb);
  normalize<VPL>(va, eps, mode);
  normalize<VPL>(vb, eps, mode);
  float4 ww[VPL / 4], bb[VPL / 4];
  ln_load_affine<VPL>(w, b, lane, ww, bb);
  ln_panel2_store<VPL, TWO, F16>(va, vb, ww, bb, y, rows, r0, two, lane, sc);
}

template <int VPL>
__global__ __launch_bounds__(256) void vit_embed_kernel(const float* __restrict__ patch_out,
                                                        const float* __restrict__ cls, const float* __restrict__ pos,
                                                        const float* __restrict__ lw, const float* __restrict__ lb,
                                                        float* __restrict__ x, int64_t rows, int T) {
  constexpr int W = 64 * VPL;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t f = row / (T + 1);
  const int tok = (int)(row - f * (T + 1));
  float v[VPL], p[VPL];
  load_row<VPL>(tok == 0 ? cls : patch_out + (f * T + tok - 1) * W, lane, v);
  load_row<VPL>(pos + (int64_t)tok * W, lane, p);
#pragma unroll
  for (int i = 0; i < VPL; ++i) v[i] += p[i];
  normalize<VPL>(v, 1e-5f, ACX_NORM_LAYER);
  store_row_affine<VPL, 0>(x + row * W, lane, v, lw, lb);
}

template <int VPL>
__global__ __launch_bounds__(256) void cls_head_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                       const float* __restrict__ lw, const float* __restrict__ lb,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ scores, int64_t rows, int gn, int gl, int seg,
                                                       const int* __restrict__ tile_table) {
  constexpr int E = 64 * VPL;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float a[VPL], c[VPL];
  load_row<VPL>(x1 + row * E, lane, a);
  load_row<VPL>(x2 + row * E, lane, c);
#pragma unroll
  for (int i = 0; i < VPL; ++i) a[i] = (a[i] + c[i]) * 0.5f;   // torch.stack(chunks).mean(0)
  normalize<VPL>(a, 1e-5f, ACX_NORM_LAYER);
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int e = elem_index<VPL>(lane, i);
    dot += (a[i] * lw[e] + lb[e]) * w[e];
  }
  dot = wave_sum(dot) + bias[0];
  if (lane == 0) {
    int64_t dst = row;
    if (tile_table) {   // batch of videos with their own segment sizes: row (tile, n, l) -> base + n * stride + l
      const int grid_sz = gn * gl;
      const int64_t tile = row / grid_sz;
      const int rem = (int)(row - tile * grid_sz);
      const int n = rem / gl, l = rem - n * gl;
      dst = (int64_t)tile_table[2 * tile] + (int64_t)n * tile_table[2 * tile + 1] + l;
    } else if (seg > 0) {  // row is ((b s) n l) -> write at ((b n s l))  (temporal_model.py:69-71)
      const int grid_sz = gn * gl;
      const int64_t per = (int64_t)grid_sz * seg;
      const int64_t bb = row / per, rem = row - bb * per;
      const int s = (int)(rem / grid_sz), rem2 = (int)(rem - (int64_t)s * grid_sz);
      const int n = rem2 / gl, l = rem2 - n * gl;
      dst = ((bb * gn + n) * seg + s) * gl + l;
    }
    scores[dst] = 1.f / (1.f + expf(-dot));
  }
}

}  // namespace

#define COMMA ,
// (a width that is no multiple of 64 takes the default: D / 64 alone would hand 96 or 130 to the 64- or 128-wide kernel)
// DISPATCH_VPL: the widths of the classification head.  DISPATCH_VPL_VIT: those and 1280 (20 values per lane: the ViT-H-14 width) for
// acx_layernorm and acx_vit_embed.  One switch (DISPATCH_VPL_); the launch goes in as the variadic tail because its commas arrive
// expanded.  The refusal of the longer list keeps the shorter one's text as it stands and names 1280 behind it.
#define VPL_NO_20(...)
#define VPL_CASE_20(...) case 20: { constexpr int V = 20; __VA_ARGS__; } break;
#define DISPATCH_VPL_(D, CASE20, WIDTHS, ...)                 \
  switch ((D) % 64 ? 0 : (D) / 64) {                          \
    case 1: { constexpr int V = 1; __VA_ARGS__; } break;      \
    case 2: { constexpr int V = 2; __VA_ARGS__; } break;      \
    case 4: { constexpr int V = 4; __VA_ARGS__; } break;      \
    case 8: { constexpr int V = 8; __VA_ARGS__; } break;      \
    case 10: { constexpr int V = 10; __VA_ARGS__; } break;    \
    case 12: { constexpr int V = 12; __VA_ARGS__; } break;    \
    case 16: { constexpr int V = 16; __VA_ARGS__; } break;    \
    CASE20(__VA_ARGS__)                                       \
    default: return acx_fail(ctx, ACX_E_UNSUPPORTED, "row width %s%ld not in " WIDTHS, "", (long)(D)); \
  }
#define DISPATCH_VPL(D, CALL) DISPATCH_VPL_(D, VPL_NO_20, "{64,128,256,512,640,768,1024}", CALL)
#define DISPATCH_VPL_VIT(D, CALL) DISPATCH_VPL_(D, VPL_CASE_20, "{64,128,256,512,640,768,1024} or 1280", CALL)

// row0 > 0 (acx_layernorm_rows; even, K-panel bf16 x 3 planes on the two-rows-per-wave kernel only): rows row0 .. rows
static int layernorm_impl(acx_ctx* ctx, const float* x, int64_t ldx, const float* w, const float* b,
                          void* y, int64_t ldy, int32_t y_dtype, int64_t rows, int32_t D, float eps,
                          int32_t mode, void* stream, int64_t row0, float y_scale = 1.f) {
  if (!x || !w || !b || !y) return acx_fail(ctx, ACX_E_BADARG, "acx_layernorm: null pointer%s");
  if (rows <= 0 || row0 >= rows) return ACX_OK;
  if (row0 && (row0 < 0 || (row0 & 1) || (y_dtype != ACX_BF16X3P && y_dtype != ACX_F16X2P) || ((uintptr_t)y & 15) || ((rows * (int64_t)D * 2) & 15)))
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_layernorm_rows: an even first row, ACX_BF16X3P or ACX_F16X2P planes, 16-byte aligned%s");
  if (D % 64 || ldx % 4 || ldy % 4) return acx_fail(ctx, ACX_E_BADARG, "acx_layernorm: D%%64 / ld%%4%s");
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_NORM, s);
  if (y_dtype == ACX_F16X2P) {         // two fp16 planes in K-panel layout (the ViT widths: the ACX_PREC_F16X3 / ACX_PREC_F32X6_LN16 drivers)
    if (ldy != D || (D != 768 && D != 1024) || ((uintptr_t)y & 15) || ((rows * (int64_t)D * 2) & 15))
      return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_layernorm: ACX_F16X2P needs ldy == D == 768 or 1024 and 16-byte aligned planes%s");
    const dim3 grid2((unsigned)((rows - row0 + 7) / 8));
    if (D == 768) layernorm_panel2_kernel<12, true, true><<<grid2, block, 0, s>>>(x, ldx, w, b, (u16*)y, rows, eps, mode, row0, y_scale);
    else layernorm_panel2_kernel<16, true, true><<<grid2, block, 0, s>>>(x, ldx, w, b, (u16*)y, rows, eps, mode, row0, y_scale);
    ACX_CHECK_LAUNCH(ctx, "acx_layernorm");
    return ACX_OK;
  }
  if (y_dtype == ACX_BF16X3P || y_dtype == ACX_BF16X2P) {   // three planes in K-panel layout [D / 32][rows][32] each (ldy == D), y + p * rows * ldy
    if (ldy != D || D % 256) return acx_fail(ctx, ACX_E_BADARG, "acx_layernorm: ACX_BF16X3P needs ldy == D, D %% 256 == 0%s");
    if (!((uintptr_t)y & 15) && !((rows * (int64_t)D * 2) & 15)) {                // 16-byte stores: two rows per wave
      const dim3 grid2((unsigned)((rows - row0 + 7) / 8));
      if (y_dtype == ACX_BF16X2P && D == 768) {                                   // (hi and mid planes only: the ViT width)
        layernorm_panel2_kernel<12, true><<<grid2, block, 0, s>>>(x, ldx, w, b, (u16*)y, rows, eps, mode, (int64_t)0, 1.f);
        ACX_CHECK_LAUNCH(ctx, "acx_layernorm");
        return ACX_OK;
      }
      switch (D / 64) {
        case 4: layernorm_panel2_kernel<4><<<grid2, block, 0, s>>>(x, ldx, w, b, (u16*)y, rows, eps, mode, row0, 1.f); break;
        case 8: layernorm_panel2_kernel<8><<<grid2, block, 0, s>>>(x, ldx, w, b, (u16*)y, rows, eps, mode, row0, 1.f); break;
        case 12: layernorm_panel2_kernel<12><<<grid2, block, 0, s>>>(x, ldx, w, b, (u16*)y, rows, eps, mode, row0, 1.f); break;
        case 16: layernorm_panel2_kernel<16><<<grid2, block, 0, s>>>(x, ldx, w, b, (u16*)y, rows, eps, mode, row0, 1.f); break;
        case 20: layernorm_panel2_kernel<20><<<grid2, block, 0, s>>>(x, ldx, w, b, (u16*)y, rows, eps, mode, row0, 1.f); break;
        default: return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_layernorm: ACX_BF16X3P needs D in {256, 512, 768, 1024, 1280}%s");
      }
    } else
    DISPATCH_VPL_VIT(D, layernorm_kernel<V COMMA 3><<<grid COMMA block COMMA 0 COMMA s>>>(x, ldx, w, b, y, ldy, rows, eps, mode));
  } else if (y_dtype == ACX_BF16X3) {  // three dense planes [rows, ldy] each, y + p * rows * ldy
    DISPATCH_VPL_VIT(D, layernorm_kernel<V COMMA 2><<<grid COMMA block COMMA 0 COMMA s>>>(x, ldx, w, b, y, ldy, rows, eps, mode));
  } else if (y_dtype == ACX_BF16) {
    DISPATCH_VPL_VIT(D, layernorm_kernel<V COMMA 1><<<grid COMMA block COMMA 0 COMMA s>>>(x, ldx, w, b, y, ldy, rows, eps, mode));
  } else {
    DISPATCH_VPL_VIT(D, layernorm_kernel<V COMMA 0><<<grid COMMA block COMMA 0 COMMA s>>>(x, ldx, w, b, y, ldy, rows, eps, mode));
  }
  ACX_CHECK_LAUNCH(ctx, "acx_layernorm");
  return ACX_OK;
}

extern "C" int acx_layernorm(acx_ctx* ctx, const float* x, int64_t ldx, const float* w, const float* b,
                             void* y, int64_t ldy, int32_t y_dtype, int64_t rows, int32_t D, float eps,
                             int32_t mode, void* stream) {
  return layernorm_impl(ctx, x, ldx, w, b, y, ldy, y_dtype, rows, D, eps, mode, stream, 0);
}

// a power of two (or 0: 1) as the F16X2P planes' scale
static inline bool ln_scale_ok(float s) { int e; return s == 0.f || (s > 0.f && s <= 3.4e38f && frexpf(s, &e) == 0.5f); }

extern "C" int acx_layernorm_scaled(acx_ctx* ctx, const float* x, int64_t ldx, const float* w, const float* b, void* y, int64_t rows,
                                    int32_t D, float eps, int32_t mode, float y_scale, void* stream) {
  if (!ln_scale_ok(y_scale)) return acx_fail(ctx, ACX_E_BADARG, "acx_layernorm_scaled: y_scale must be a power of two%s");
  return layernorm_impl(ctx, x, ldx, w, b, y, D, ACX_F16X2P, rows, D, eps, mode, stream, 0, y_scale != 0.f ? y_scale : 1.f);
}

// acx_gemm_ln's remainder: the LayerNorm of rows row0 .. rows into ACX_BF16X3P planes of `rows` rows, or ACX_F16X2P planes of
// y_scale * y (acx_internal.h)
int acx_layernorm_rows(acx_ctx* ctx, const float* x, int64_t ldx, const float* w, const float* b, void* y, int32_t y_dtype, float y_scale,
                       int64_t rows, int64_t row0, int32_t D, float eps, int32_t mode, void* stream) {
  return layernorm_impl(ctx, x, ldx, w, b, y, D, y_dtype, rows, D, eps, mode, stream, row0, y_scale != 0.f ? y_scale : 1.f);
}

extern "C" int acx_vit_embed(acx_ctx* ctx, const float* patch_out, const float* cls, const float* pos,
                             const float* ln_w, const float* ln_b, float* x, int32_t F, int32_t T, int32_t W,
                             void* stream) {
  if (!patch_out || !cls || !pos || !ln_w || !ln_b || !x) return acx_fail(ctx, ACX_E_BADARG, "acx_vit_embed: null pointer%s");
  const int64_t rows = (int64_t)F * (T + 1);
  if (rows <= 0) return ACX_OK;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_NORM, s);
  DISPATCH_VPL_VIT(W, vit_embed_kernel<V><<<grid COMMA block COMMA 0 COMMA s>>>(patch_out, cls, pos, ln_w, ln_b, x, rows, T));
  ACX_CHECK_LAUNCH(ctx, "acx_vit_embed");
  return ACX_OK;
}

extern "C" int acx_cls_head(acx_ctx* ctx, const float* x1, const float* x2, const float* ln_w, const float* ln_b,
                            const float* lin_w, const float* lin_b, float* scores, int64_t rows, int32_t E,
                            int32_t gn, int32_t gl, int32_t seg, void* stream) {
  if (!x1 || !x2 || !ln_w || !ln_b || !lin_w || !lin_b || !scores) return acx_fail(ctx, ACX_E_BADARG, "acx_cls_head: null pointer%s");
  if (rows <= 0) return ACX_OK;
  if (seg > 0 && (gn <= 0 || gl <= 0 || rows % ((int64_t)gn * gl * seg)))
    return acx_fail(ctx, ACX_E_BADARG, "acx_cls_head: rows not a multiple of gn*gl*seg%s");
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_NORM, s);
  DISPATCH_VPL(E, cls_head_kernel<V><<<grid COMMA block COMMA 0 COMMA s>>>(x1, x2, ln_w, ln_b, lin_w, lin_b, scores, rows, gn, gl, seg, nullptr));
  ACX_CHECK_LAUNCH(ctx, "acx_cls_head");
  return ACX_OK;
}

extern "C" int acx_cls_head_tiles(acx_ctx* ctx, const float* x1, const float* x2, const float* ln_w, const float* ln_b,
                                  const float* lin_w, const float* lin_b, float* scores, int64_t rows, int32_t E, int32_t gn,
                                  int32_t gl, const int32_t* tile_table, void* stream) {
  if (!x1 || !x2 || !ln_w || !ln_b || !lin_w || !lin_b || !scores || !tile_table)
    return acx_fail(ctx, ACX_E_BADARG, "acx_cls_head_tiles: null pointer%s");
  if (rows <= 0) return ACX_OK;
  if (gn <= 0 || gl <= 0 || rows % ((int64_t)gn * gl)) return acx_fail(ctx, ACX_E_BADARG, "acx_cls_head_tiles: rows %% (gn*gl) != 0%s");
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t s = (hipStream_t)stream;
  AcxProfScope prof__(ctx, ACX_K_NORM, s);
  DISPATCH_VPL(E, cls_head_kernel<V><<<grid COMMA block COMMA 0 COMMA s>>>(x1, x2, ln_w, ln_b, lin_w, lin_b, scores, rows, gn, gl, 0, tile_table));
  ACX_CHECK_LAUNCH(ctx, "acx_cls_head_tiles");
  return ACX_OK;
}
