// The CLIP ResNet image encoder (ModifiedResNet, clip/model.py:111-171) in eval mode: its kernels that acx_gemm does not
// cover (stem im2col, 2x2 average pool on NHWC rows, the attention pool's mean token + positional add) and the driver that
// sequences them with acx_gemm and acx_attention_cls on the caller's stream (no allocation, no synchronisation).
//
// Layout: activations are NHWC rows [frames * H * W][Cp], Cp = the channel count rounded up to 32 (RN50x4's 40 / 80 and
// RN50x16's 48: the f32 CONV3X3 row map and the K-steps need multiples of 32).  The padding channels are zero: the caller's
// weights carry zero rows / columns there and zero biases, so every ReLU keeps them at 0.
#include "acx_internal.h"

extern "C" int acx_attention_cls(acx_ctx* ctx, const float* qkv, int64_t ldqkv, float* out, int64_t ldo, int32_t batch,
                                 int32_t L, int32_t heads, void* stream);
extern "C" size_t acx_bn_workspace_bytes(int64_t rows, int32_t C1);
extern "C" int acx_bn_stats(acx_ctx* ctx, const float* raw, int64_t rows, int32_t C1, float* mean, float* var_biased,
                            float* var_unbiased, void* workspace, size_t workspace_bytes, void* stream);
extern "C" int acx_bn_running_update(acx_ctx* ctx, const float* mean, const float* var_unbiased, float* running_mean,
                                     float* running_var, int64_t* num_batches_tracked, int32_t C1, float momentum, float one_minus,
                                     void* stream);

namespace {

inline int rn_cp(int c) { return (c + 31) / 32 * 32; }
inline size_t rn_al(size_t x) { return (x + 255) & ~(size_t)255; }

// stem conv1 (3x3, stride 2, pad 1) as im2col: out[(f, oy, ox)][k], k = c * 9 + ky * 3 + kx (conv1.weight.reshape(N, 27)), k >= 27 zero
__global__ __launch_bounds__(256) void rn_stem_im2col_kernel(const float* __restrict__ frames, float* __restrict__ out, int F, int R) {
  const int G = R / 2;
  const int64_t total = (int64_t)F * G * G * 32;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int k = (int)(i & 31);
  const int64_t row = i >> 5;
  const int ox = (int)(row % G);
  const int64_t t = row / G;
  const int oy = (int)(t % G);
  const int64_t f = t / G;
  float v = 0.f;
  if (k < 27) {
    const int c = k / 9, tap = k - c * 9, ky = tap / 3, kx = tap - ky * 3;
    const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
    if ((unsigned)iy < (unsigned)R && (unsigned)ix < (unsigned)R) v = frames[((f * 3 + c) * R + iy) * (int64_t)R + ix];
  }
  out[i] = v;
}

// AvgPool2d(2) on NHWC rows: out[f, y, x, :] = (in[2y, 2x] + in[2y, 2x + 1] + in[2y + 1, 2x] + in[2y + 1, 2x + 1]) * 0.25
// (the sum in PyTorch's window order; / 4 is exact as * 0.25).  C % 4 == 0, four channels per lane.
__global__ __launch_bounds__(256) void rn_avgpool2_kernel(const float* __restrict__ in, float* __restrict__ out, int F, int H, int W, int C) {
  const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
  const int64_t total = (int64_t)F * Ho * Wo * C4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4) * 4;
  const int64_t px = i / C4;
  const int x = (int)(px % Wo);
  const int64_t t = px / Wo;
  const int y = (int)(t % Ho);
  const int64_t f = t / Ho;
  const float* p = in + ((f * H + 2 * y) * W + 2 * x) * (int64_t)C + c;
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + C);
  const float4 e = *reinterpret_cast<const float4*>(p + (int64_t)W * C);
  const float4 g = *reinterpret_cast<const float4*>(p + (int64_t)W * C + C);
  *reinterpret_cast<float4*>(out + px * C + c) = make_float4((a.x + b.x + e.x + g.x) * 0.25f, (a.y + b.y + e.y + g.y) * 0.25f,
                                                             (a.z + b.z + e.z + g.z) * 0.25f, (a.w + b.w + e.w + g.w) * 0.25f);
}

// AttentionPool2d tokens (clip/model.py:82-84): x [F * HW][E] -> tok [F * (HW + 1)][E], token 0 = mean over HW, then + pos[t].
// One lane per (frame, column): the mean is an f64 sum over HW in token order (deterministic), rounded once.
__global__ __launch_bounds__(256) void rn_attnpool_tokens_kernel(const float* __restrict__ x, const float* __restrict__ pos,
                                                                 float* __restrict__ tok, int F, int HW, int E) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)F * E) return;
  const int c = (int)(i % E);
  const int64_t f = i / E;
  const float* src = x + f * HW * (int64_t)E + c;
  float* dst = tok + f * (HW + 1) * (int64_t)E + c;
  double sum = 0.0;
  for (int t = 0; t < HW; ++t) {
    const float v = src[(int64_t)t * E];
    sum += v;
    dst[(int64_t)(t + 1) * E] = v + pos[(int64_t)(t + 1) * E + c];
  }
  dst[0] = (float)(sum / HW) + pos[c];
}

// training-mode BatchNorm2d, per channel: alpha = gamma / sqrt(var_b + eps), beta' = beta - mean alpha (f64, rounded once);
// the padding channels C..Cp get 0 / 0
__global__ __launch_bounds__(256) void rn_bn_prepare_kernel(const float* __restrict__ mean, const float* __restrict__ var_b,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, int C,
                                                            int Cp, float eps, float* __restrict__ alpha, float* __restrict__ shift) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= Cp) return;
  if (c >= C) { alpha[c] = 0.f; shift[c] = 0.f; return; }
  const double a = (double)gamma[c] / sqrt((double)var_b[c] + (double)eps);
  alpha[c] = (float)a;
  shift[c] = (float)((double)beta[c] - (double)mean[c] * a);
}

// y = x alpha + shift (+ residual), then ReLU when relu != 0 -- in place allowed (y == x); Cp % 4 == 0, four channels per lane
__global__ __launch_bounds__(256) void rn_bn_apply_kernel(const float* x, const float* __restrict__ alpha,
                                                          const float* __restrict__ shift, const float* residual, float* y,
                                                          int64_t rows, int Cp, int relu) {
  const int C4 = Cp / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C4) return;
  const int c = (int)(i % C4) * 4;
  const float4 v = reinterpret_cast<const float4*>(x)[i];
  const float4 a = *reinterpret_cast<const float4*>(alpha + c), b = *reinterpret_cast<const float4*>(shift + c);
  float o[4] = {v.x * a.x + b.x, v.y * a.y + b.y, v.z * a.z + b.z, v.w * a.w + b.w};
  if (residual) {
    const float4 r = reinterpret_cast<const float4*>(residual)[i];
    o[0] += r.x; o[1] += r.y; o[2] += r.z; o[3] += r.w;
  }
  if (relu) {
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], 0.f);
  }
  reinterpret_cast<float4*>(y)[i] = make_float4(o[0], o[1], o[2], o[3]);
}

}  // namespace

extern "C" int acx_bn_apply_nhwc(acx_ctx* ctx, const float* x, const float* mean, const float* var_biased, const float* gamma,
                                 const float* beta, const float* residual, float* y, int64_t rows, int32_t C, int32_t Cp, float eps,
                                 int32_t relu, float* scratch, void* stream) {
  if (!x || !mean || !var_biased || !gamma || !beta || !y || !scratch) return acx_fail(ctx, ACX_E_BADARG, "acx_bn_apply_nhwc: null pointer%s");
  if (rows <= 0 || C <= 0 || Cp < C || Cp % 4 || ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)residual | (uintptr_t)scratch) & 15)))
    return acx_fail(ctx, ACX_E_BADARG, "acx_bn_apply_nhwc: need rows > 0, C <= Cp, Cp %% 4 == 0 and 16-byte aligned buffers%s");
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  hipStream_t s = (hipStream_t)stream;
  float* alpha = scratch;
  float* shift = scratch + ((Cp + 3) / 4) * 4;
  hipLaunchKernelGGL(rn_bn_prepare_kernel, dim3((unsigned)((Cp + 255) / 256)), dim3(256), 0, s, mean, var_biased, gamma, beta, C, Cp,
                     eps, alpha, shift);
  const int64_t total = rows * (Cp / 4);
  hipLaunchKernelGGL(rn_bn_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, x, (const float*)alpha,
                     (const float*)shift, residual, y, rows, Cp, relu);
  ACX_CHECK_LAUNCH(ctx, "acx_bn_apply_nhwc");
  return ACX_OK;
}

extern "C" int acx_resnet_stem_im2col(acx_ctx* ctx, const float* frames, float* cols, int32_t F, int32_t R, void* stream) {
  if (!frames || !cols) return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_stem_im2col: null pointer%s");
  if (F <= 0 || R <= 0 || R % 2) return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_stem_im2col: need F > 0 and an even resolution%s");
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  const int64_t total = (int64_t)F * (R / 2) * (R / 2) * 32;
  hipLaunchKernelGGL(rn_stem_im2col_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, frames, cols, F, R);
  ACX_CHECK_LAUNCH(ctx, "acx_resnet_stem_im2col");
  return ACX_OK;
}

extern "C" int acx_avgpool2_nhwc(acx_ctx* ctx, const float* in, float* out, int32_t F, int32_t H, int32_t W, int32_t C, void* stream) {
  if (!in || !out) return acx_fail(ctx, ACX_E_BADARG, "acx_avgpool2_nhwc: null pointer%s");
  if (F <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2 || C <= 0 || C % 4 || (((uintptr_t)in | (uintptr_t)out) & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_avgpool2_nhwc: need even H, W, C %% 4 == 0 and 16-byte aligned buffers%s");
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  const int64_t total = (int64_t)F * (H / 2) * (W / 2) * (C / 4);
  hipLaunchKernelGGL(rn_avgpool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, F, H, W, C);
  ACX_CHECK_LAUNCH(ctx, "acx_avgpool2_nhwc");
  return ACX_OK;
}

extern "C" int acx_attnpool_tokens(acx_ctx* ctx, const float* x, const float* pos, float* tokens, int32_t F, int32_t HW, int32_t E,
                                   void* stream) {
  if (!x || !pos || !tokens) return acx_fail(ctx, ACX_E_BADARG, "acx_attnpool_tokens: null pointer%s");
  if (F <= 0 || HW <= 0 || E <= 0) return acx_fail(ctx, ACX_E_BADARG, "acx_attnpool_tokens: need F, HW, E > 0%s");
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  const int64_t total = (int64_t)F * E;
  hipLaunchKernelGGL(rn_attnpool_tokens_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, pos,
                     tokens, F, HW, E);
  ACX_CHECK_LAUNCH(ctx, "acx_attnpool_tokens");
  return ACX_OK;
}

// ------------------------------------------------------------------------------------------------------------- the driver
namespace {

struct RnGeom {
  int R, w, G1, E, HW, out, heads, nblocks;
  int64_t max_act;     // floats per frame of the largest activation buffer (stem and every block)
};

RnGeom rn_geom(const acx_resnet_desc* d) {
  RnGeom g;
  g.R = d->resolution; g.w = d->width; g.G1 = d->resolution / 2; g.E = d->width * 32; g.out = d->output_dim; g.heads = d->heads;
  const int Hf = d->resolution / 32;
  g.HW = Hf * Hf;
  g.nblocks = d->layers[0] + d->layers[1] + d->layers[2] + d->layers[3];
  int64_t m = (int64_t)g.G1 * g.G1 * rn_cp(g.w);
  m = m > (int64_t)g.G1 * g.G1 * 32 ? m : (int64_t)g.G1 * g.G1 * 32;
  int H = g.G1 / 2, inpl = g.w;
  for (int li = 0; li < 4; ++li) {
    const int planes = g.w << li;
    for (int j = 0; j < d->layers[li]; ++j) {
      const int64_t a = (int64_t)H * H * rn_cp(planes > inpl ? planes : inpl);
      if (a > m) m = a;
      if (li > 0 && j == 0) H /= 2;
      const int64_t o = (int64_t)H * H * 4 * planes;
      if (o > m) m = o;
      inpl = 4 * planes;
    }
  }
  g.max_act = m;
  return g;
}

// frames per internal batch: the largest activation stays below 2^31 bytes (every row index and operand offset of the GEMM
// kernels is then far inside 32 bits), at most 512
int rn_batch(const RnGeom& g) {
  int64_t fb = ((int64_t)1 << 31) / (g.max_act * 4);
  if (fb < 1) fb = 1;
  return (int)(fb > 512 ? 512 : fb);
}

struct RnWs {
  float *cols, *x, *t1, *t2, *p, *ds, *tok, *qkv, *o;
  // ACX_PREC_BF16X6 only: three buffers of three bf16 planes each (the A operands of the plane products) and the 256-byte zero
  // page of the convolution taps outside a frame
  char *pl0, *pl1, *pl2;
  void* zero;
  size_t total;
};

// The routing rule of ACX_PREC_BF16X6: which products run as pairs = 6 products of bf16 planes (gemm_x6_p4_kernel).  A rule on
// (K, N, convolution or not) ONLY -- never on the rows of a launch, so every internal batch and every frame count takes the same
// kernels: every 3x3 convolution, and every 1x1 convolution / linear layer from K = 64 (the K = 32 stem product stays f32).  The
// one-row-per-frame products of the attention pool (q of token 0, c_proj) are not asked: they stay on the few-row f32 kernel.
inline bool rn_routed(int K, int N, bool conv) {
  (void)N;
  return conv || K >= 64;
}

RnWs rn_carve(char* base, const RnGeom& g, int fb, bool planes) {
  RnWs w;
  size_t off = 0;
  auto take = [&](size_t floats) { float* p = (float*)(base + off); off += rn_al(floats * 4); return p; };
  w.cols = take((size_t)fb * g.G1 * g.G1 * 32);
  w.x = take((size_t)fb * g.max_act);
  w.t1 = take((size_t)fb * g.max_act);
  w.t2 = take((size_t)fb * g.max_act);
  w.p = take((size_t)fb * g.max_act);
  w.ds = take((size_t)fb * g.max_act);
  w.tok = take((size_t)fb * (g.HW + 1) * g.E);
  w.qkv = take((size_t)fb * (g.HW + 1) * 3 * g.E);
  w.o = take((size_t)fb * g.E);
  w.pl0 = w.pl1 = w.pl2 = nullptr;
  w.zero = nullptr;
  if (planes) {                                                  // (behind the f32 carve: that part is the same for every precision)
    const size_t tok = (size_t)(g.HW + 1) * g.E;
    const size_t el = (size_t)fb * ((size_t)g.max_act > tok ? (size_t)g.max_act : tok);
    auto take_b = [&](size_t bytes) { char* p = base + off; off += rn_al(bytes); return p; };
    w.pl0 = take_b(3 * el * 2);
    w.pl1 = take_b(3 * el * 2);
    w.pl2 = take_b(3 * el * 2);
    w.zero = take_b(256);
  }
  w.total = off;
  return w;
}

// one f32 product of the encoder: identity rows or the implicit 3x3 convolution on an H x W grid per frame (no split-K
// workspace: every row of a launch sums K in the same order, so identical frames give identical rows)
int rn_gemm(acx_ctx* ctx, const float* A, int lda, const float* W, int N, int K, float* C, int ldc, int64_t M, const float* bias,
            int act, const float* residual, int gh, int gw, int cin, hipStream_t s) {
  acx_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.A = A; d.W = W; d.C = C;
  d.M = (int32_t)M; d.N = N; d.K = K; d.lda = lda; d.ldw = K; d.ldc = ldc;
  d.a_dtype = ACX_F32; d.c_dtype = ACX_F32; d.prec = ACX_PREC_F32;
  d.bias = bias; d.act = act; d.residual = residual; d.ldr = ldc;
  if (cin) { d.amap = ACX_AMAP_CONV3X3; d.gn = gh; d.gl = gw; d.cin = cin; }
  return acx_gemm(ctx, &d, s);
}

// ACX_PREC_BF16X6: the three bf16 planes of an f32 activation [rows][cols] (dense planes, plane stride rows * cols * 2 bytes)
int rn_split(acx_ctx* ctx, const float* src, int cols, void* dst, int64_t rows, hipStream_t s) {
  return acx_split_bf16x3(ctx, src, cols, dst, rows * cols * 2, rows, cols, s);
}

// one pairs = 6 product of the encoder: A3 = three dense bf16 planes [M][lda], W3 = three planes [N][K] of the folded weight; the
// result as f32 rows (planes_out = false; ldc) or as the three planes of the next product's A operand (dense [M][N]).  No workspace:
// whole tiles, whole K per tile -- a row's bits do not depend on where its frame sits in the launch.
int rn_gemm6(acx_ctx* ctx, const void* A3, int lda, const void* W3, int N, int K, void* C, int ldc, bool planes_out, int64_t M,
             const float* bias, int act, const float* residual, int gh, int gw, int cin, const void* zero, hipStream_t s) {
  if (!W3) return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_encode: ACX_PREC_BF16X6 needs the w3 planes of every routed convolution%s");
  acx_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.A = A3; d.W = W3; d.C = C;
  d.M = (int32_t)M; d.N = N; d.K = K; d.lda = lda; d.ldw = K; d.ldc = planes_out ? N : ldc;
  d.a_dtype = ACX_BF16; d.c_dtype = planes_out ? ACX_BF16X3 : ACX_F32; d.prec = ACX_PREC_BF16; d.pairs = 6;
  d.a_plane_stride = M * lda * 2; d.w_plane_stride = (int64_t)N * K * 2;
  d.bias = bias; d.act = act; d.residual = residual; d.ldr = ldc;
  if (cin) { d.amap = ACX_AMAP_CONV3X3; d.gn = gh; d.gl = gw; d.cin = cin; d.zero_page = zero; }
  return acx_gemm(ctx, &d, s);
}

// attention pool (:71-108) of n frames x [n HW][E]: tokens, k | v for every token into a [n (HW + 1)][3E] q | k | v buffer, q for
// token 0 only, single-query attention per head (head dim 64, scale 64^-0.5), c_proj
int rn_attnpool(acx_ctx* ctx, const acx_resnet_weights* w, const RnGeom& g, const RnWs& ws, const float* x, int n, float* features,
                hipStream_t s, bool x6 = false) {
  int rc;
  const int E = g.E, L = g.HW + 1;
  if ((rc = acx_attnpool_tokens(ctx, x, w->positional_embedding, ws.tok, n, g.HW, E, s))) return rc;
  if (x6 && rn_routed(E, 2 * E, false)) {                         // k | v of every token: planes of the tokens, f32 rows out
    if ((rc = rn_split(ctx, ws.tok, E, ws.pl0, (int64_t)n * L, s))) return rc;
    if ((rc = rn_gemm6(ctx, ws.pl0, E, w->kv_w3, 2 * E, E, ws.qkv + E, 3 * E, false, (int64_t)n * L, w->kv_b, ACX_ACT_NONE, nullptr,
                       0, 0, 0, nullptr, s))) return rc;
  } else if ((rc = rn_gemm(ctx, ws.tok, E, w->kv_w, 2 * E, E, ws.qkv + E, 3 * E, (int64_t)n * L, w->kv_b, ACX_ACT_NONE, nullptr, 0, 0, 0, s)))
    return rc;
  if ((rc = rn_gemm(ctx, ws.tok, L * E, w->q_w, E, E, ws.qkv, L * 3 * E, n, w->q_b, ACX_ACT_NONE, nullptr, 0, 0, 0, s))) return rc;
  if ((rc = acx_attention_cls(ctx, ws.qkv, 3 * E, ws.o, E, n, L, g.heads, s))) return rc;
  return rn_gemm(ctx, ws.o, E, w->c_w, g.out, E, features, g.out, n, w->c_b, ACX_ACT_NONE, nullptr, 0, 0, 0, s);
}

int rn_encode_batch(acx_ctx* ctx, const acx_resnet_desc* d, const acx_resnet_weights* w, const RnGeom& g, const RnWs& ws,
                    const float* frames, int n, float* features, hipStream_t s) {
  int rc;
  const int c1 = rn_cp(g.w / 2), c2 = rn_cp(g.w);
  const int G = g.G1;
  const int64_t M1 = (int64_t)n * G * G;
  // stem (clip/model.py:157-162): conv1 (stride 2) as im2col + GEMM, conv2 / conv3 implicit 3x3, each BN (folded) + ReLU; AvgPool2d(2)
  if ((rc = acx_resnet_stem_im2col(ctx, frames, ws.cols, n, g.R, s))) return rc;
  if ((rc = rn_gemm(ctx, ws.cols, 32, w->stem[0].w, c1, 32, ws.t1, c1, M1, w->stem[0].b, ACX_ACT_RELU, nullptr, 0, 0, 0, s))) return rc;
  if ((rc = rn_gemm(ctx, ws.t1, c1, w->stem[1].w, c1, 9 * c1, ws.t2, c1, M1, w->stem[1].b, ACX_ACT_RELU, nullptr, G, G, c1, s))) return rc;
  if ((rc = rn_gemm(ctx, ws.t2, c1, w->stem[2].w, c2, 9 * c1, ws.t1, c2, M1, w->stem[2].b, ACX_ACT_RELU, nullptr, G, G, c1, s))) return rc;
  if ((rc = acx_avgpool2_nhwc(ctx, ws.t1, ws.x, n, G, G, c2, s))) return rc;
  // layer1..4 of Bottlenecks (:10-68)
  int H = G / 2, inpl = g.w, bi = 0;
  for (int li = 0; li < 4; ++li) {
    const int planes = g.w << li, pp = rn_cp(planes), cin = rn_cp(inpl), cout = 4 * planes;
    for (int j = 0; j < d->layers[li]; ++j, ++bi) {
      const acx_resnet_block& b = w->blocks[bi];
      const bool stride = li > 0 && j == 0;
      const int cin_b = j == 0 ? cin : cout;
      const int64_t M = (int64_t)n * H * H;
      // relu(bn1(conv1 1x1)), relu(bn2(conv2 3x3 pad 1))
      if ((rc = rn_gemm(ctx, ws.x, cin_b, b.conv1.w, pp, cin_b, ws.t1, pp, M, b.conv1.b, ACX_ACT_RELU, nullptr, 0, 0, 0, s))) return rc;
      if ((rc = rn_gemm(ctx, ws.t1, pp, b.conv2.w, pp, 9 * pp, ws.t2, pp, M, b.conv2.b, ACX_ACT_RELU, nullptr, H, H, pp, s))) return rc;
      const float* a3 = ws.t2;
      const float* xin = ws.x;
      const int Ho = stride ? H / 2 : H;
      if (stride) {                                              // avgpool(stride) of the branch and of the identity's input
        if ((rc = acx_avgpool2_nhwc(ctx, ws.t2, ws.t1, n, H, H, pp, s))) return rc;
        if ((rc = acx_avgpool2_nhwc(ctx, ws.x, ws.p, n, H, H, cin_b, s))) return rc;
        a3 = ws.t1; xin = ws.p;
      }
      const int64_t Mo = (int64_t)n * Ho * Ho;
      const float* ident = ws.x;
      if (b.downsample.w) {                                      // downsample: (avgpool) -> conv1x1 -> bn
        if ((rc = rn_gemm(ctx, xin, cin_b, b.downsample.w, cout, cin_b, ws.ds, cout, Mo, b.downsample.b, ACX_ACT_NONE, nullptr,
                          0, 0, 0, s))) return rc;
        ident = ws.ds;
      } else if (stride || cin_b != cout) {
        return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_encode: a block that changes shape needs downsample weights%s");
      }
      // relu(bn3(conv3 1x1) + identity): the identity is the block's input when there is no downsample (residual aliases C)
      if ((rc = rn_gemm(ctx, a3, pp, b.conv3.w, cout, pp, ws.x, cout, Mo, b.conv3.b, ACX_ACT_RESRELU, ident, 0, 0, 0, s))) return rc;
      H = Ho;
    }
    inpl = 4 * planes;
  }
  return rn_attnpool(ctx, w, g, ws, ws.x, n, features, s);
}

// The same batch at ACX_PREC_BF16X6: every product rn_routed names runs on the plane kernel.  A product whose only consumer is the
// next product writes that product's A planes itself (conv1 -> conv2, conv2 -> conv3 in a block without stride, the stem's conv2
// -> conv3); a result that is also needed as f32 rows -- a block's output (the next identity, the average pools' input), a pooled
// tensor, the stem's first product -- is split by acx_split_bf16x3.  Plane buffers: pl0 = the block input (then the pooled input
// of a downsample), pl1 = conv1's output (then the pooled branch), pl2 = conv2's output.
int rn_encode_batch_x6(acx_ctx* ctx, const acx_resnet_desc* d, const acx_resnet_weights* w, const RnGeom& g, const RnWs& ws,
                       const float* frames, int n, float* features, hipStream_t s) {
  int rc;
  const int c1 = rn_cp(g.w / 2), c2 = rn_cp(g.w);
  const int G = g.G1;
  const int64_t M1 = (int64_t)n * G * G;
  const void* Z = ws.zero;
  // one product: planes in (a3) when routed, else the f32 rows (af); planes out (c3) when routed and asked for, else f32 rows (cf)
  auto prod = [&](const float* af, const void* a3, int lda, const acx_resnet_conv& cv, int N, int K, float* cf, void* c3, int64_t M,
                  int act, const float* res, int gh, int cin) -> int {
    if (rn_routed(K, N, cin != 0))
      return rn_gemm6(ctx, a3, lda, cv.w3, N, K, c3 ? c3 : (void*)cf, N, c3 != nullptr, M, cv.b, act, res, gh, gh, cin, Z, s);
    int r = rn_gemm(ctx, af, lda, cv.w, N, K, cf, N, M, cv.b, act, res, gh, gh, cin, s);
    if (!r && c3) r = rn_split(ctx, cf, N, c3, M, s);
    return r;
  };
  if ((rc = acx_resnet_stem_im2col(ctx, frames, ws.cols, n, g.R, s))) return rc;
  if ((rc = rn_gemm(ctx, ws.cols, 32, w->stem[0].w, c1, 32, ws.t1, c1, M1, w->stem[0].b, ACX_ACT_RELU, nullptr, 0, 0, 0, s))) return rc;
  if ((rc = rn_split(ctx, ws.t1, c1, ws.pl0, M1, s))) return rc;
  if ((rc = prod(ws.t1, ws.pl0, c1, w->stem[1], c1, 9 * c1, ws.t2, ws.pl1, M1, ACX_ACT_RELU, nullptr, G, c1))) return rc;
  if ((rc = prod(ws.t2, ws.pl1, c1, w->stem[2], c2, 9 * c1, ws.t1, nullptr, M1, ACX_ACT_RELU, nullptr, G, c1))) return rc;
  if ((rc = acx_avgpool2_nhwc(ctx, ws.t1, ws.x, n, G, G, c2, s))) return rc;
  int H = G / 2, inpl = g.w, bi = 0;
  for (int li = 0; li < 4; ++li) {
    const int planes = g.w << li, pp = rn_cp(planes), cin = rn_cp(inpl), cout = 4 * planes;
    for (int j = 0; j < d->layers[li]; ++j, ++bi) {
      const acx_resnet_block& b = w->blocks[bi];
      const bool stride = li > 0 && j == 0;
      const int cin_b = j == 0 ? cin : cout;
      const int64_t M = (int64_t)n * H * H;
      const int Ho = stride ? H / 2 : H;
      const int64_t Mo = (int64_t)n * Ho * Ho;
      const bool r1 = rn_routed(cin_b, pp, false), r3 = rn_routed(pp, cout, false);
      const bool rds = b.downsample.w && rn_routed(cin_b, cout, false);
      // the block input's planes: conv1's A, and the downsample's in a block without stride
      if (r1 || (rds && !stride)) { if ((rc = rn_split(ctx, ws.x, cin_b, ws.pl0, M, s))) return rc; }
      if ((rc = prod(ws.x, ws.pl0, cin_b, b.conv1, pp, cin_b, ws.t1, ws.pl1, M, ACX_ACT_RELU, nullptr, 0, 0))) return rc;
      // conv2: planes for conv3 directly, or f32 rows for the average pool of a block with stride
      const bool direct = !stride && r3;
      if ((rc = prod(ws.t1, ws.pl1, pp, b.conv2, pp, 9 * pp, ws.t2, direct ? ws.pl2 : nullptr, M, ACX_ACT_RELU, nullptr, H, pp))) return rc;
      const float* a3f = ws.t2;
      const void* a3p = ws.pl2;
      const float* xin = ws.x;
      const void* xinp = ws.pl0;
      if (stride) {                                              // avgpool(stride) of the branch and of the identity's input
        if ((rc = acx_avgpool2_nhwc(ctx, ws.t2, ws.t1, n, H, H, pp, s))) return rc;
        if ((rc = acx_avgpool2_nhwc(ctx, ws.x, ws.p, n, H, H, cin_b, s))) return rc;
        a3f = ws.t1; xin = ws.p;
        if (r3) { if ((rc = rn_split(ctx, ws.t1, pp, ws.pl1, Mo, s))) return rc; }
        a3p = ws.pl1;
        if (rds) { if ((rc = rn_split(ctx, ws.p, cin_b, ws.pl0, Mo, s))) return rc; }
      } else if (!r3) {
        a3p = nullptr;
      }
      const float* ident = ws.x;
      if (b.downsample.w) {
        if ((rc = prod(xin, xinp, cin_b, b.downsample, cout, cin_b, ws.ds, nullptr, Mo, ACX_ACT_NONE, nullptr, 0, 0))) return rc;
        ident = ws.ds;
      } else if (stride || cin_b != cout) {
        return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_encode: a block that changes shape needs downsample weights%s");
      }
      if ((rc = prod(a3f, a3p, pp, b.conv3, cout, pp, ws.x, nullptr, Mo, ACX_ACT_RESRELU, ident, 0, 0))) return rc;
      H = Ho;
    }
    inpl = 4 * planes;
  }
  return rn_attnpool(ctx, w, g, ws, ws.x, n, features, s, true);
}

int rn_check(acx_ctx* ctx, const acx_resnet_desc* d) {
  // width % 8: every block's 4 * planes output (and so the next block's input) is a multiple of 32 channels, unpadded
  if (d->resolution <= 0 || d->resolution % 32 || d->width <= 0 || d->width % 8 || d->output_dim <= 0 || d->output_dim % 4)
    return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_encode: need resolution %% 32 == 0, width %% 8 == 0 and output_dim %% 4 == 0%s");
  for (int i = 0; i < 4; ++i)
    if (d->layers[i] <= 0) return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_encode: every layer needs >= 1 block%s");
  if (d->width * 32 != d->heads * 64) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_resnet_encode: head dim must be 64 (heads = width / 2)%s");
  const int Hf = d->resolution / 32;
  if (Hf * Hf + 1 > 1024) return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_resnet_encode: more than 1024 attention-pool tokens%s");
  // (the training-mode pass takes the same values and runs the f32 kernels for all of them)
  if (d->prec != ACX_PREC_F32 && d->prec != ACX_PREC_F32X6 && d->prec != ACX_PREC_BF16X6)
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_resnet_encode: ACX_PREC_F32 / ACX_PREC_F32X6 / ACX_PREC_BF16X6 only%s");
  return ACX_OK;
}

}  // namespace

extern "C" size_t acx_resnet_workspace_bytes(const acx_resnet_desc* d, int32_t frames) {
  if (!d || frames <= 0 || rn_check(nullptr, d)) return 0;
  const RnGeom g = rn_geom(d);
  const int fb = rn_batch(g);
  return rn_carve(nullptr, g, frames < fb ? frames : fb, d->prec == ACX_PREC_BF16X6).total;
}

extern "C" int acx_resnet_encode(acx_ctx* ctx, const acx_resnet_desc* d, const acx_resnet_weights* w, const float* frames,
                                 int32_t nframes, float* features, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !w || !frames || !features || !workspace || !w->blocks) return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_encode: null pointer%s");
  if (nframes <= 0) return ACX_OK;
  int rc;
  if ((rc = rn_check(ctx, d))) return rc;
  const RnGeom g = rn_geom(d);
  int fb = rn_batch(g);
  if (nframes < fb) fb = nframes;
  // batches of (nearly) equal size: ceil(nframes / fb) of them
  const int nb = (nframes + fb - 1) / fb;
  const int per = (nframes + nb - 1) / nb;
  const bool x6 = d->prec == ACX_PREC_BF16X6;
  const RnWs ws = rn_carve((char*)workspace, g, per, x6);
  if (ws.total > workspace_bytes) return acx_fail(ctx, ACX_E_WORKSPACE, "acx_resnet_encode: workspace too small (acx_resnet_workspace_bytes)%s");
  if (x6) {                                                      // the workspace is the caller's and holds anything: the zero page, every call
    if (((uintptr_t)workspace & 15)) return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_encode: ACX_PREC_BF16X6 needs a 16-byte aligned workspace%s");
    if (hipMemsetAsync(ws.zero, 0, 256, (hipStream_t)stream) != hipSuccess)
      return acx_fail(ctx, ACX_E_HIP, "acx_resnet_encode: clearing the zero page failed%s");
  }
  const int64_t fstride = (int64_t)3 * g.R * g.R;
  for (int f0 = 0; f0 < nframes; f0 += per) {
    const int n = nframes - f0 < per ? nframes - f0 : per;
    rc = x6 ? rn_encode_batch_x6(ctx, d, w, g, ws, frames + f0 * fstride, n, features + (int64_t)f0 * g.out, (hipStream_t)stream)
            : rn_encode_batch(ctx, d, w, g, ws, frames + f0 * fstride, n, features + (int64_t)f0 * g.out, (hipStream_t)stream);
    if (rc) return rc;
  }
  return ACX_OK;
}

// --------------------------------------------------------------------------------------------- training mode (BatchNorm2d.train())
// Lightning's model.train() leaves the frozen encoder's BatchNorms in training mode (anomaly_clip_module.py:68-69,160-166): every
// BatchNorm normalises with the statistics of ALL frames, H and W of the call and updates its running statistics.  So the call runs
// layer by layer over all its frames: each convolution's raw output (products in batches of at most rn_batch frames), then
// acx_bn_stats over all its rows, acx_bn_running_update, and acx_bn_apply_nhwc (scale / shift, + identity, ReLU) in place.
namespace {

struct RnTrainWs {
  RnWs b;                          // the eval carve for ALL frames (activations) -- tok / qkv / o used per batch
  float *mean, *var_b, *var_u, *scratch;
  void* bnws;
  size_t bnws_bytes, total;
};

RnTrainWs rn_carve_train(char* base, const RnGeom& g, int F) {
  RnTrainWs t;
  t.b = rn_carve(base, g, F, false);
  size_t off = t.b.total;
  const int cmax = g.E;                                          // widest BatchNorm: layer4's 4 * 8 width = 32 width
  auto take = [&](size_t bytes) { char* p = base + off; off += rn_al(bytes); return p; };
  t.mean = (float*)take((size_t)cmax * 4);
  t.var_b = (float*)take((size_t)cmax * 4);
  t.var_u = (float*)take((size_t)cmax * 4);
  t.scratch = (float*)take((size_t)2 * cmax * 4);
  const int64_t rows_max = (int64_t)F * g.G1 * g.G1;
  t.bnws_bytes = acx_bn_workspace_bytes(rows_max, cmax);
  const size_t narrow = acx_bn_workspace_bytes(rows_max, 64);
  if (narrow > t.bnws_bytes) t.bnws_bytes = narrow;
  t.bnws = take(t.bnws_bytes);
  t.total = off;
  return t;
}

// conv (no bias: the raw product into `out`) -> batch statistics -> running statistics -> y = act(bn(raw) (+ residual)) into y
// (y == out: in place)
int rn_conv_bn_train(acx_ctx* ctx, const RnTrainWs& t, const float* A, int lda, const float* W, int Np, int K, float* out,
                     int rows_per_frame, int F, int fb, int gh, int gw, int cin, const acx_resnet_bn& bn, int C, float eps,
                     float momentum, const float* residual, int relu, hipStream_t s, float* y = nullptr) {
  int rc;
  if (!W || !bn.weight || !bn.bias || !bn.running_mean || !bn.running_var)
    return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_encode_train: missing convolution or BatchNorm pointers%s");
  for (int f0 = 0; f0 < F; f0 += fb) {
    const int n = F - f0 < fb ? F - f0 : fb;
    const int64_t r0 = (int64_t)f0 * rows_per_frame;
    if ((rc = rn_gemm(ctx, A + r0 * lda, lda, W, Np, K, out + r0 * Np, Np, (int64_t)n * rows_per_frame, nullptr, ACX_ACT_NONE,
                      nullptr, gh, gw, cin, s))) return rc;
  }
  const int64_t rows = (int64_t)F * rows_per_frame;
  if ((rc = acx_bn_stats(ctx, out, rows, Np, t.mean, t.var_b, t.var_u, t.bnws, t.bnws_bytes, s))) return rc;
  if ((rc = acx_bn_running_update(ctx, t.mean, t.var_u, bn.running_mean, bn.running_var, bn.num_batches_tracked, C, momentum,
                                  1.f - momentum, s))) return rc;
  return acx_bn_apply_nhwc(ctx, out, t.mean, t.var_b, bn.weight, bn.bias, residual, y ? y : out, rows, C, Np, eps, relu, t.scratch, s);
}

}  // namespace

extern "C" size_t acx_resnet_train_workspace_bytes(const acx_resnet_desc* d, int32_t frames) {
  if (!d || frames <= 0 || rn_check(nullptr, d)) return 0;
  return rn_carve_train(nullptr, rn_geom(d), frames).total;
}

extern "C" int acx_resnet_encode_train(acx_ctx* ctx, const acx_resnet_desc* d, const acx_resnet_weights* w, const acx_resnet_train_bn* bn,
                                       const float* frames, int32_t F, float* features, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  if (!d || !w || !bn || !frames || !features || !workspace || !w->blocks || !bn->blocks)
    return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_encode_train: null pointer%s");
  if (F <= 0) return ACX_OK;
  int rc;
  if ((rc = rn_check(ctx, d))) return rc;
  const RnGeom g = rn_geom(d);
  const RnTrainWs t = rn_carve_train((char*)workspace, g, F);
  if (t.total > workspace_bytes) return acx_fail(ctx, ACX_E_WORKSPACE, "acx_resnet_encode_train: workspace too small (acx_resnet_train_workspace_bytes)%s");
  hipStream_t s = (hipStream_t)stream;
  const RnWs& ws = t.b;
  const float eps = bn->eps, mom = bn->momentum;
  int fb = rn_batch(g);
  if (F < fb) fb = F;
  const int c1 = rn_cp(g.w / 2), c2 = rn_cp(g.w), G = g.G1;
  // stem (clip/model.py:157-162)
  if ((rc = acx_resnet_stem_im2col(ctx, frames, ws.cols, F, g.R, s))) return rc;
  if ((rc = rn_conv_bn_train(ctx, t, ws.cols, 32, w->stem[0].w, c1, 32, ws.t1, G * G, F, fb, 0, 0, 0, bn->stem[0], g.w / 2, eps, mom,
                             nullptr, 1, s))) return rc;
  if ((rc = rn_conv_bn_train(ctx, t, ws.t1, c1, w->stem[1].w, c1, 9 * c1, ws.t2, G * G, F, fb, G, G, c1, bn->stem[1], g.w / 2, eps, mom,
                             nullptr, 1, s))) return rc;
  if ((rc = rn_conv_bn_train(ctx, t, ws.t2, c1, w->stem[2].w, c2, 9 * c1, ws.t1, G * G, F, fb, G, G, c1, bn->stem[2], g.w, eps, mom,
                             nullptr, 1, s))) return rc;
  if ((rc = acx_avgpool2_nhwc(ctx, ws.t1, ws.x, F, G, G, c2, s))) return rc;
  int H = G / 2, inpl = g.w, bi = 0;
  for (int li = 0; li < 4; ++li) {
    const int planes = g.w << li, pp = rn_cp(planes), cin = rn_cp(inpl), cout = 4 * planes;
    for (int j = 0; j < d->layers[li]; ++j, ++bi) {
      const acx_resnet_block& b = w->blocks[bi];
      const acx_resnet_block_bn& bb = bn->blocks[bi];
      const bool stride = li > 0 && j == 0;
      const int cin_b = j == 0 ? cin : cout;
      if ((rc = rn_conv_bn_train(ctx, t, ws.x, cin_b, b.conv1.w, pp, cin_b, ws.t1, H * H, F, fb, 0, 0, 0, bb.bn1, planes, eps, mom,
                                 nullptr, 1, s))) return rc;
      if ((rc = rn_conv_bn_train(ctx, t, ws.t1, pp, b.conv2.w, pp, 9 * pp, ws.t2, H * H, F, fb, H, H, pp, bb.bn2, planes, eps, mom,
                                 nullptr, 1, s))) return rc;
      const float* a3 = ws.t2;
      const float* xin = ws.x;
      float* raw3 = ws.t1;
      const int Ho = stride ? H / 2 : H;
      if (stride) {
        if ((rc = acx_avgpool2_nhwc(ctx, ws.t2, ws.t1, F, H, H, pp, s))) return rc;
        if ((rc = acx_avgpool2_nhwc(ctx, ws.x, ws.p, F, H, H, cin_b, s))) return rc;
        a3 = ws.t1; xin = ws.p; raw3 = ws.t2;
      }
      const float* ident = ws.x;
      if (b.downsample.w) {
        if ((rc = rn_conv_bn_train(ctx, t, xin, cin_b, b.downsample.w, cout, cin_b, ws.ds, Ho * Ho, F, fb, 0, 0, 0, bb.downsample, cout,
                                   eps, mom, nullptr, 0, s))) return rc;
        ident = ws.ds;
      } else if (stride || cin_b != cout) {
        return acx_fail(ctx, ACX_E_BADARG, "acx_resnet_encode_train: a block that changes shape needs downsample weights%s");
      }
      // relu(bn3(conv3) + identity): the raw product in a free buffer, then the apply pass writes the block output over x
      if ((rc = rn_conv_bn_train(ctx, t, a3, pp, b.conv3.w, cout, pp, raw3, Ho * Ho, F, fb, 0, 0, 0, bb.bn3, cout, eps, mom, ident,
                                 1, s, ws.x))) return rc;
      H = Ho;
    }
    inpl = 4 * planes;
  }
  for (int f0 = 0; f0 < F; f0 += fb) {
    const int n = F - f0 < fb ? F - f0 : fb;
    if ((rc = rn_attnpool(ctx, w, g, ws, ws.x + (int64_t)f0 * g.HW * g.E, n, features + (int64_t)f0 * g.out, s))) return rc;
  }
  return ACX_OK;
}
