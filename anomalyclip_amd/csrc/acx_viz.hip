// The qualitative videos (data.visualize=True; reference src/utils/visualizer.py): the per-frame picture composed on the device, and
// the forward half of a baseline JPEG encoder -- colour conversion, 2x2 chroma mean, forward DCT and quantisation into the
// coefficient layout the decoder of acx_jpeg.hip reads.  Huffman coding is the host's (acx_jpeg_enc_host.h), behind the C ABI here,
// or the device's (acx_jpeg_enc.hip).
#include "acx_internal.h"
#include "acx_jpeg_enc_host.h"

extern "C" int64_t acx_jpeg_encode_bound(int32_t H, int32_t W) { return acx_jpeg::encode_bound(H, W); }

extern "C" int64_t acx_jpeg_entropy_encode(const int16_t* coef, size_t coef_elems, const uint16_t* qtabs, int32_t H, int32_t W,
                                           uint8_t* dst, size_t cap) {
  return acx_jpeg::entropy_encode(coef, coef_elems, qtabs, H, W, dst, cap);
}

namespace {

typedef unsigned int viz_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int viz_u32x4 __attribute__((ext_vector_type(4)));
typedef short viz_i16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short viz_u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ unsigned char viz_clip8_22(int v) {
  v >>= 22;
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---------------------------------------------------------------------------------------------------------------- composition
// every canvas starts as the video's static layer: 16 bytes per thread where a canvas is a whole number of them
template <bool VEC>
__global__ __launch_bounds__(256) void viz_static_kernel(const uint8_t* __restrict__ layer, uint8_t* __restrict__ canvases, int64_t bytes) {
  const int64_t at = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  if (at >= bytes) return;
  uint8_t* dst = canvases + (int64_t)blockIdx.y * bytes + at;
  if (VEC) {
    *(viz_u32x4*)dst = *(const viz_u32x4*)(layer + at);
  } else {
    const int n = bytes - at < 16 ? (int)(bytes - at) : 16;
    for (int k = 0; k < n; ++k) dst[k] = layer[at + k];
  }
}

// Pillow's two-pass 8-bit resampler (the arithmetic of acx_preprocess_frames' two-kernel route), here with the triangle filter's
// tables: tmp[b][y][xo][c] = clip8(0.5 + sum_x in[b][y][xmin + x][c] * k[xo][x]).  A thread makes the three channels of one pixel.
// Table entries are clamped to the source: whatever the tables hold, no read leaves the frame.
__global__ __launch_bounds__(256) void viz_resize_h_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ tmp,
                                                           const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                           int64_t total, int W, int fw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int xo = (int)(i % fw);
  const int64_t row = i / fw;                                           // b * H + y
  const int xmin = min(max(bounds[2 * xo], 0), W - 1), xn = min(min(bounds[2 * xo + 1], ksize), W - xmin);
  const uint8_t* p = in + (row * W + xmin) * 3;
  const int* k = kk + (int64_t)xo * ksize;
  int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
  for (int x = 0; x < xn; ++x) {
    const int c = k[x];
    a0 += (int)p[3 * x] * c;
    a1 += (int)p[3 * x + 1] * c;
    a2 += (int)p[3 * x + 2] * c;
  }
  uint8_t* q = tmp + i * 3;
  q[0] = viz_clip8_22(a0);
  q[1] = viz_clip8_22(a1);
  q[2] = viz_clip8_22(a2);
}

// canvas[b][fy + yo][fx + xo][c] = clip8(0.5 + sum_y tmp[b][ymin + y][xo][c] * k[yo][y])
__global__ __launch_bounds__(256) void viz_resize_v_kernel(const uint8_t* __restrict__ tmp, uint8_t* __restrict__ canvases,
                                                           const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                           acx_viz_geom g) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= g.fw * g.fh) return;
  const int yo = i / g.fw, xo = i - yo * g.fw;
  const int64_t b = blockIdx.y;
  const int ymin = min(max(bounds[2 * yo], 0), g.H - 1), yn = min(min(bounds[2 * yo + 1], ksize), g.H - ymin);
  const int64_t ld = (int64_t)g.fw * 3;
  const uint8_t* p = tmp + ((b * g.H + ymin) * g.fw + xo) * 3;
  const int* k = kk + (int64_t)yo * ksize;
  int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
  for (int y = 0; y < yn; ++y) {
    const int c = k[y];
    a0 += (int)p[y * ld] * c;
    a1 += (int)p[y * ld + 1] * c;
    a2 += (int)p[y * ld + 2] * c;
  }
  uint8_t* q = canvases + ((b * g.Hc + g.fy + yo) * g.Wc + g.fx + xo) * 3;
  q[0] = viz_clip8_22(a0);
  q[1] = viz_clip8_22(a1);
  q[2] = viz_clip8_22(a2);
}

__device__ __forceinline__ void viz_put(uint8_t* cv, const acx_viz_geom& g, int x, int y, int r, int gr, int bl) {
  uint8_t* q = cv + ((int64_t)y * g.Wc + x) * 3;
  q[0] = (uint8_t)r;
  q[1] = (uint8_t)gr;
  q[2] = (uint8_t)bl;
}

// The border around the frame, the bars and the cursor of canvas blockIdx.y; the workgroups of a canvas share its pixels out.
// Bar k is h_k = floor(p_k * PH + 0.5) rows high, in float32 with a rounded product and a rounded sum (no fused multiply-add:
// numpy's float32 gives the same integer), clipped to 0 .. PH.  The three largest p_k (the lower index wins a tie) are red where
// the score is not below the threshold.
__global__ __launch_bounds__(256) void viz_overlay_kernel(uint8_t* __restrict__ canvases, const float* __restrict__ scores,
                                                          const float* __restrict__ softmax, const int* __restrict__ frame_idx,
                                                          acx_viz_geom g) {
  __shared__ int s_h[64];
  __shared__ int s_top[3];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.y;
  const float score = scores[b];
  const float* p = softmax + b * g.C1;
  if (t < g.C1) {
    const float v = __fadd_rn(__fmul_rn(p[t], (float)g.bh), 0.5f);
    s_h[t] = v >= 1.f ? (v >= (float)g.bh ? g.bh : (int)v) : 0;
  }
  if (t == 0) {
    int i0 = -1, i1 = -1, i2 = -1;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    for (int k = 0; k < g.C1; ++k) {
      const float v = p[k];
      if (i0 < 0 || v > v0) {
        i2 = i1; v2 = v1; i1 = i0; v1 = v0; i0 = k; v0 = v;
      } else if (i1 < 0 || v > v1) {
        i2 = i1; v2 = v1; i1 = k; v1 = v;
      } else if (i2 < 0 || v > v2) {
        i2 = k; v2 = v;
      }
    }
    s_top[0] = i0; s_top[1] = i1; s_top[2] = i2;
  }
  __syncthreads();
  uint8_t* cv = canvases + b * g.Hc * g.Wc * 3;
  const int step = gridDim.x * 256, first = blockIdx.x * 256 + t;
  // the border: two strips over the whole outer width, two beside the frame
  const int ow = g.fw + 2 * g.border, n_tb = ow * g.border, n_lr = g.border * g.fh;
  const int below = score < g.threshold;
  const int br = below ? 0 : 255, bb = below ? 255 : 0;
  for (int i = first; i < 2 * (n_tb + n_lr); i += step) {
    int x, y;
    if (i < 2 * n_tb) {
      const int j = i < n_tb ? i : i - n_tb;
      y = (i < n_tb ? g.fy - g.border : g.fy + g.fh) + j / ow;
      x = g.fx - g.border + j % ow;
    } else {
      const int i2 = i - 2 * n_tb, j = i2 < n_lr ? i2 : i2 - n_lr;
      x = (i2 < n_lr ? g.fx - g.border : g.fx + g.fw) + j % g.border;
      y = g.fy + j / g.border;
    }
    viz_put(cv, g, x, y, br, 0, bb);
  }
  // the bars
  const bool hot = score >= g.threshold;
  const int per = g.bar_w * g.bh;
  for (int i = first; i < g.C1 * per; i += step) {
    const int k = i / per, r = i - k * per, yy = r / g.bar_w, xx = r - yy * g.bar_w;
    if (yy < g.bh - s_h[k]) continue;
    const bool red = hot && (k == s_top[0] || k == s_top[1] || k == s_top[2]);
    viz_put(cv, g, g.bx + k * g.bar_pitch + xx, g.by + yy, red ? 255 : 128, red ? 0 : 128, red ? 0 : 128);
  }
  // the cursor
  const int fi = frame_idx[b];
  if (fi >= 0 && fi < g.T) {
    const int x0 = g.sx + (int)(((int64_t)fi * (g.sw - 1)) / g.T);
    for (int i = first; i < g.cursor_w * g.sh; i += step) viz_put(cv, g, x0 + i % g.cursor_w, g.sy + i / g.cursor_w, 255, 0, 0);
  }
}

// ---------------------------------------------------------------------------------------------------------------- forward JPEG
// The 8-point DCT as a fixed-point matrix: C[u][x] = round(2^14 * a(u) * cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2 --
// the orthonormal basis, so that a pass keeps the scale of its input.
constexpr int kVizCos[8] = {8192, 8035, 7568, 6811, 5793, 4551, 3135, 1598};      // round(8192 cos(k pi / 16))
constexpr int viz_dct_c(int u, int x) {
  if (u == 0) return 5793;
  int m = ((2 * x + 1) * u) & 31, sgn = 1;
  if (m > 16) m = 32 - m;
  if (m > 8) {
    m = 16 - m;
    sgn = -1;
  }
  return m == 8 ? 0 : sgn * kVizCos[m];
}

// y[u] = (sum_x C[u][x] x[x] + 2^13) >> 14
__device__ __forceinline__ void viz_dct8(const int (&x)[8], int (&y)[8]) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    int acc = 1 << 13;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += viz_dct_c(u, k) * x[k];
    y[u] = acc >> 14;
  }
}

__device__ __forceinline__ int viz_byte(const unsigned (&w)[12], int j) { return (int)((w[j >> 2] >> (8 * (j & 3))) & 255u); }

struct VizJpegGeom {
  uint32_t Hc, Wc;
  uint32_t bw0, bwc;                 // blocks per row of the luma / of a chroma plane
  uint32_t nb0, nbc, nb;             // blocks of the luma, of one chroma plane, of a frame
};

constexpr int VIZ_TILE = 8 * 72;     // words of one wave's tile: 8 blocks of 8 x 9 (acx_jpeg.hip's inverse transform, the other way)

// One wave = 8 blocks, lane = (block, row r).  The lane reads row r of its block from the canvas (24 bytes of a luma block; two
// rows of 48 bytes of a chroma block, which covers 16 x 16 pixels), converts to samples with 6 fraction bits, transforms its row,
// and the block goes through the wave's LDS tile to be transformed down the columns and back to be quantised and stored by rows.
__global__ __launch_bounds__(256) void jpeg_forward_kernel(const uint8_t* __restrict__ canvases, const viz_u16x8* __restrict__ qtabs,
                                                           viz_i16x8* __restrict__ coef, VizJpegGeom g, uint64_t total_blocks) {
  __shared__ int tile[4 * VIZ_TILE];
  const uint32_t lane = threadIdx.x & 63, r = lane & 7;
  int* t = tile + (threadIdx.x >> 6) * VIZ_TILE + (lane >> 3) * 72;
  const uint64_t blk_raw = (uint64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  const bool live = blk_raw < total_blocks;
  const uint64_t blk = live ? blk_raw : total_blocks - 1;          // past the end: redo the last block, store nothing
  const uint64_t f = blk / g.nb;
  const uint32_t b = (uint32_t)(blk - f * g.nb);
  uint32_t c = 0, local = b, bw = g.bw0;
  if (b >= g.nb0) {
    c = 1 + (b - g.nb0) / g.nbc;
    local = b - g.nb0 - (c - 1) * g.nbc;
    bw = g.bwc;
  }
  const uint32_t by = local / bw, bx = local - by * bw;
  const uint8_t* frame = canvases + f * g.Hc * g.Wc * 3;
  int x[8], y[8];
  unsigned w[12];
  if (c == 0) {
    const viz_u32x2* src = (const viz_u32x2*)(frame + ((uint64_t)(by * 8 + r) * g.Wc + bx * 8) * 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const viz_u32x2 v = src[k];
      w[2 * k] = v.x;
      w[2 * k + 1] = v.y;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int R = viz_byte(w, 3 * k), G = viz_byte(w, 3 * k + 1), B = viz_byte(w, 3 * k + 2);
      x[k] = (19595 * R + 38470 * G + 7471 * B - (128 << 16) + 512) >> 10;
    }
  } else {
    const int kr = c == 1 ? -11059 : 32768, kg = c == 1 ? -21709 : -27439, kb = c == 1 ? 32768 : -5329;
    int acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
      const viz_u32x4* src = (const viz_u32x4*)(frame + ((uint64_t)(by * 16 + 2 * r + row) * g.Wc + bx * 16) * 3);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const viz_u32x4 v = src[k];
        w[4 * k] = v.x;
        w[4 * k + 1] = v.y;
        w[4 * k + 2] = v.z;
        w[4 * k + 3] = v.w;
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k >> 1] += kr * viz_byte(w, 3 * k) + kg * viz_byte(w, 3 * k + 1) + kb * viz_byte(w, 3 * k + 2);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = (acc[k] + 2048) >> 12;
  }
  viz_dct8(x, y);                                                    // along the row: y[u]
#pragma unroll
  for (int k = 0; k < 8; ++k) t[r * 9 + k] = y[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = t[k * 9 + r];                   // column u = r
  __syncthreads();
  viz_dct8(x, y);                                                    // down the column: y[v]
#pragma unroll
  for (int k = 0; k < 8; ++k) t[k * 9 + r] = y[k];
  __syncthreads();
  const viz_u16x8 qv = qtabs[(c ? 8 : 0) + r];
  viz_i16x8 out;
#pragma unroll
  for (int k = 0; k < 8; ++k) {                                      // row v = r of the coefficients, 6 fraction bits
    const int v = t[r * 9 + k];
    const unsigned q64 = (unsigned)qv[k] * 64u, a = (unsigned)(v < 0 ? -v : v);
    int n = (int)((a + (q64 >> 1)) / q64);
    n = n > 1023 ? 1023 : n;
    out[k] = (short)(v < 0 ? -n : n);
  }
  if (live) coef[blk * 8 + r] = out;
}

}  // namespace

extern "C" int acx_viz_compose(acx_ctx* ctx, const uint8_t* static_layer, const uint8_t* frames, const float* scores,
                               const float* softmax, const int32_t* frame_idx, const int32_t* hbounds, const int32_t* hcoef,
                               int32_t hksize, const int32_t* vbounds, const int32_t* vcoef, int32_t vksize, const acx_viz_geom* geom,
                               int32_t B, uint8_t* tmp, uint8_t* canvases, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (B == 0) return ACX_OK;
  if (!static_layer || !frames || !scores || !softmax || !frame_idx || !hbounds || !hcoef || !vbounds || !vcoef || !geom || !tmp ||
      !canvases)
    return acx_fail(ctx, ACX_E_BADARG, "acx_viz_compose: null pointer%s");
  const acx_viz_geom g = *geom;
  if (B < 0 || B > 65535 || g.Hc < 1 || g.Wc < 1 || g.Hc > 65535 || g.Wc > 65535 || g.H < 1 || g.W < 1 || g.H > 65535 || g.W > 65535)
    return acx_fail(ctx, ACX_E_BADARG, "acx_viz_compose: 0 <= B <= 65535 and canvas and source sizes in 1 .. 65535%s");
  if (g.C1 < 1 || g.C1 > 64) return acx_fail(ctx, ACX_E_BADARG, "acx_viz_compose: 1 <= C1 <= 64%s");
  if (hksize < 1 || vksize < 1 || g.T < 1) return acx_fail(ctx, ACX_E_BADARG, "acx_viz_compose: table widths and T are positive%s");
  // every rectangle lies strictly inside the canvas: one that touches its edge is refused, not clipped
  auto inside = [&](int64_t x0, int64_t y0, int64_t x1, int64_t y1) { return x0 > 0 && y0 > 0 && x0 < x1 && y0 < y1 && x1 < g.Wc && y1 < g.Hc; };
  if (g.border < 1 || g.fw < 1 || g.fh < 1 ||
      !inside((int64_t)g.fx - g.border, (int64_t)g.fy - g.border, (int64_t)g.fx + g.fw + g.border, (int64_t)g.fy + g.fh + g.border))
    return acx_fail(ctx, ACX_E_BADARG, "acx_viz_compose: the frame rectangle and its border must lie inside the canvas%s");
  if (g.bar_w < 1 || g.bar_pitch < g.bar_w || g.bh < 1 ||
      !inside(g.bx, g.by, (int64_t)g.bx + (int64_t)(g.C1 - 1) * g.bar_pitch + g.bar_w, (int64_t)g.by + g.bh))
    return acx_fail(ctx, ACX_E_BADARG, "acx_viz_compose: the bars must lie inside the canvas%s");
  if (g.cursor_w < 1 || g.sw < 2 || g.sh < 1 || !inside(g.sx, g.sy, (int64_t)g.sx + g.sw - 2 + g.cursor_w, (int64_t)g.sy + g.sh) ||
      (int64_t)g.sx + g.sw >= g.Wc)
    return acx_fail(ctx, ACX_E_BADARG, "acx_viz_compose: the score panel and its cursor must lie inside the canvas%s");
  hipStream_t s = (hipStream_t)stream;
  const int64_t bytes = (int64_t)g.Hc * g.Wc * 3;
  const dim3 cgrid((unsigned)((bytes + 4095) / 4096), (unsigned)B);
  if (bytes % 16 == 0 && !(((uintptr_t)static_layer | (uintptr_t)canvases) & 15))
    hipLaunchKernelGGL(viz_static_kernel<true>, cgrid, dim3(256), 0, s, static_layer, canvases, bytes);
  else
    hipLaunchKernelGGL(viz_static_kernel<false>, cgrid, dim3(256), 0, s, static_layer, canvases, bytes);
  ACX_CHECK_LAUNCH(ctx, "acx_viz_compose (static layer)");
  const int64_t t1 = (int64_t)B * g.H * g.fw;
  if ((t1 + 255) / 256 > INT32_MAX) return acx_fail(ctx, ACX_E_BADARG, "acx_viz_compose: B * H * fw beyond a launch (split the batch)%s");
  hipLaunchKernelGGL(viz_resize_h_kernel, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, s, frames, tmp, hbounds, hcoef, hksize, t1, g.W,
                     g.fw);
  ACX_CHECK_LAUNCH(ctx, "acx_viz_compose (horizontal pass)");
  const int64_t t2 = (int64_t)g.fw * g.fh;
  if (t2 > INT32_MAX - 256) return acx_fail(ctx, ACX_E_BADARG, "acx_viz_compose: the frame rectangle is too large%s");
  hipLaunchKernelGGL(viz_resize_v_kernel, dim3((unsigned)((t2 + 255) / 256), (unsigned)B), dim3(256), 0, s, (const uint8_t*)tmp, canvases,
                     vbounds, vcoef, vksize, g);
  ACX_CHECK_LAUNCH(ctx, "acx_viz_compose (vertical pass)");
  hipLaunchKernelGGL(viz_overlay_kernel, dim3(32, (unsigned)B), dim3(256), 0, s, canvases, scores, softmax, frame_idx, g);
  ACX_CHECK_LAUNCH(ctx, "acx_viz_compose (overlay)");
  return ACX_OK;
}

extern "C" int acx_jpeg_forward(acx_ctx* ctx, const uint8_t* canvases, const uint16_t* qtabs, int32_t Hc, int32_t Wc, int32_t B,
                                int16_t* coef, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (B == 0) return ACX_OK;
  if (!canvases || !qtabs || !coef) return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_forward: null pointer%s");
  if (B < 0 || Hc < 16 || Wc < 16 || Hc > 65520 || Wc > 65520 || (Hc & 15) || (Wc & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_forward: B >= 0; Hc and Wc multiples of 16 in 16 .. 65520%s");
  if (((uintptr_t)canvases | (uintptr_t)qtabs | (uintptr_t)coef) & 15)
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_forward: canvases, qtabs and coef 16-byte aligned%s");
  VizJpegGeom g;
  g.Hc = (uint32_t)Hc;
  g.Wc = (uint32_t)Wc;
  g.bw0 = g.Wc / 8;
  g.bwc = g.Wc / 16;
  g.nb0 = g.bw0 * (g.Hc / 8);
  g.nbc = g.bwc * (g.Hc / 16);
  g.nb = g.nb0 + 2 * g.nbc;
  const uint64_t blocks = (uint64_t)B * g.nb;
  if ((blocks + 31) / 32 > (uint64_t)INT32_MAX) return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_forward: B * blocks beyond a launch (split the batch)%s");
  hipLaunchKernelGGL(jpeg_forward_kernel, dim3((unsigned)((blocks + 31) / 32)), dim3(256), 0, (hipStream_t)stream, canvases,
                     (const viz_u16x8*)qtabs, (viz_i16x8*)coef, g, blocks);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_forward");
  return ACX_OK;
}
