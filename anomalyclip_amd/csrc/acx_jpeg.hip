// Baseline JPEG frames: the host entropy decoder (acx_jpeg_host.h) behind the C ABI, and the reconstruction of its coefficient
// blocks on the device -- dequantisation, libjpeg's integer "islow" inverse DCT, "fancy" chroma upsampling and the table-exact
// YCbCr -> RGB conversion, bit for bit what Pillow (libjpeg-turbo with its defaults) writes.
#include "acx_internal.h"
#include "acx_jpeg_host.h"
#include "acx_jpeg_sync.h"

extern "C" int acx_jpeg_parse(const uint8_t* data, size_t n, acx_jpeg_info* info) { return acx_jpeg::parse(data, n, info); }

extern "C" int acx_jpeg_entropy_decode(const uint8_t* data, size_t n, const acx_jpeg_info* info, int16_t* coef, size_t coef_elems) {
  return acx_jpeg::entropy_decode(data, n, info, coef, coef_elems);
}

// ---------------------------------------------------------------------------------------------------------------- geometry
// F frames of one geometry.  A frame's coefficients are component after component, each [blocks high][blocks wide][64] int16;
// its planes lie at the same offsets, each [blocks high * 8][blocks wide * 8] uint8 (a block's 64 coefficients become 64 bytes).
struct JpegGeom {
  uint32_t H, W, ncomp, hs, vs;      // hs, vs: the luma sampling factors (1 or 2); chroma is 1 x 1
  uint32_t bw0, bwc;                 // blocks per row of the luma / of a chroma plane
  uint32_t nb0, nbc;                 // blocks of the luma / of one chroma plane
  uint32_t nb;                       // blocks of a frame
  uint32_t dw, dh;                   // real samples of a chroma plane
};

static inline JpegGeom jpeg_geom(int32_t H, int32_t W, int32_t ncomp, int32_t hs, int32_t vs) {
  JpegGeom g;
  g.H = (uint32_t)H; g.W = (uint32_t)W; g.ncomp = (uint32_t)ncomp; g.hs = (uint32_t)hs; g.vs = (uint32_t)vs;
  const uint32_t mx = (g.W + 8 * g.hs - 1) / (8 * g.hs), my = (g.H + 8 * g.vs - 1) / (8 * g.vs);
  g.bw0 = mx * g.hs;
  g.bwc = mx;
  g.nb0 = g.bw0 * my * g.vs;
  g.nbc = ncomp == 3 ? mx * my : 0;
  g.nb = g.nb0 + 2 * g.nbc;
  g.dw = (g.W + g.hs - 1) / g.hs;
  g.dh = (g.H + g.vs - 1) / g.vs;
  return g;
}

// ---------------------------------------------------------------------------------------------------------------- inverse DCT
// libjpeg's jidctint ("islow"): CONST_BITS 13, PASS1_BITS 2; one 8-point pass, rounded and shifted right by S
template <int S>
__device__ __forceinline__ void idct8(const int (&x)[8], int (&y)[8]) {
  int z1 = (x[2] + x[6]) * 4433;
  const int t2 = z1 - x[6] * 15137, t3 = z1 + x[2] * 6270;
  const int t0 = (x[0] + x[4]) * 8192, t1 = (x[0] - x[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int o0 = x[7], o1 = x[5], o2 = x[3], o3 = x[1];
  z1 = o0 + o3;
  int z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const int z5 = (z3 + z4) * 9633;
  o0 *= 2446; o1 *= 16819; o2 *= 25172; o3 *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
  constexpr int R = 1 << (S - 1);
  y[0] = (t10 + o3 + R) >> S; y[7] = (t10 - o3 + R) >> S;
  y[1] = (t11 + o2 + R) >> S; y[6] = (t11 - o2 + R) >> S;
  y[2] = (t12 + o1 + R) >> S; y[5] = (t12 - o1 + R) >> S;
  y[3] = (t13 + o0 + R) >> S; y[4] = (t13 - o0 + R) >> S;
}

typedef short acx_i16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short acx_u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int acx_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int acx_u32x4 __attribute__((ext_vector_type(4)));

// One wave = 8 blocks, lane = (block, row or column); four waves per workgroup.  A lane reads row r of its block (16 bytes) and the
// quantisation row, and multiplies.  Pass 1 runs down the columns, so the products go through the wave's LDS tile once (row in,
// column out), pass 2 along the rows takes them back the other way, and the lane that holds row r writes its 8 samples.  A tile row
// is padded to 9 words: the 32 lanes of a half wave (4 blocks x 8) then hit 32 different banks both ways.
constexpr int IDCT_TILE = 8 * 72;     // words of one wave's tile: 8 blocks of 8 x 9

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const acx_i16x8* __restrict__ coef, const acx_u16x8* __restrict__ qtabs,
                                                        uint8_t* __restrict__ planes, JpegGeom g, uint32_t total_blocks) {
  __shared__ int tile[4 * IDCT_TILE];
  const uint32_t lane = threadIdx.x & 63, r = lane & 7;
  int* t = tile + (threadIdx.x >> 6) * IDCT_TILE + (lane >> 3) * 72;
  const uint32_t blk_raw = blockIdx.x * 32 + (threadIdx.x >> 3);
  const bool live = blk_raw < total_blocks;
  const uint32_t blk = live ? blk_raw : total_blocks - 1;          // past the end: redo the last block, store nothing
  const uint32_t f = blk / g.nb, b = blk - f * g.nb;
  uint32_t c = 0, local = b, bw = g.bw0;
  if (b >= g.nb0) {
    c = 1 + (b - g.nb0) / g.nbc;
    local = b - g.nb0 - (c - 1) * g.nbc;
    bw = g.bwc;
  }
  const acx_i16x8 cv = coef[(size_t)blk * 8 + r];
  const acx_u16x8 qv = qtabs[((size_t)f * g.ncomp + c) * 8 + r];
  int x[8], y[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) t[r * 9 + k] = (int)cv[k] * (int)qv[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = t[k * 9 + r];                 // column r
  __syncthreads();
  idct8<11>(x, y);
#pragma unroll
  for (int k = 0; k < 8; ++k) t[k * 9 + r] = y[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = t[r * 9 + k];                 // row r
  idct8<18>(x, y);
  uint32_t px[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) px[k] = (uint32_t)min(max(y[k] + 128, 0), 255);
  acx_u32x2 out;
  out.x = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
  out.y = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
  const uint32_t by = local / bw, bx = local - by * bw;
  const size_t comp_off = c == 0 ? 0 : ((size_t)g.nb0 + (size_t)(c - 1) * g.nbc) * 64;
  const size_t at = (size_t)f * g.nb * 64 + comp_off + ((size_t)by * 8 + r) * ((size_t)bw * 8) + (size_t)bx * 8;
  if (live) *(acx_u32x2*)(planes + at) = out;
}

// ---------------------------------------------------------------------------------------------------------------- upsample, colour
// the chroma sample of output pixel (y, x): libjpeg's "fancy" (triangle) upsampling; a neighbour beyond the plane's REAL edge
// (dw x dh samples; the plane is `ld` bytes wide, padded to whole blocks) is the edge sample
__device__ __forceinline__ int jpeg_chroma(const uint8_t* __restrict__ p, uint32_t ld, uint32_t dw, uint32_t dh, uint32_t hs, uint32_t vs,
                                           uint32_t y, uint32_t x) {
  if (hs == 1) return p[(size_t)y * ld + x];
  const uint32_t cx = x >> 1;
  const uint32_t cn = (x & 1) ? (cx + 1 < dw ? cx + 1 : cx) : (cx > 0 ? cx - 1 : 0);      // the nearer neighbour column
  if (vs == 1) {
    const uint8_t* row = p + (size_t)y * ld;
    return (3 * row[cx] + row[cn] + 1 + (int)(x & 1)) >> 2;
  }
  const uint32_t cy = y >> 1;
  const uint32_t rn = (y & 1) ? (cy + 1 < dh ? cy + 1 : cy) : (cy > 0 ? cy - 1 : 0);      // the nearer neighbour row
  const uint8_t* r0 = p + (size_t)cy * ld;
  const uint8_t* r1 = p + (size_t)rn * ld;
  const int s = 3 * r0[cx] + r1[cx], sn = 3 * r0[cn] + r1[cn];
  return (3 * s + sn + 8 - (int)(x & 1)) >> 4;
}

// A thread makes 16 consecutive pixels of the flat [F * H * W] pixel array: 48 bytes, three 16-byte stores at a 16-byte aligned
// offset whatever W is (the pixels may run over a row's or a frame's end: the position is stepped, not divided, per pixel).  The
// last thread of a batch whose pixel count is no multiple of 16 stores its pixels byte by byte.
__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ rgb, JpegGeom g,
                                                          uint32_t total_pixels) {
  const uint32_t p0 = (blockIdx.x * 256 + threadIdx.x) * 16;
  if (p0 >= total_pixels) return;
  const uint32_t hw = g.H * g.W;
  uint32_t f = p0 / hw;
  const uint32_t rem = p0 - f * hw;
  uint32_t y = rem / g.W, x = rem - y * g.W;
  const size_t frame_bytes = (size_t)g.nb * 64;
  const uint32_t ld0 = g.bw0 * 8, ldc = g.bwc * 8;
  const size_t cb_off = (size_t)g.nb0 * 64, cr_off = cb_off + (size_t)g.nbc * 64;
  uint32_t w[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) w[k] = 0;
  const uint32_t n = total_pixels - p0 < 16 ? total_pixels - p0 : 16;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    if ((uint32_t)i < n) {
      const uint8_t* fp = planes + (size_t)f * frame_bytes;
      const int Y = fp[(size_t)y * ld0 + x];
      int R = Y, G = Y, B = Y;
      if (g.ncomp == 3) {
        const int cb = jpeg_chroma(fp + cb_off, ldc, g.dw, g.dh, g.hs, g.vs, y, x) - 128;
        const int cr = jpeg_chroma(fp + cr_off, ldc, g.dw, g.dh, g.hs, g.vs, y, x) - 128;
        R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
        G = min(max(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16), 0), 255);
        B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
      }
      w[(3 * i) >> 2] |= (uint32_t)R << (8 * ((3 * i) & 3));
      w[(3 * i + 1) >> 2] |= (uint32_t)G << (8 * ((3 * i + 1) & 3));
      w[(3 * i + 2) >> 2] |= (uint32_t)B << (8 * ((3 * i + 2) & 3));
      if (++x == g.W) {
        x = 0;
        if (++y == g.H) {
          y = 0;
          ++f;
        }
      }
    }
  }
  uint8_t* dst = rgb + (size_t)p0 * 3;
  if (n == 16) {
    acx_u32x4* d4 = (acx_u32x4*)dst;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      acx_u32x4 v;
      v.x = w[4 * k]; v.y = w[4 * k + 1]; v.z = w[4 * k + 2]; v.w = w[4 * k + 3];
      d4[k] = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 45; ++k)
      if ((uint32_t)k < 3 * n) dst[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  }
}

extern "C" int acx_jpeg_reconstruct(acx_ctx* ctx, const int16_t* coef, const uint16_t* qtabs, int32_t H, int32_t W, int32_t ncomp,
                                    int32_t hs, int32_t vs, int32_t F, uint8_t* planes, uint8_t* rgb, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (F == 0) return ACX_OK;
  if (!coef || !qtabs || !planes || !rgb) return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_reconstruct: null pointer%s");
  if (F < 0 || H < 1 || W < 1 || H > 65535 || W > 65535)
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_reconstruct: F >= 0 and 1 <= H, W <= 65535%s");
  if (!((ncomp == 1 && hs == 1 && vs == 1) || (ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2))))))
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_jpeg_reconstruct: 1 component, or 3 with luma sampling 1x1, 2x1 or 2x2%s");
  if (hs == 2 && (W + 1) / 2 <= 2)      // (libjpeg replicates such a plane's samples instead of filtering them)
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_jpeg_reconstruct: a downsampled chroma plane of one or two samples per row%s");
  if ((((uintptr_t)coef | (uintptr_t)qtabs | (uintptr_t)rgb) & 15) || ((uintptr_t)planes & 7))
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_reconstruct: coef, qtabs and rgb 16-byte aligned, planes 8-byte aligned%s");
  const JpegGeom g = jpeg_geom(H, W, ncomp, hs, vs);
  const int64_t blocks = (int64_t)F * g.nb, pixels = (int64_t)F * H * W;
  if (blocks > INT32_MAX || pixels > INT32_MAX)
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_reconstruct: F * blocks and F * H * W must stay below 2^31 (split the batch)%s");
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((blocks + 31) / 32)), dim3(256), 0, (hipStream_t)stream, (const acx_i16x8*)coef,
                     (const acx_u16x8*)qtabs, planes, g, (uint32_t)blocks);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_reconstruct (idct)");
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((pixels + 4095) / 4096)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)planes, rgb, g, (uint32_t)pixels);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_reconstruct (colour)");
  return ACX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- entropy decoding
extern "C" int acx_jpeg_scan_pack(const uint8_t* data, size_t n, const acx_jpeg_info* info, uint8_t* dst, size_t cap,
                                  int64_t* payload_bytes, acx_jpeg_huff* huff) {
  return acx_jpeg::scan_pack(data, n, info, dst, cap, payload_bytes, huff);
}

static_assert(sizeof(acx_jpeg_huff) == acx_jsync::kHuffBytes, "acx_jpeg_huff is the record acx_jpeg_sync.h reads");
static_assert(ACX_JPEG_MAX_SUBSEQ == acx_jsync::kThreads, "one thread per subsequence");
static_assert(sizeof(acx_jsync::Shared) <= 48 * 1024, "the tables and the records stay well inside the 64 KB a launch gets");

// One workgroup per frame, thread t owns subsequence t: the phases of acx_jpeg_sync.h with the workgroup's barriers between them.
// A frame whose scan, offset or tables are not usable is a status, decided by values every thread of the workgroup sees alike.
__global__ __launch_bounds__(1024) void jpeg_entropy_kernel(const uint8_t* __restrict__ scans, int64_t scans_bytes,
                                                            const int64_t* __restrict__ scan_off, const int32_t* __restrict__ scan_bits,
                                                            const uint8_t* __restrict__ huff, acx_jsync::Geo g, uint32_t sub_arg,
                                                            int16_t* __restrict__ coef, int32_t* __restrict__ status) {
  using namespace acx_jsync;
  __shared__ Shared S;
  __shared__ int s_bad;
  const uint32_t t = threadIdx.x, f = blockIdx.x;
  const int64_t off = scan_off[f], bits64 = scan_bits[f];
  const uint8_t* hf = huff + (size_t)f * kHuffBytes;
  const uint32_t sub = sub_arg ? sub_arg : min_sub_bits(bits64 < 0 ? 0 : (uint64_t)bits64);
  bool ok = bits64 >= 0 && off >= 0 && (off & 31) == 0 && (uint64_t)sub * kThreads >= (uint64_t)bits64 &&
            (off >> 3) + (bits64 + 31) / 32 * 4 <= scans_bytes;
  uint32_t used = 0, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
#pragma unroll
  for (uint32_t c = 0; c < 3; ++c)
    if (c < g.ncomp) {
      td[c] = hf[kHuffTd + c];
      ta[c] = hf[kHuffTa + c];
      ok = ok && td[c] < 4 && ta[c] < 4;
      td[c] &= 3;
      ta[c] &= 3;
      ok = ok && hf[kHuffPresent + td[c]] && hf[kHuffPresent + 4 + ta[c]];
      used |= (1u << td[c]) | (16u << ta[c]);
    }
  if (!ok) {
    if (t == 0) status[f] = kBad;
    return;
  }
  const uint32_t bits = (uint32_t)bits64;
  const uint32_t nsub = bits == 0 ? 1u : (bits + sub - 1) / sub;           // <= kThreads

  for (uint32_t i = t; i < 8 * 512; i += kThreads) S.tab[i >> 9].look[i & 511] = 0;
  for (uint32_t i = t; i < 8 * 256; i += kThreads) S.tab[i >> 8].vals[i & 255] = hf[kHuffVals + i];
  if (t == 0) {
    s_bad = 0;
    S.err = S.done = 0;
  }
  if (t < 3) {
    S.sel[0][t] = t == 0 ? td[0] : t == 1 ? td[1] : td[2];
    S.sel[1][t] = 4 + (t == 0 ? ta[0] : t == 1 ? ta[1] : ta[2]);
  }
  S.pos[t] = 0;
  S.bk[t] = 0;
  S.nblk[t] = 0;
  S.dc[0][t] = S.dc[1][t] = S.dc[2][t] = 0;
  __syncthreads();
  if (t < 8 && ((used >> t) & 1))
    if (derive_codes(hf + kHuffBits + t * 17, &S.tab[t]) != 0) s_bad = 1;
  __syncthreads();
  if (s_bad) {
    if (t == 0) status[f] = kBad;
    return;
  }

  Scan sc;
  scan_init(&sc, (const uint32_t*)(scans + (off >> 3)), bits);
  State st = {0, 0, 0};
  bool active = t < nsub;
  if (active) phase_speculate(S, g, sc, t, sub, st);
  __syncthreads();
  for (uint32_t r = 1; r < nsub; ++r) {                                    // nsub is the workgroup's: every thread takes the barrier
    const bool changed = phase_sync_round(S, g, sc, t, r, sub, nsub, st, active);
    if (!__syncthreads_or(changed ? 1 : 0)) break;
  }
  __syncthreads();
  for (uint32_t d = 1; d < kThreads; d <<= 1) {                            // inclusive scans of the counts over the records
    uint32_t a = 0;
    uint32_t b0 = 0, b1 = 0, b2 = 0;
    if (t >= d) {
      a = S.nblk[t - d];
      b0 = S.dc[0][t - d];
      b1 = S.dc[1][t - d];
      b2 = S.dc[2][t - d];
    }
    __syncthreads();
    S.nblk[t] += a;
    S.dc[0][t] += b0;
    S.dc[1][t] += b1;
    S.dc[2][t] += b2;
    __syncthreads();
  }
  if (t < nsub) phase_write(S, g, sc, t, sub, coef + (size_t)f * g.coef_elems);
  __syncthreads();
  if (t == 0) status[f] = (S.err || !S.done) ? kBad : 0;
}

extern "C" int acx_jpeg_entropy_decode_dev(acx_ctx* ctx, const uint8_t* scans, int64_t scans_bytes, const int64_t* scan_off,
                                           const int32_t* scan_bits, const acx_jpeg_huff* huff, int32_t H, int32_t W, int32_t ncomp,
                                           int32_t hs, int32_t vs, int32_t F, int64_t max_scan_bits, int32_t sub_bits, int16_t* coef,
                                           int32_t* status, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (F == 0) return ACX_OK;
  if (!scans || !scan_off || !scan_bits || !huff || !coef || !status)
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_decode_dev: null pointer%s");
  if (F < 0 || H < 1 || W < 1 || H > 65535 || W > 65535)
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_decode_dev: F >= 0 and 1 <= H, W <= 65535%s");
  if (!((ncomp == 1 && hs == 1 && vs == 1) || (ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2))))))
    return acx_fail(ctx, ACX_E_UNSUPPORTED, "acx_jpeg_entropy_decode_dev: 1 component, or 3 with luma sampling 1x1, 2x1 or 2x2%s");
  acx_jsync::Geo g;
  if (!acx_jsync::make_geo(H, W, ncomp, hs, vs, &g))
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_decode_dev: a frame's coefficients must stay below 2^31%s");
  if (scans_bytes < 0 || max_scan_bits < 0 || max_scan_bits > 0x7FFF0000ll || (max_scan_bits + 7) / 8 > scans_bytes)
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_decode_dev: 0 <= max_scan_bits <= 8 * scans_bytes, below 2^31%s");
  if (sub_bits < 0 || (sub_bits & 31))
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_decode_dev: sub_bits is a multiple of 32, or 0 for each frame's smallest%s");
  if (sub_bits && (int64_t)sub_bits * acx_jsync::kThreads < max_scan_bits)
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_decode_dev: %ssub_bits %ld does not cover the longest scan with 1024 subsequences: needs %ld",
                    "", (long)sub_bits, (long)acx_jsync::min_sub_bits((uint64_t)max_scan_bits));
  if (((uintptr_t)scans & 3) || ((uintptr_t)scan_off & 7) || ((uintptr_t)scan_bits & 3) || ((uintptr_t)coef & 1) || ((uintptr_t)status & 3))
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_decode_dev: scans 4-byte aligned, the arrays aligned to their element%s");
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)F), dim3(acx_jsync::kThreads), 0, (hipStream_t)stream, scans, scans_bytes, scan_off,
                     scan_bits, (const uint8_t*)huff, g, (uint32_t)sub_bits, coef, status);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_entropy_decode_dev");
  return ACX_OK;
}
