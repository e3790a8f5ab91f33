// Training batches and test-mode tiles out of a feature set resident in HBM (anomalyclip_amd/feature_bank.py): one gather launch per
// batch / per group of videos.
#include "acx_internal.h"

// out[b, c, n*L + l, :] = bank[row_off[vid[b]] + ((starts[b*N + n] + l*stride) mod frames[vid[b]]) * ncrops + c, :]
//
// A pure row copy: ONE WAVE PER OUTPUT ROW, four rows per wave in flight.  The row number is wave-uniform (readfirstlane), so the
// whole decomposition (b, c, n, l), the table reads and the modulus are scalar work done once per row; the lanes only add
// their 16-byte column offset.  Rows are D4 = D / 4 float4 wide; every element offset is 64-bit (a UCF-Crime bank holds more
// than 2^31 floats).  The grid is capped and strides over the rows.
constexpr int SAMPLE_ROWS_PER_WAVE = 4;

__global__ __launch_bounds__(256) void sample_segments_kernel(const f32x4* __restrict__ bank, const int64_t* __restrict__ row_off,
                                                              const int32_t* __restrict__ frames, const int32_t* __restrict__ vid,
                                                              const int32_t* __restrict__ starts, f32x4* __restrict__ out,
                                                              uint32_t rows, uint32_t N, uint32_t L, uint32_t stride,
                                                              uint32_t ncrops, uint32_t D4) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const uint32_t NL = N * L;
  const uint64_t step = (uint64_t)gridDim.x * 4 * SAMPLE_ROWS_PER_WAVE;
  for (uint64_t r0 = (uint64_t)wave * SAMPLE_ROWS_PER_WAVE; r0 < rows; r0 += step) {
    const f32x4* src[SAMPLE_ROWS_PER_WAVE];
#pragma unroll
    for (int j = 0; j < SAMPLE_ROWS_PER_WAVE; ++j) {
      const uint32_t r = (uint32_t)(r0 + j < rows ? r0 + j : rows - 1);     // past the end: re-read the last row, store nothing
      const uint32_t bc = r / NL, nl = r - bc * NL;
      const uint32_t b = bc / ncrops, c = bc - b * ncrops;
      const uint32_t n = nl / L, l = nl - n * L;
      const int32_t v = vid[b];
      const int64_t T = frames[v];
      int64_t t = ((int64_t)starts[(uint64_t)b * N + n] + (int64_t)l * stride) % T;
      if (t < 0) t += T;                                                     // a true modulus, whatever the sign of the start
      src[j] = bank + (row_off[v] + t * ncrops + c) * (int64_t)D4;
    }
    for (uint32_t k = lane; k < D4; k += 64) {
      f32x4 x[SAMPLE_ROWS_PER_WAVE];
#pragma unroll
      for (int j = 0; j < SAMPLE_ROWS_PER_WAVE; ++j) x[j] = src[j][k];
#pragma unroll
      for (int j = 0; j < SAMPLE_ROWS_PER_WAVE; ++j)
        if (r0 + j < rows) out[(r0 + j) * D4 + k] = x[j];
    }
  }
}

extern "C" int acx_sample_segments(acx_ctx* ctx, const float* bank, const int64_t* row_off, const int32_t* frames, const int32_t* vid,
                                   const int32_t* starts, float* out, int32_t B, int32_t N, int32_t L, int32_t stride,
                                   int32_t ncrops, int32_t D, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (B == 0) return ACX_OK;
  if (!bank || !row_off || !frames || !vid || !starts || !out) return acx_fail(ctx, ACX_E_BADARG, "acx_sample_segments: null pointer%s");
  if (B < 0 || N <= 0 || L <= 0 || stride <= 0 || ncrops <= 0 || D <= 0)
    return acx_fail(ctx, ACX_E_BADARG, "acx_sample_segments: B, N, L, stride, ncrops and D must be positive%s");
  if (D % 4 || (((uintptr_t)bank | (uintptr_t)out) & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_sample_segments: D %% 4 == 0 and 16-byte aligned bank / out (the copy moves 16 bytes per lane)%s");
  const int64_t rows = (int64_t)B * ncrops * N * L;
  if ((int64_t)N * L > INT32_MAX || rows > INT32_MAX || (int64_t)L * stride > INT32_MAX)
    return acx_fail(ctx, ACX_E_BADARG, "acx_sample_segments: B * ncrops * N * L and L * stride must stay below 2^31%s");
  const int64_t groups = (rows + 4 * SAMPLE_ROWS_PER_WAVE - 1) / (4 * SAMPLE_ROWS_PER_WAVE);     // one per workgroup of four waves
  const unsigned grid = (unsigned)(groups < 2048 ? groups : 2048);
  hipLaunchKernelGGL(sample_segments_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const f32x4*)bank, row_off, frames, vid,
                     starts, (f32x4*)out, (uint32_t)rows, (uint32_t)N, (uint32_t)L, (uint32_t)stride, (uint32_t)ncrops, (uint32_t)(D / 4));
  ACX_CHECK_LAUNCH(ctx, "acx_sample_segments");
  return ACX_OK;
}

// out[out_off[j] + c * rows[j] + r, :] = bank[row_off[vid[j]] + ((r * stride) mod frames[vid[j]]) * ncrops + c, :]
//
// The test-mode tiles of a group of videos, video after video, each crop-major (what AnomalyCLIP.forward_test_many takes).  The same
// row copy as above: one wave per output row, four rows per wave in flight, all row arithmetic wave-uniform.  Every rows[j] is a
// multiple of NL = N * L, so `blk` (one entry per NL output rows, built on the host) names the video of an output row without a
// search; out_off[j] + c * rows[j] + r IS the output row, so only the source needs the decomposition.  r * stride stays below
// 2^32 (the entry point checks total rows * stride), the modulus is a 32-bit one.
__global__ __launch_bounds__(256) void tile_videos_kernel(const f32x4* __restrict__ bank, const int64_t* __restrict__ row_off,
                                                          const int32_t* __restrict__ frames, const int32_t* __restrict__ vid,
                                                          const int64_t* __restrict__ out_off, const int32_t* __restrict__ vrows,
                                                          const int32_t* __restrict__ blk, f32x4* __restrict__ out, uint32_t rows,
                                                          uint32_t NL, uint32_t stride, uint32_t ncrops, uint32_t D4) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const uint64_t step = (uint64_t)gridDim.x * 4 * SAMPLE_ROWS_PER_WAVE;
  for (uint64_t r0 = (uint64_t)wave * SAMPLE_ROWS_PER_WAVE; r0 < rows; r0 += step) {
    const f32x4* src[SAMPLE_ROWS_PER_WAVE];
#pragma unroll
    for (int i = 0; i < SAMPLE_ROWS_PER_WAVE; ++i) {
      const uint32_t R = (uint32_t)(r0 + i < rows ? r0 + i : rows - 1);     // past the end: re-read the last row, store nothing
      const int32_t j = blk[R / NL];
      const int32_t v = vid[j];
      const uint32_t q = (uint32_t)((int64_t)R - out_off[j]);                // c * rows[j] + r
      const uint32_t vr = (uint32_t)vrows[j];
      const uint32_t c = q / vr, r = q - c * vr;
      const uint32_t t = (r * stride) % (uint32_t)frames[v];
      src[i] = bank + (row_off[v] + (int64_t)t * ncrops + c) * (int64_t)D4;
    }
    for (uint32_t k = lane; k < D4; k += 64) {
      f32x4 x[SAMPLE_ROWS_PER_WAVE];
#pragma unroll
      for (int i = 0; i < SAMPLE_ROWS_PER_WAVE; ++i) x[i] = src[i][k];
#pragma unroll
      for (int i = 0; i < SAMPLE_ROWS_PER_WAVE; ++i)
        if (r0 + i < rows) out[(r0 + i) * D4 + k] = x[i];
    }
  }
}

extern "C" int acx_tile_videos(acx_ctx* ctx, const float* bank, const int64_t* row_off, const int32_t* frames, const int32_t* vid,
                               const int64_t* out_off, const int32_t* rows, const int32_t* blk, float* out, int32_t V,
                               int64_t total_rows, int32_t N, int32_t L, int32_t stride, int32_t ncrops, int32_t D, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (V == 0) return ACX_OK;
  if (!bank || !row_off || !frames || !vid || !out_off || !rows || !blk || !out)
    return acx_fail(ctx, ACX_E_BADARG, "acx_tile_videos: null pointer%s");
  if (V < 0 || total_rows <= 0 || N <= 0 || L <= 0 || stride <= 0 || ncrops <= 0 || D <= 0)
    return acx_fail(ctx, ACX_E_BADARG, "acx_tile_videos: V, total_rows, N, L, stride, ncrops and D must be positive%s");
  if (D % 4 || (((uintptr_t)bank | (uintptr_t)out) & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_tile_videos: D %% 4 == 0 and 16-byte aligned bank / out (the copy moves 16 bytes per lane)%s");
  if (total_rows > INT32_MAX || (int64_t)N * L > INT32_MAX || total_rows * stride > INT32_MAX)
    return acx_fail(ctx, ACX_E_BADARG, "acx_tile_videos: total_rows, N * L and total_rows * stride must stay below 2^31%s");
  if (total_rows % ((int64_t)N * L))
    return acx_fail(ctx, ACX_E_BADARG, "acx_tile_videos: total_rows must be a multiple of N * L (blk has one entry per N * L rows)%s");
  const int64_t groups = (total_rows + 4 * SAMPLE_ROWS_PER_WAVE - 1) / (4 * SAMPLE_ROWS_PER_WAVE);     // one per workgroup of four waves
  const unsigned grid = (unsigned)(groups < 2048 ? groups : 2048);
  hipLaunchKernelGGL(tile_videos_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const f32x4*)bank, row_off, frames, vid, out_off,
                     rows, blk, (f32x4*)out, (uint32_t)total_rows, (uint32_t)(N * L), (uint32_t)stride, (uint32_t)ncrops, (uint32_t)(D / 4));
  ACX_CHECK_LAUNCH(ctx, "acx_tile_videos");
  return ACX_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Half-precision feature files: the same banks and tiles with float16 rows.  The halves are numpy's ('<f2', IEEE binary16); every
// gather widens them on the way out (exact), so what the head sees is float32 as before.

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// float32 bits -> float16 bits, round to nearest even with subnormal halves, in integer arithmetic: numpy's astype(float16) bit for
// bit (npy_floatbits_to_halfbits), NaN payloads included, whatever denormal mode the kernel runs under.
__host__ __device__ static inline uint32_t acx_f32_to_f16_bits(uint32_t x) {
  const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
  if (a >= 0x7f800000u) {                                     // inf, NaN: the payload's top ten bits, never all zero
    if (a == 0x7f800000u) return sign | 0x7c00u;
    const uint32_t h = 0x7c00u | ((a & 0x007fffffu) >> 13);
    return sign | (h == 0x7c00u ? 0x7c01u : h);
  }
  if (a >= 0x38800000u) {                                     // a normal half, or past the largest: the carry of the rounding runs into
    uint32_t h = (a - 0x38000000u) >> 13;                     // the exponent, 0x7c00 (inf) from 65520 on
    const uint32_t rem = a & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) ++h;
    return sign | (h < 0x7c00u ? h : 0x7c00u);
  }
  if (a < 0x33000000u) return sign;                           // below 2^-25: zero (2^-25 itself is a tie, handled below: to even, zero)
  const uint32_t s = 126u - (a >> 23);                        // 14 ... 24: the half's unit is 2^-24
  const uint32_t m = (a & 0x007fffffu) | 0x00800000u;
  uint32_t h = m >> s;
  const uint32_t rem = m & ((1u << s) - 1u), half = 1u << (s - 1);
  if (rem > half || (rem == half && (h & 1))) ++h;            // (a carry out of the subnormals lands on 0x0400 = 2^-14)
  return sign | h;
}

// dst[r, :cols] = half(src[r, :cols]), src rows `ld` floats apart.  One wave per row, four rows per wave in flight: a lane loads 16
// bytes and stores 8.  A finite input whose half is not is counted: per lane, reduced over the wave, one atomic per workgroup.
__global__ __launch_bounds__(256) void cast_rows_f16_kernel(const f32x4* __restrict__ src, u16x4* __restrict__ dst, uint64_t rows,
                                                            uint32_t C4, uint64_t ld4, unsigned long long* __restrict__ overflow) {
  __shared__ uint32_t wave_over[4];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const uint64_t step = (uint64_t)gridDim.x * 4 * SAMPLE_ROWS_PER_WAVE;
  uint32_t over = 0;
  for (uint64_t r0 = (uint64_t)wave * SAMPLE_ROWS_PER_WAVE; r0 < rows; r0 += step) {
    for (uint32_t k = lane; k < C4; k += 64) {
      f32x4 x[SAMPLE_ROWS_PER_WAVE];
#pragma unroll
      for (int j = 0; j < SAMPLE_ROWS_PER_WAVE; ++j) x[j] = src[(r0 + j < rows ? r0 + j : rows - 1) * ld4 + k];     // past the end: the last row again
#pragma unroll
      for (int j = 0; j < SAMPLE_ROWS_PER_WAVE; ++j) {
        if (r0 + j >= rows) continue;
        u16x4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t b = __float_as_uint(x[j][e]);
          const uint32_t q = acx_f32_to_f16_bits(b);
          h[e] = (unsigned short)q;
          over += ((b & 0x7fffffffu) < 0x7f800000u && (q & 0x7fffu) == 0x7c00u) ? 1u : 0u;
        }
        dst[(r0 + j) * C4 + k] = h;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) over += __shfl_xor(over, o);
  if (lane == 0) wave_over[threadIdx.x >> 6] = over;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t n = wave_over[0] + wave_over[1] + wave_over[2] + wave_over[3];
    if (n) atomicAdd(overflow, (unsigned long long)n);
  }
}

extern "C" int acx_cast_rows_f16(acx_ctx* ctx, const float* src, void* dst, int64_t rows, int32_t cols, int64_t ld,
                                 int64_t* overflow_count, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (rows == 0) return ACX_OK;
  if (!src || !dst || !overflow_count) return acx_fail(ctx, ACX_E_BADARG, "acx_cast_rows_f16: null pointer%s");
  if (rows < 0 || cols <= 0 || ld < cols) return acx_fail(ctx, ACX_E_BADARG, "acx_cast_rows_f16: rows >= 0, cols > 0 and ld >= cols%s");
  if (cols % 4 || ld % 4 || ((uintptr_t)src & 15) || (((uintptr_t)dst | (uintptr_t)overflow_count) & 7))
    return acx_fail(ctx, ACX_E_BADARG, "acx_cast_rows_f16: cols %% 4 == 0, ld %% 4 == 0, 16-byte aligned src, 8-byte aligned dst and "
                                       "overflow_count (a lane loads 16 bytes and stores 8)%s");
  const int64_t groups = (rows + 4 * SAMPLE_ROWS_PER_WAVE - 1) / (4 * SAMPLE_ROWS_PER_WAVE);
  const unsigned grid = (unsigned)(groups < 2048 ? groups : 2048);
  hipLaunchKernelGGL(cast_rows_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const f32x4*)src, (u16x4*)dst, (uint64_t)rows,
                     (uint32_t)(cols / 4), (uint64_t)(ld / 4), (unsigned long long*)overflow_count);
  ACX_CHECK_LAUNCH(ctx, "acx_cast_rows_f16");
  return ACX_OK;
}

// The row copy of the two gathers from a float16 bank: a lane loads four halves (8 bytes: a half row of D % 4 == 0 elements is
// 8-byte aligned only) and stores four floats.  (16-byte loads where D % 8 == 0 were measured and did not pay at D = 512: DESIGN.md.)
__device__ __forceinline__ void copy_rows_f16(const f16x4* const (&src)[SAMPLE_ROWS_PER_WAVE], f32x4* __restrict__ out, uint64_t r0,
                                              uint32_t rows, uint32_t D4, uint32_t lane) {
  for (uint32_t k = lane; k < D4; k += 64) {
    f16x4 x[SAMPLE_ROWS_PER_WAVE];
#pragma unroll
    for (int j = 0; j < SAMPLE_ROWS_PER_WAVE; ++j) x[j] = src[j][k];
#pragma unroll
    for (int j = 0; j < SAMPLE_ROWS_PER_WAVE; ++j)
      if (r0 + j < rows) out[(r0 + j) * D4 + k] = __builtin_convertvector(x[j], f32x4);     // exact: every half is a float
  }
}

// acx_sample_segments' kernel on a float16 bank: the same row arithmetic, out stays float32
__global__ __launch_bounds__(256) void sample_segments_f16_kernel(const f16x4* __restrict__ bank, const int64_t* __restrict__ row_off,
                                                                  const int32_t* __restrict__ frames, const int32_t* __restrict__ vid,
                                                                  const int32_t* __restrict__ starts, f32x4* __restrict__ out,
                                                                  uint32_t rows, uint32_t N, uint32_t L, uint32_t stride,
                                                                  uint32_t ncrops, uint32_t D4) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const uint32_t NL = N * L;
  const uint64_t step = (uint64_t)gridDim.x * 4 * SAMPLE_ROWS_PER_WAVE;
  for (uint64_t r0 = (uint64_t)wave * SAMPLE_ROWS_PER_WAVE; r0 < rows; r0 += step) {
    const f16x4* src[SAMPLE_ROWS_PER_WAVE];
#pragma unroll
    for (int j = 0; j < SAMPLE_ROWS_PER_WAVE; ++j) {
      const uint32_t r = (uint32_t)(r0 + j < rows ? r0 + j : rows - 1);     // past the end: re-read the last row, store nothing
      const uint32_t bc = r / NL, nl = r - bc * NL;
      const uint32_t b = bc / ncrops, c = bc - b * ncrops;
      const uint32_t n = nl / L, l = nl - n * L;
      const int32_t v = vid[b];
      const int64_t T = frames[v];
      int64_t t = ((int64_t)starts[(uint64_t)b * N + n] + (int64_t)l * stride) % T;
      if (t < 0) t += T;                                                     // a true modulus, whatever the sign of the start
      src[j] = bank + (row_off[v] + t * ncrops + c) * (int64_t)D4;
    }
    copy_rows_f16(src, out, r0, rows, D4, lane);
  }
}

// acx_tile_videos' kernel on a float16 bank
__global__ __launch_bounds__(256) void tile_videos_f16_kernel(const f16x4* __restrict__ bank, const int64_t* __restrict__ row_off,
                                                              const int32_t* __restrict__ frames, const int32_t* __restrict__ vid,
                                                              const int64_t* __restrict__ out_off, const int32_t* __restrict__ vrows,
                                                              const int32_t* __restrict__ blk, f32x4* __restrict__ out, uint32_t rows,
                                                              uint32_t NL, uint32_t stride, uint32_t ncrops, uint32_t D4) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
  const uint64_t step = (uint64_t)gridDim.x * 4 * SAMPLE_ROWS_PER_WAVE;
  for (uint64_t r0 = (uint64_t)wave * SAMPLE_ROWS_PER_WAVE; r0 < rows; r0 += step) {
    const f16x4* src[SAMPLE_ROWS_PER_WAVE];
#pragma unroll
    for (int i = 0; i < SAMPLE_ROWS_PER_WAVE; ++i) {
      const uint32_t R = (uint32_t)(r0 + i < rows ? r0 + i : rows - 1);     // past the end: re-read the last row, store nothing
      const int32_t j = blk[R / NL];
      const int32_t v = vid[j];
      const uint32_t q = (uint32_t)((int64_t)R - out_off[j]);                // c * rows[j] + r
      const uint32_t vr = (uint32_t)vrows[j];
      const uint32_t c = q / vr, r = q - c * vr;
      const uint32_t t = (r * stride) % (uint32_t)frames[v];
      src[i] = bank + (row_off[v] + (int64_t)t * ncrops + c) * (int64_t)D4;
    }
    copy_rows_f16(src, out, r0, rows, D4, lane);
  }
}

extern "C" int acx_sample_segments_f16(acx_ctx* ctx, const void* bank, const int64_t* row_off, const int32_t* frames, const int32_t* vid,
                                       const int32_t* starts, float* out, int32_t B, int32_t N, int32_t L, int32_t stride,
                                       int32_t ncrops, int32_t D, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (B == 0) return ACX_OK;
  if (!bank || !row_off || !frames || !vid || !starts || !out) return acx_fail(ctx, ACX_E_BADARG, "acx_sample_segments_f16: null pointer%s");
  if (B < 0 || N <= 0 || L <= 0 || stride <= 0 || ncrops <= 0 || D <= 0)
    return acx_fail(ctx, ACX_E_BADARG, "acx_sample_segments_f16: B, N, L, stride, ncrops and D must be positive%s");
  if (D % 4 || ((uintptr_t)bank & 7) || ((uintptr_t)out & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_sample_segments_f16: D %% 4 == 0, 8-byte aligned bank and 16-byte aligned out (the copy loads 8 "
                                       "bytes and stores 16 per lane)%s");
  const int64_t rows = (int64_t)B * ncrops * N * L;
  if ((int64_t)N * L > INT32_MAX || rows > INT32_MAX || (int64_t)L * stride > INT32_MAX)
    return acx_fail(ctx, ACX_E_BADARG, "acx_sample_segments_f16: B * ncrops * N * L and L * stride must stay below 2^31%s");
  const int64_t groups = (rows + 4 * SAMPLE_ROWS_PER_WAVE - 1) / (4 * SAMPLE_ROWS_PER_WAVE);     // one per workgroup of four waves
  const unsigned grid = (unsigned)(groups < 2048 ? groups : 2048);
  hipLaunchKernelGGL(sample_segments_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const f16x4*)bank, row_off, frames, vid, starts, (f32x4*)out,
                     (uint32_t)rows, (uint32_t)N, (uint32_t)L, (uint32_t)stride, (uint32_t)ncrops, (uint32_t)(D / 4));
  ACX_CHECK_LAUNCH(ctx, "acx_sample_segments_f16");
  return ACX_OK;
}

extern "C" int acx_tile_videos_f16(acx_ctx* ctx, const void* bank, const int64_t* row_off, const int32_t* frames, const int32_t* vid,
                                   const int64_t* out_off, const int32_t* rows, const int32_t* blk, float* out, int32_t V,
                                   int64_t total_rows, int32_t N, int32_t L, int32_t stride, int32_t ncrops, int32_t D, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (V == 0) return ACX_OK;
  if (!bank || !row_off || !frames || !vid || !out_off || !rows || !blk || !out)
    return acx_fail(ctx, ACX_E_BADARG, "acx_tile_videos_f16: null pointer%s");
  if (V < 0 || total_rows <= 0 || N <= 0 || L <= 0 || stride <= 0 || ncrops <= 0 || D <= 0)
    return acx_fail(ctx, ACX_E_BADARG, "acx_tile_videos_f16: V, total_rows, N, L, stride, ncrops and D must be positive%s");
  if (D % 4 || ((uintptr_t)bank & 7) || ((uintptr_t)out & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_tile_videos_f16: D %% 4 == 0, 8-byte aligned bank and 16-byte aligned out (the copy loads 8 bytes "
                                       "and stores 16 per lane)%s");
  if (total_rows > INT32_MAX || (int64_t)N * L > INT32_MAX || total_rows * stride > INT32_MAX)
    return acx_fail(ctx, ACX_E_BADARG, "acx_tile_videos_f16: total_rows, N * L and total_rows * stride must stay below 2^31%s");
  if (total_rows % ((int64_t)N * L))
    return acx_fail(ctx, ACX_E_BADARG, "acx_tile_videos_f16: total_rows must be a multiple of N * L (blk has one entry per N * L rows)%s");
  const int64_t groups = (total_rows + 4 * SAMPLE_ROWS_PER_WAVE - 1) / (4 * SAMPLE_ROWS_PER_WAVE);     // one per workgroup of four waves
  const unsigned grid = (unsigned)(groups < 2048 ? groups : 2048);
  hipLaunchKernelGGL(tile_videos_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const f16x4*)bank, row_off, frames, vid, out_off, rows, blk,
                     (f32x4*)out, (uint32_t)total_rows, (uint32_t)(N * L), (uint32_t)stride, (uint32_t)ncrops, (uint32_t)(D / 4));
  ACX_CHECK_LAUNCH(ctx, "acx_tile_videos_f16");
  return ACX_OK;
}

// dst[i] = float(src[i]) over rows * D contiguous elements (the streamed test path uploads halves and widens them here): nothing to
// look up, so the rows are one flat run of 8-byte pieces; 64-bit offsets, a capped grid that strides.
__global__ __launch_bounds__(256) void expand_rows_f16_kernel(const f16x4* __restrict__ src, f32x4* __restrict__ dst, uint64_t n4) {
  const uint64_t step = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += step) dst[i] = __builtin_convertvector(src[i], f32x4);
}

extern "C" int acx_expand_rows_f16(acx_ctx* ctx, const void* src, float* dst, int64_t rows, int32_t D, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (rows == 0) return ACX_OK;
  if (!src || !dst) return acx_fail(ctx, ACX_E_BADARG, "acx_expand_rows_f16: null pointer%s");
  if (rows < 0 || D <= 0) return acx_fail(ctx, ACX_E_BADARG, "acx_expand_rows_f16: rows >= 0 and D > 0%s");
  if (D % 4 || ((uintptr_t)src & 7) || ((uintptr_t)dst & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_expand_rows_f16: D %% 4 == 0, 8-byte aligned src and 16-byte aligned dst (a lane loads 8 bytes "
                                       "and stores 16)%s");
  const uint64_t n4 = (uint64_t)rows * (uint64_t)(D / 4);
  const uint64_t groups = (n4 + 1023) / 1024;                              // four pieces per lane before the grid strides
  const unsigned grid = (unsigned)(groups < 4096 ? groups : 4096);
  hipLaunchKernelGGL(expand_rows_f16_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const f16x4*)src, (f32x4*)dst, n4);
  ACX_CHECK_LAUNCH(ctx, "acx_expand_rows_f16");
  return ACX_OK;
}
