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
