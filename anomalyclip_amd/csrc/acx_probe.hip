// Measured denominators for the roofline report ("the builder must measure a GEMM peak and a
// stream-copy peak on the box and report both nominal and measured denominators").  Two micro-kernels, no product path
// uses them:
//   acx_probe_mfma  -- register-only MFMA loop (v_mfma_f32_32x32x2_f32 or v_mfma_f32_32x32x16_bf16), four independent
//                      accumulator chains per wave, `waves_per_simd` waves on every SIMD of the chip: the issue-rate
//                      ceiling of the matrix pipe at the clock the chip sustains under that load (bf16 = 1: constant operands;
//                      bf16 = 2: random operands -- the rate the power limit leaves with operands that toggle like data;
//                      bf16 = 3: mode 2 on v_mfma_f32_16x16x32_bf16 (sixteen 16 x 16 accumulators: the same 64 registers);
//                      bf16 = 4 / 5: the plane-reuse kernel's X half-step without its DMA and barriers on 32x32x16 / 16x16x32 --
//                      128 x 128 outputs per wave, every operand fragment re-read from LDS by ds_read_b128 in each 32-wide K-step);
//   acx_probe_copy  -- 16-byte-per-lane grid-stride copy (global_load_dwordx4 / global_store_dwordx4): the HBM stream
//                      ceiling (read + write) the row kernels are measured against.
#include "acx_internal.h"
#include <algorithm>

namespace {

template <int BF16>
__global__ __launch_bounds__(256) void probe_mfma_kernel(int iters, float* __restrict__ sink) {
  f32x16 a0, a1, a2, a3;
#pragma unroll
  for (int e = 0; e < 16; ++e) { a0[e] = 0.f; a1[e] = 0.f; a2[e] = 0.f; a3[e] = 0.f; }
  const float x = 1.0f + (float)(threadIdx.x & 7) * 0.125f, y = 0.5f;
  if constexpr (BF16 == 2) {
    // RANDOM operands: four different (A, B) fragment pairs per lane, bf16 values with random sign / mantissa and exponents in
    // [2^-3, 2^1) -- the matrix pipe's sustained rate at the chip's power limit with operands that toggle like real data (the
    // constant-operand loop above measures the issue rate at a clock real operands do not sustain)
    bf16x8 ra[4], rb[4];
    unsigned st = (unsigned)(blockIdx.x * 256 + threadIdx.x) * 2654435761u + 12345u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      typedef unsigned short u16x8_ __attribute__((ext_vector_type(8)));
      u16x8_ va, vb;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        st = st * 1664525u + 1013904223u;
        va[e] = (unsigned short)(((st >> 16) & 0x807fu) | ((124u + ((st >> 9) & 3u)) << 7));
        st = st * 1664525u + 1013904223u;
        vb[e] = (unsigned short)(((st >> 16) & 0x807fu) | ((124u + ((st >> 9) & 3u)) << 7));
      }
      ra[q] = __builtin_bit_cast(bf16x8, va); rb[q] = __builtin_bit_cast(bf16x8, vb);
    }
    for (int i = 0; i < iters; ++i) {
      a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[0], rb[0], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[1], rb[1], a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[2], rb[2], a2, 0, 0, 0);
      a3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ra[3], rb[3], a3, 0, 0, 0);
    }
  } else if constexpr (BF16 == 3) {
    // mode 2 on the 16 x 16 x 32 shape: a 64 x 64 output block per wave as sixteen 16 x 16 accumulators (the same 64 registers),
    // four random A and four random B fragments per lane; an iteration is 16 MFMAs (the FLOPs and MFMA cycles of TWO mode 2 iterations)
    bf16x8 ra[4], rb[4];
    unsigned st = (unsigned)(blockIdx.x * 256 + threadIdx.x) * 2654435761u + 12345u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      typedef unsigned short u16x8_ __attribute__((ext_vector_type(8)));
      u16x8_ va, vb;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        st = st * 1664525u + 1013904223u;
        va[e] = (unsigned short)(((st >> 16) & 0x807fu) | ((124u + ((st >> 9) & 3u)) << 7));
        st = st * 1664525u + 1013904223u;
        vb[e] = (unsigned short)(((st >> 16) & 0x807fu) | ((124u + ((st >> 9) & 3u)) << 7));
      }
      ra[q] = __builtin_bit_cast(bf16x8, va); rb[q] = __builtin_bit_cast(bf16x8, vb);
    }
    f32x4 c[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) c[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < iters; ++i) {
#pragma unroll
      for (int qa = 0; qa < 4; ++qa)
#pragma unroll
        for (int qb = 0; qb < 4; ++qb)   // (in-out AGPR accumulator: see PB_MM below)
          asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c[qa][qb]) : "v"(ra[qa]), "v"(rb[qb]));
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) { a0[0] += c[i][j][0]; a1[0] += c[i][j][1]; a2[0] += c[i][j][2]; a3[0] += c[i][j][3]; }
  } else if constexpr (BF16 == 1) {
    bf16x8 xa, xb;
#pragma unroll
    for (int e = 0; e < 8; ++e) { xa[e] = (__bf16)x; xb[e] = (__bf16)y; }
    for (int i = 0; i < iters; ++i) {
      a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa, xb, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa, xb, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa, xb, a2, 0, 0, 0);
      a3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa, xb, a3, 0, 0, 0);
    }
  } else {
    for (int i = 0; i < iters; ++i) {
      a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, a2, 0, 0, 0);
      a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, a3, 0, 0, 0);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) s += a0[e] + a1[e] + a2[e] + a3[e];
  if (s == 12345.678f) sink[0] = s;              // keeps the chains alive; never true
}

// LDS-fed loop (modes 4, 5): one wave per SIMD, 2 x 2 waves, 128 x 128 outputs per wave (256 accumulator registers), four 16 KB
// units of random bf16 (256 rows x 64 B: "A" and three "W" planes).  An iteration is one 32-wide K-step of three products that
// share the A fragments: 32 ds_read_b128 per wave (8 + 24 fragments of 16 rows x 32 k, or two substeps of 4 + 12 fragments of
// 32 rows x 16 k) feeding 192 MFMAs of 16x16x32 or 96 of 32x32x16 -- the same LDS bytes, the same 3,072 MFMA cycles.  Addresses
// are conflict-free by the bank model: 32-row fragments at chunk ^ ((row >> 2) & 3) (the product kernel's swizzle), 16-row
// fragments at chunk ^ ((row >> 1) & 3).  The fragment base passes through an empty asm in every iteration: the reads stay in
// the loop.  (`iters` is rounded up to an even number.)
template <int S16>
__global__ __launch_bounds__(256, 1) void probe_mfma_lds_kernel(int iters, float* __restrict__ sink) {
  extern __shared__ __attribute__((aligned(1024))) char psm[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  {
    unsigned st = (unsigned)(blockIdx.x * 256 + t) * 2654435761u + 777u;
    unsigned* w32 = reinterpret_cast<unsigned*>(psm);
    for (int i = t; i < 4 * 16384 / 4; i += 256) {
      st = st * 1664525u + 1013904223u;
      const unsigned lo = ((st >> 16) & 0x807fu) | ((124u + ((st >> 9) & 3u)) << 7);
      st = st * 1664525u + 1013904223u;
      const unsigned hi = ((st >> 16) & 0x807fu) | ((124u + ((st >> 9) & 3u)) << 7);
      w32[i] = lo | (hi << 16);
    }
  }
  __syncthreads();
  float s = 0.f;
  if constexpr (S16 != 0) {
    f32x4 acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int r = lane & 15, c = (lane >> 4) ^ ((r >> 1) & 3);
    int fa = (wm * 128 + r) * 64 + c * 16, fw = 16384 + (wn * 128 + r) * 64 + c * 16;
    // hand-placed like the product kernel (hipcc's own schedule of this loop shuffles the accumulators between register files):
    // the A fragments of a K-step stay resident, the W fragments come in four groups of two column blocks x three planes,
    // double-buffered; a block is the 48 MFMAs of one group with the next group's reads one per MFMA gap, the K-step's last group
    // runs beside the next K-step's first reads.  Two K-steps per loop trip (the A sets alternate).
    bf16x8 A0[8], A1[8], WA[6], WB[6];
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) A1[q][e] = (__bf16)0.f;
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) WB[q][e] = (__bf16)0.f;
#define PB_FR(off) (*reinterpret_cast<const bf16x8*>(psm + (off)))
#define PB_RDW(WX, g, f) WX[f] = PB_FR(fw + ((f) >> 1) * 16384 + (2 * (g) + ((f) & 1)) * 1024)
// (inline asm with the accumulator as an in-out AGPR operand: hipcc does not tie the destination of this 4-register MFMA to
// its SrcC, and resolves the difference with hundreds of v_accvgpr moves per trip; an accumulator is touched once per 16 MFMAs)
#define PB_MM(WX, AS, g, q)                                                                                       \
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[((q) % 16) / 2][2 * (g) + (q) % 2])          \
               : "v"(WX[2 * ((q) / 16) + (q) % 2]), "v"(AS[((q) % 16) / 2]))
#define PB_REP48(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15) M(16) M(17) M(18) M(19) M(20) M(21) M(22) M(23) M(24) M(25) M(26) M(27) M(28) M(29) M(30) M(31) M(32) M(33) M(34) M(35) M(36) M(37) M(38) M(39) M(40) M(41) M(42) M(43) M(44) M(45) M(46) M(47)
#define PB_B0(q) { if constexpr ((q) < 8) PB_AC[(q) & 7] = PB_FR(fa + ((q) & 7) * 1024); else if constexpr ((q) < 14) PB_RDW(WA, 0, ((q) - 8) % 6); \
                   PB_MM(WB, PB_AP, 3, q); __builtin_amdgcn_sched_barrier(0); }
#define PB_B1(q) { if constexpr ((q) < 6) PB_RDW(WB, 1, (q) % 6); PB_MM(WA, PB_AC, 0, q); __builtin_amdgcn_sched_barrier(0); }
#define PB_B2(q) { if constexpr ((q) < 6) PB_RDW(WA, 2, (q) % 6); PB_MM(WB, PB_AC, 1, q); __builtin_amdgcn_sched_barrier(0); }
#define PB_B3(q) { if constexpr ((q) < 6) PB_RDW(WB, 3, (q) % 6); PB_MM(WA, PB_AC, 2, q); __builtin_amdgcn_sched_barrier(0); }
    for (int it = 0; it < iters; it += 2) {
      asm volatile("" : "+v"(fa), "+v"(fw));
#define PB_AC A0
#define PB_AP A1
      PB_REP48(PB_B0) PB_REP48(PB_B1) PB_REP48(PB_B2) PB_REP48(PB_B3)
#undef PB_AC
#undef PB_AP
      asm volatile("" : "+v"(fa), "+v"(fw));
#define PB_AC A1
#define PB_AP A0
      PB_REP48(PB_B0) PB_REP48(PB_B1) PB_REP48(PB_B2) PB_REP48(PB_B3)
#undef PB_AC
#undef PB_AP
    }
#undef PB_B3
#undef PB_B2
#undef PB_B1
#undef PB_B0
#undef PB_REP48
#undef PB_MM
#undef PB_RDW
#undef PB_FR
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");       // the last MFMAs' results, before the sum below reads them
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) s += acc[i][j][0] + acc[i][j][1] + acc[i][j][2] + acc[i][j][3];
  } else {
    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int r = lane & 31, hh = lane >> 5, sw = (r >> 2) & 3;
    int fa = (wm * 128 + r) * 64, fw = 16384 + (wn * 128 + r) * 64;
    // the product kernel's schedule: two sets of 16 fragments (4 A row blocks + 3 x 4 W column blocks of one 16-wide substep), a
    // block is the 48 MFMAs of one set with the other set's 16 reads in its first 16 gaps
    bf16x8 F0[16], F1[16];
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) F1[q][e] = (__bf16)0.f;
    const int c0 = ((0 + hh) ^ sw) * 16, c1 = ((2 + hh) ^ sw) * 16;
#define PB_FR(off) (*reinterpret_cast<const bf16x8*>(psm + (off)))
#define PB_RD(F, cc, q) F[q] = (q) < 4 ? PB_FR(fa + cc + (q) * 2048) : PB_FR(fw + cc + (((q) - 4) >> 2) * 16384 + ((q) & 3) * 2048)
#define PB_MM(F, q) acc[((q) % 16) / 4][(q) % 4] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F[4 + 4 * ((q) / 16) + (q) % 4], F[((q) % 16) / 4], acc[((q) % 16) / 4][(q) % 4], 0, 0, 0)
#define PB_REP48(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15) M(16) M(17) M(18) M(19) M(20) M(21) M(22) M(23) M(24) M(25) M(26) M(27) M(28) M(29) M(30) M(31) M(32) M(33) M(34) M(35) M(36) M(37) M(38) M(39) M(40) M(41) M(42) M(43) M(44) M(45) M(46) M(47)
#define PB_B0(q) { if constexpr ((q) < 16) PB_RD(F0, c0, (q) & 15); PB_MM(F1, q); __builtin_amdgcn_sched_barrier(0); }
#define PB_B1(q) { if constexpr ((q) < 16) PB_RD(F1, c1, (q) & 15); PB_MM(F0, q); __builtin_amdgcn_sched_barrier(0); }
    for (int it = 0; it < iters; ++it) {
      asm volatile("" : "+v"(fa), "+v"(fw));
      PB_REP48(PB_B0) PB_REP48(PB_B1)
    }
#undef PB_B1
#undef PB_B0
#undef PB_REP48
#undef PB_MM
#undef PB_RD
#undef PB_FR
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) s += acc[i][j][e];
  }
  if (s == 12345.678f) sink[0] = s;              // keeps the chains alive; never true
}

__global__ __launch_bounds__(256) void probe_copy_kernel(const f32x4* __restrict__ src, f32x4* __restrict__ dst, int64_t n16) {
  const int64_t stride = (int64_t)gridDim.x * 256 * 8;
  for (int64_t i = (int64_t)blockIdx.x * 2048 + threadIdx.x; i < n16; i += stride) {
    f32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (i + 256 * k < n16) v[k] = __builtin_nontemporal_load(src + i + 256 * k);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (i + 256 * k < n16) __builtin_nontemporal_store(v[k], dst + i + 256 * k);
  }
}

// read-only stream: every lane folds its 16-byte pieces into one value, nothing is written (the sink store never happens) --
// the floor of a ONE-SHOT launch that reads `bytes` once (ramp-up and tail included): what the skinny reductions of the head
// (selector projection, column sums: 67 MB in, a few KB out) are measured against
__global__ __launch_bounds__(256) void probe_read_kernel(const f32x4* __restrict__ src, int64_t n16, float* __restrict__ sink) {
  const int64_t stride = (int64_t)gridDim.x * 256 * 8;
  f32x4 a = {0.f, 0.f, 0.f, 0.f};
  for (int64_t i = (int64_t)blockIdx.x * 2048 + threadIdx.x; i < n16; i += stride) {
    f32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = i + 256 * k < n16 ? src[i + 256 * k] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 8; ++k) a += v[k];
  }
  if (a[0] + a[1] + a[2] + a[3] == 12345.678f) sink[0] = a[0];   // never true for the probe's inputs
}

}  // namespace

extern "C" int acx_probe_read(acx_ctx* ctx, const void* src, int64_t bytes, float* sink, void* stream) {
  if (!src || !sink || bytes <= 0 || (bytes & 15) || ((uintptr_t)src & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_probe_read: need a 16-byte aligned buffer and size%s");
  const int ncu = ctx && ctx->multiprocessors > 0 ? ctx->multiprocessors : 256;
  const int64_t n16 = bytes / 16;
  const int64_t want = (n16 + 2047) / 2048;
  hipLaunchKernelGGL(probe_read_kernel, dim3((unsigned)std::min<int64_t>(want, (int64_t)ncu * 16)), dim3(256), 0, (hipStream_t)stream,
                     (const f32x4*)src, n16, sink);
  ACX_CHECK_LAUNCH(ctx, "acx_probe_read");
  return ACX_OK;
}

extern "C" int acx_probe_mfma(acx_ctx* ctx, int32_t bf16, int32_t iters, int32_t waves_per_simd, float* sink, double* flops_out,
                              void* stream) {
  if (!sink || iters <= 0 || waves_per_simd <= 0 || waves_per_simd > 8 || bf16 < 0 || bf16 > 5 || (bf16 >= 4 && waves_per_simd != 1))
    return acx_fail(ctx, ACX_E_BADARG, "acx_probe_mfma: bad argument%s");
  const int ncu = ctx && ctx->multiprocessors > 0 ? ctx->multiprocessors : 256;
  const dim3 grid((unsigned)(ncu * waves_per_simd)), block(256);           // 4 waves per block = one per SIMD
  hipStream_t s = (hipStream_t)stream;
  if (bf16 >= 4) {                                                          // LDS-fed K-steps: 3 x 128 x 128 x 32 MACs per wave and iteration
    if (bf16 == 5) hipLaunchKernelGGL((probe_mfma_lds_kernel<1>), grid, block, 4 * 16384, s, iters, sink);
    else hipLaunchKernelGGL((probe_mfma_lds_kernel<0>), grid, block, 4 * 16384, s, iters, sink);
    if (flops_out) *flops_out = (double)grid.x * 4.0 * (double)(bf16 == 5 ? (iters + 1) & ~1 : iters) * 3.0 * 2.0 * 128.0 * 128.0 * 32.0;
    ACX_CHECK_LAUNCH(ctx, "acx_probe_mfma");
    return ACX_OK;
  }
  if (bf16 == 3) hipLaunchKernelGGL((probe_mfma_kernel<3>), grid, block, 0, s, iters, sink);
  else if (bf16 == 2) hipLaunchKernelGGL((probe_mfma_kernel<2>), grid, block, 0, s, iters, sink);
  else if (bf16) hipLaunchKernelGGL((probe_mfma_kernel<1>), grid, block, 0, s, iters, sink);
  else hipLaunchKernelGGL((probe_mfma_kernel<0>), grid, block, 0, s, iters, sink);
  if (flops_out) *flops_out = (double)grid.x * 4.0 * (double)iters * (bf16 == 3 ? 16.0 * 16384.0 : 4.0 * (bf16 ? 32768.0 : 4096.0));
  ACX_CHECK_LAUNCH(ctx, "acx_probe_mfma");
  return ACX_OK;
}

extern "C" int acx_probe_copy(acx_ctx* ctx, const void* src, void* dst, int64_t bytes, void* stream) {
  if (!src || !dst || bytes <= 0 || (bytes & 15) || (((uintptr_t)src | (uintptr_t)dst) & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_probe_copy: need 16-byte aligned buffers and size%s");
  const int ncu = ctx && ctx->multiprocessors > 0 ? ctx->multiprocessors : 256;
  hipLaunchKernelGGL(probe_copy_kernel, dim3((unsigned)(ncu * 16)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)src,
                     (f32x4*)dst, bytes / 16);
  ACX_CHECK_LAUNCH(ctx, "acx_probe_copy");
  return ACX_OK;
}
