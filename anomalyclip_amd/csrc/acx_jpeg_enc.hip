// Huffman coding of the qualitative videos' frames on the device (Visualizer(entropy="gpu")): the phases of acx_jpeg_enc_dev.h as
// launches on the caller's stream -- count, scan, zero, write, FF count, FF scan, emit.  What one workgroup needs from another it
// gets at a launch boundary: no workgroup waits on another, no counter, no spin.  The two scans run as ONE workgroup per frame (a
// frame of 1200 x 800 has 22,500 blocks and, coded, a few hundred chunks: some tens of tiles of 1,024).
#include "acx_internal.h"
#include "acx_jpeg_enc_dev.h"

extern "C" int64_t acx_jpeg_encode_header(const uint16_t* qtabs, int32_t H, int32_t W, uint8_t* dst, size_t cap) {
  return acx_jpeg::encode_header(qtabs, H, W, dst, cap);
}

static_assert(acx_jpeg::kHeaderBytes == 623, "APP0, two DQT, SOF0, four DHT, SOS");

namespace {

using acx_jenc::Geo;
using acx_jenc::Tabs;

typedef unsigned int jenc_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMeta = acx_jenc::kMetaWords;              // per frame: bits, U, refused, FF bytes

// the frame's string in memory: words past the frame's part of the workspace are dropped (none is: a block never passes
// kMaxBlockBits, which the part is sized for)
struct DevMem {
  uint32_t* words;
  uint32_t nwords;
  __device__ __forceinline__ void store(uint32_t w, uint32_t v) const {
    if (w < nwords) words[w] = __builtin_bswap32(v);
  }
  __device__ __forceinline__ void merge(uint32_t w, uint32_t v) const {
    if (w < nwords) atomicOr(&words[w], __builtin_bswap32(v));
  }
};

// a lane's block in 32 registers: the 128 bytes as eight 16-byte loads; every index the unrolled coder asks for is a constant
struct RegBlock {
  uint32_t w[32];
  __device__ __forceinline__ void load(const int16_t* p) {
    const jenc_u32x4* q = (const jenc_u32x4*)p;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const jenc_u32x4 v = q[k];
      w[4 * k] = v.x;
      w[4 * k + 1] = v.y;
      w[4 * k + 2] = v.z;
      w[4 * k + 3] = v.w;
    }
  }
  __device__ __forceinline__ int operator()(int i) const { return (int)(int16_t)(w[i >> 1] >> ((i & 1) * 16)); }
};

__device__ __forceinline__ void load_tabs(Tabs* t) {
  uint32_t* dst = (uint32_t*)t;
  const uint32_t* src = (const uint32_t*)&acx_jenc::kTabs;
  for (uint32_t i = threadIdx.x; i < sizeof(Tabs) / 4; i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- count
// one lane per block of the scan, frame blockIdx.y
__global__ __launch_bounds__(256) void jenc_count_kernel(const int16_t* __restrict__ coef, Geo g, uint32_t* __restrict__ lens,
                                                         uint32_t lens_stride) {
  __shared__ Tabs tabs;
  load_tabs(&tabs);
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= g.nb) return;
  const int16_t* frame = coef + (size_t)blockIdx.y * acx_jenc::coef_elems(g);
  uint32_t comp;
  RegBlock blk;
  blk.load(frame + acx_jenc::block_offset(g, s, &comp));
  lens[(size_t)blockIdx.y * lens_stride + s] = acx_jenc::count_block(blk, acx_jenc::pred_dc(g, frame, s), comp, &tabs);
}

// ---------------------------------------------------------------------------------------------------------------- scan
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// p[0 .. n) -> its exclusive prefix sums, in place, by the 1,024 threads of a workgroup in tiles; -> the sum.  The top bit of an
// entry is a flag, not part of the value: *flags ORs them (per thread).  n is the same in every thread.
__device__ __forceinline__ uint32_t scan_in_place(uint32_t* __restrict__ p, uint32_t n, uint32_t* wsum, uint32_t* flags) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < n; base += 1024u) {
    const uint32_t i = base + tid;
    uint32_t v = i < n ? p[i] : 0u;
    *flags |= v & acx_jenc::kErrBit;
    v &= ~acx_jenc::kErrBit;
    const uint32_t incl = wave_inclusive(v, lane);
    if (lane == 63u) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) {
      const uint32_t x = wsum[k];
      before += k < wave ? x : 0u;
      total += x;
    }
    if (i < n) p[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
  return carry;
}

// one workgroup per frame: the blocks' bit counts -> their bit offsets; meta: the frame's bits, its bytes, whether it is refused
__global__ __launch_bounds__(1024) void jenc_scan_kernel(uint32_t* __restrict__ lens, uint32_t lens_stride, uint32_t nb,
                                                         uint32_t* __restrict__ meta) {
  __shared__ uint32_t wsum[16];
  uint32_t flags = 0;
  const uint32_t bits = scan_in_place(lens + (size_t)blockIdx.x * lens_stride, nb, wsum, &flags);
  const int refused = __syncthreads_or(flags != 0u);
  if (threadIdx.x == 0) {
    uint32_t* m = meta + (size_t)blockIdx.x * kMeta;
    m[0] = bits;
    m[1] = acx_jenc::scan_bytes(bits);
    m[2] = refused ? 1u : 0u;
    m[3] = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- zero
// the words the write pass ORs into: the frame's U bytes rounded up to 16 (its part of the workspace has 16 bytes to spare)
__global__ __launch_bounds__(256) void jenc_zero_kernel(uint8_t* __restrict__ bits, uint64_t bits_stride, const uint32_t* __restrict__ meta) {
  const uint32_t n16 = (meta[(size_t)blockIdx.y * kMeta + 1] + 15u) >> 4;
  jenc_u32x4* p = (jenc_u32x4*)(bits + (size_t)blockIdx.y * bits_stride);
  const uint32_t most = (uint32_t)(bits_stride >> 4);
  const jenc_u32x4 z = {0u, 0u, 0u, 0u};
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n16 && i < most; i += gridDim.x * 256u) p[i] = z;
}

// ---------------------------------------------------------------------------------------------------------------- write
__global__ __launch_bounds__(256) void jenc_write_kernel(const int16_t* __restrict__ coef, Geo g, const uint32_t* __restrict__ offs,
                                                         uint32_t lens_stride, uint8_t* __restrict__ bits, uint64_t bits_stride) {
  __shared__ Tabs tabs;
  load_tabs(&tabs);
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= g.nb) return;
  const int16_t* frame = coef + (size_t)blockIdx.y * acx_jenc::coef_elems(g);
  const DevMem mem = {(uint32_t*)(bits + (size_t)blockIdx.y * bits_stride), (uint32_t)(bits_stride >> 2)};
  uint32_t comp;
  RegBlock blk;
  blk.load(frame + acx_jenc::block_offset(g, s, &comp));
  acx_jenc::write_block(blk, acx_jenc::pred_dc(g, frame, s), comp, s == g.nb - 1u, offs[(size_t)blockIdx.y * lens_stride + s], &tabs, mem);
}

// ---------------------------------------------------------------------------------------------------------------- stuff
// a wave per chunk of 256 bytes, a lane per word; the workgroups of a frame share its chunks out
__global__ __launch_bounds__(256) void jenc_ff_count_kernel(const uint8_t* __restrict__ bits, uint64_t bits_stride,
                                                            const uint32_t* __restrict__ meta, uint32_t* __restrict__ cnt,
                                                            uint32_t cnt_stride) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t U = meta[(size_t)blockIdx.y * kMeta + 1], nch = min(acx_jenc::chunks_of(U), cnt_stride);
  const uint32_t* words = (const uint32_t*)(bits + (size_t)blockIdx.y * bits_stride);
  for (uint32_t c = blockIdx.x * 4u + wave; c < nch; c += gridDim.x * 4u) {
    const uint32_t byte0 = c * acx_jenc::kChunkBytes + lane * 4u;
    const uint32_t w = byte0 < U ? words[byte0 >> 2] : 0u;
    const uint32_t incl = wave_inclusive(acx_jenc::ff_count(w, byte0, U), lane);
    if (lane == 63u) cnt[(size_t)blockIdx.y * cnt_stride + c] = incl;
  }
}

// one workgroup per frame: the chunks' FF counts -> the FF bytes before each chunk; the frame's size and status
__global__ __launch_bounds__(1024) void jenc_ff_scan_kernel(uint32_t* __restrict__ cnt, uint32_t cnt_stride, uint32_t* __restrict__ meta,
                                                            int32_t header_bytes, int64_t cap, int32_t* __restrict__ nbytes,
                                                            int32_t* __restrict__ status) {
  __shared__ uint32_t wsum[16];
  uint32_t* m = meta + (size_t)blockIdx.x * kMeta;
  const uint32_t U = m[1], refused = m[2];
  uint32_t flags = 0;
  const uint32_t ff = scan_in_place(cnt + (size_t)blockIdx.x * cnt_stride, min(acx_jenc::chunks_of(U), cnt_stride), wsum, &flags);
  if (threadIdx.x == 0) {
    const int64_t need = acx_jenc::file_bytes(header_bytes, U, ff);
    m[3] = ff;
    nbytes[blockIdx.x] = refused ? 0 : (int32_t)need;
    status[blockIdx.x] = refused ? ACX_E_BADARG : (need > cap ? ACX_E_WORKSPACE : ACX_OK);
  }
}

// header | stuffed scan | FF D9 into the frame's slot, nothing at or past its `cap`; a refused frame's slot is left alone
__global__ __launch_bounds__(256) void jenc_emit_kernel(const uint8_t* __restrict__ bits, uint64_t bits_stride,
                                                        const uint32_t* __restrict__ meta, const uint32_t* __restrict__ cnt,
                                                        uint32_t cnt_stride, const uint8_t* __restrict__ header, int32_t header_bytes,
                                                        uint8_t* __restrict__ files, int64_t cap) {
  const uint32_t* m = meta + (size_t)blockIdx.y * kMeta;
  if (m[2]) return;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t U = m[1], ff = m[3], nch = min(acx_jenc::chunks_of(U), cnt_stride);
  uint8_t* dst = files + (int64_t)blockIdx.y * cap;
  if (blockIdx.x == 0) {
    for (int64_t i = threadIdx.x; i < header_bytes && i < cap; i += 256) dst[i] = header[i];
    if (threadIdx.x < 2u) {
      const int64_t at = (int64_t)header_bytes + U + ff + threadIdx.x;
      if (at < cap) dst[at] = threadIdx.x ? 0xD9 : 0xFF;
    }
  }
  const uint32_t* words = (const uint32_t*)(bits + (size_t)blockIdx.y * bits_stride);
  for (uint32_t c = blockIdx.x * 4u + wave; c < nch; c += gridDim.x * 4u) {
    const uint32_t byte0 = c * acx_jenc::kChunkBytes + lane * 4u;
    const uint32_t w = byte0 < U ? words[byte0 >> 2] : 0u;
    const uint32_t n = acx_jenc::ff_count(w, byte0, U);
    const uint32_t before = cnt[(size_t)blockIdx.y * cnt_stride + c] + wave_inclusive(n, lane) - n;
    acx_jenc::emit_word(w, byte0, U, (int64_t)header_bytes + byte0 + before, dst, cap);
  }
}

}  // namespace

extern "C" size_t acx_jpeg_entropy_encode_dev_workspace_bytes(int32_t H, int32_t W, int32_t B) {
  Geo g;
  if (B < 1 || B > 65535 || !acx_jenc::make_geo(H, W, &g)) return 0;
  acx_jenc::Plan p;
  acx_jenc::make_plan(g, (uint64_t)B, &p);
  return (size_t)p.bytes;
}

extern "C" int acx_jpeg_entropy_encode_dev(acx_ctx* ctx, const int16_t* coef, const uint8_t* header, int32_t header_bytes, int32_t H,
                                           int32_t W, int32_t B, uint8_t* files, int64_t cap, int32_t* nbytes, int32_t* status,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  AcxProfScope prof__(ctx, ACX_K_OTHER, (hipStream_t)stream);
  if (!coef || !header || !files || !nbytes || !status || !workspace)
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_encode_dev: null pointer%s");
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 65535 || W > 65535)
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_encode_dev: 1 <= B, H, W <= 65535%s");
  if (header_bytes < 1 || header_bytes > 65535 || cap < 0)
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_encode_dev: 1 <= header_bytes <= 65535 and cap >= 0%s");
  Geo g;
  if (!acx_jenc::make_geo(H, W, &g))
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_encode_dev: blocks x 1658 bits must stay below 2^31 (bit offsets are 32-bit)%s");
  if (((uintptr_t)coef & 15) || ((uintptr_t)nbytes & 3) || ((uintptr_t)status & 3) || ((uintptr_t)workspace & 15))
    return acx_fail(ctx, ACX_E_BADARG, "acx_jpeg_entropy_encode_dev: coef and workspace 16-byte aligned, nbytes and status to their element%s");
  acx_jenc::Plan p;
  acx_jenc::make_plan(g, (uint64_t)B, &p);
  if ((uint64_t)workspace_bytes < p.bytes)
    return acx_fail(ctx, ACX_E_WORKSPACE, "acx_jpeg_entropy_encode_dev: %sworkspace of %ld bytes, needs %ld", "", (long)workspace_bytes,
                    (long)p.bytes);
  hipStream_t s = (hipStream_t)stream;
  uint8_t* ws = (uint8_t*)workspace;
  uint32_t* meta = (uint32_t*)(ws + p.meta);
  uint32_t* lens = (uint32_t*)(ws + p.lens);
  uint32_t* cnt = (uint32_t*)(ws + p.cnt);
  uint8_t* bits = ws + p.bits;
  const uint32_t lens_stride = (uint32_t)p.lens_stride, cnt_stride = (uint32_t)p.cnt_stride;
  const dim3 per_block((g.nb + 255u) / 256u, (unsigned)B);
  // the workgroups that share a frame's string out: enough for the longest, a loop for the rest
  const uint64_t most16 = p.bits_stride / 16u;
  const dim3 per_zero((unsigned)((most16 + 255u) / 256u < 64u ? (most16 + 255u) / 256u : 64u), (unsigned)B);
  const dim3 per_chunk((unsigned)((p.cnt_stride + 3u) / 4u < 128u ? (p.cnt_stride + 3u) / 4u : 128u), (unsigned)B);
  hipLaunchKernelGGL(jenc_count_kernel, per_block, dim3(256), 0, s, coef, g, lens, lens_stride);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_entropy_encode_dev (count)");
  hipLaunchKernelGGL(jenc_scan_kernel, dim3((unsigned)B), dim3(1024), 0, s, lens, lens_stride, g.nb, meta);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_entropy_encode_dev (scan)");
  hipLaunchKernelGGL(jenc_zero_kernel, per_zero, dim3(256), 0, s, bits, p.bits_stride, (const uint32_t*)meta);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_entropy_encode_dev (zero)");
  hipLaunchKernelGGL(jenc_write_kernel, per_block, dim3(256), 0, s, coef, g, (const uint32_t*)lens, lens_stride, bits, p.bits_stride);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_entropy_encode_dev (write)");
  hipLaunchKernelGGL(jenc_ff_count_kernel, per_chunk, dim3(256), 0, s, (const uint8_t*)bits, p.bits_stride, (const uint32_t*)meta, cnt,
                     cnt_stride);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_entropy_encode_dev (FF count)");
  hipLaunchKernelGGL(jenc_ff_scan_kernel, dim3((unsigned)B), dim3(1024), 0, s, cnt, cnt_stride, meta, header_bytes, cap, nbytes, status);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_entropy_encode_dev (FF scan)");
  hipLaunchKernelGGL(jenc_emit_kernel, per_chunk, dim3(256), 0, s, (const uint8_t*)bits, p.bits_stride, (const uint32_t*)meta,
                     (const uint32_t*)cnt, cnt_stride, (const uint8_t*)header, header_bytes, files, cap);
  ACX_CHECK_LAUNCH(ctx, "acx_jpeg_entropy_encode_dev (emit)");
  return ACX_OK;
}
