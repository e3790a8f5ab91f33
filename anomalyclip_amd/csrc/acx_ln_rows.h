// Row arithmetic of the LayerNorm kernels, shared between acx_norm.hip (layernorm_kernel, layernorm_panel2_kernel, ...) and the
// LayerNorm RIDER of the plane-reuse GEMM (acx_gemm_x6.h): ONE expression tree per quantity, so that hipcc's contraction choices
// -- and the bits of a row's planes -- are the same whichever kernel produced the row.
#pragma once
#include "acx_internal.h"

template <int VPL>
__device__ __forceinline__ void normalize(float (&v)[VPL], float eps, int mode) {
  constexpr float invD = 1.f / (64 * VPL);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) s += v[i];
  const float mean = wave_sum(s) * invD;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    v[i] -= mean;
    q += v[i] * v[i];
  }
  const float var = wave_sum(q) * invD;
  const float scale = mode == ACX_NORM_LAYER ? 1.f / sqrtf(var + eps) : 1.f / (sqrtf(var) + eps);
#pragma unroll
  for (int i = 0; i < VPL; ++i) v[i] *= scale;
}

// the affine parameters of the elements a lane owns (load_row's layout: float4 groups at 4 lane + 256 i)
template <int VPL>
__device__ __forceinline__ void ln_load_affine(const float* __restrict__ w, const float* __restrict__ b, int lane, float4 (&ww)[VPL / 4],
                                               float4 (&bb)[VPL / 4]) {
#pragma unroll
  for (int i = 0; i < VPL / 4; ++i) {
    ww[i] = *reinterpret_cast<const float4*>(w + 4 * lane + 256 * i);
    bb[i] = *reinterpret_cast<const float4*>(b + 4 * lane + 256 * i);
  }
}

// K-panel planes (ACX_BF16X3P) of the row PAIR r0 (even), r0 + 1 held by one wave (va / vb: the normalised rows in load_row's
// layout): lane pairs trade halves -- the even lane of a pair ends up with eight consecutive elements of row r0, the odd lane
// with the same eight of row r0 + 1 -- so that eight lanes write the 128 contiguous bytes the two rows occupy in a panel with
// 16-byte stores.  `rows` is the plane's TOTAL row count (element e of row r at ((e / 32) rows + r) 32 + e % 32, plane p at
// y + p rows 64 VPL); two = false: row r0 + 1 does not exist (vb is a copy of va, nothing is stored for it).
// TWO (ACX_BF16X2P): the hi and mid planes only;  F16 (ACX_F16X2P): two fp16 planes hi | lo instead of bf16 planes -- of sc * y,
// sc a power of two (exact: the caller's proof that sc * y stays inside fp16's range; the bf16 planes do not read sc)
template <int VPL, bool TWO, bool F16>
__device__ __forceinline__ void ln_panel2_store(const float (&va)[VPL], const float (&vb)[VPL], const float4 (&wv)[VPL / 4],
                                                const float4 (&bv)[VPL / 4], u16* __restrict__ y, int64_t rows, int64_t r0, bool two,
                                                int lane, float sc = 1.f) {
  const int64_t plane = rows * (int64_t)(64 * VPL);
  const int odd = lane & 1;
#pragma unroll
  for (int i = 0; i < VPL / 4; ++i) {
    const float4 ww = wv[i];
    const float4 bb = bv[i];
    float oa[4] = {va[4 * i] * ww.x + bb.x, va[4 * i + 1] * ww.y + bb.y, va[4 * i + 2] * ww.z + bb.z, va[4 * i + 3] * ww.w + bb.w};
    float ob[4] = {vb[4 * i] * ww.x + bb.x, vb[4 * i + 1] * ww.y + bb.y, vb[4 * i + 2] * ww.z + bb.z, vb[4 * i + 3] * ww.w + bb.w};
    // the pair (2 j, 2 j + 1) holds elements 8 j .. 8 j + 7 of both rows: even keeps row a (own four + the odd lane's four), odd row b
    float o8[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float give = odd ? oa[k] : ob[k];                                    // what the partner needs from this lane
      const float got = __shfl_xor(give, 1, 64);
      o8[k] = odd ? got : oa[k];                                                 // elements 8 j + k
      o8[4 + k] = odd ? ob[k] : got;                                             // elements 8 j + 4 + k
    }
    u16 hh[8], mm[8], ll[8];
    if constexpr (F16) {
#pragma unroll
      for (int k = 0; k < 8; ++k) o8[k] *= sc;
#pragma unroll
      for (int k = 0; k < 8; k += 2) {
        const uint32_t ph_ = f2h2(o8[k], o8[k + 1]);
        const uint32_t pl_ = f2h2(o8[k] - h2f_lo(ph_), o8[k + 1] - h2f_hi(ph_));
        hh[k] = (u16)(ph_ & 0xffffu); hh[k + 1] = (u16)(ph_ >> 16);
        mm[k] = (u16)(pl_ & 0xffffu); mm[k + 1] = (u16)(pl_ >> 16);
        ll[k] = ll[k + 1] = 0;
      }
    } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      hh[k] = f2bf(o8[k]);
      const float r1 = o8[k] - bf2f(hh[k]);
      mm[k] = f2bf(r1);
      ll[k] = f2bf(r1 - bf2f(mm[k]));
    }
    }
    const int e8 = 8 * (lane >> 1) + 256 * i;
    const int64_t row = r0 + odd;
    if (odd && !two) continue;
    u16* dst = y + ((int64_t)(e8 >> 5) * rows + row) * 32 + (e8 & 31);
#define LNP_PACK(a) make_uint4((uint32_t)a[0] | ((uint32_t)a[1] << 16), (uint32_t)a[2] | ((uint32_t)a[3] << 16), \
                               (uint32_t)a[4] | ((uint32_t)a[5] << 16), (uint32_t)a[6] | ((uint32_t)a[7] << 16))
    *reinterpret_cast<uint4*>(dst) = LNP_PACK(hh);
    *reinterpret_cast<uint4*>(dst + plane) = LNP_PACK(mm);
    if constexpr (!TWO) *reinterpret_cast<uint4*>(dst + 2 * plane) = LNP_PACK(ll);
#undef LNP_PACK
  }
}

// The LayerNorm job a pairs = 6 product carries for the workgroups of its last round that have no tile (acx_gemm_ln): rows
// row0 .. row0 + nrows (both even) of x [*, 64 VPL] -> ACX_BF16X3P planes y of `rows` rows, or (f16 != 0) the two ACX_F16X2P
// planes of ysc * y.
struct LnRide {
  const float* x; const float* w; const float* b;
  u16* y;
  long long ldx, rows, row0, nrows;
  float eps;
  int mode, vpl;
  float ysc; int f16;
};

// One rider workgroup (4 waves; ordinal `rider` of `nriders`): the job's row PAIRS are divided into contiguous ranges, one per
// wave, so that the riders end together.  A wave keeps GP row pairs in flight: the next group's rows are requested before the
// current group is normalised and stored (one workgroup per CU: nothing else hides the latency).
template <int VPL>
__device__ __forceinline__ void ln_ride_rows(const LnRide& j, int rider, int nriders, int wave, int lane) {
  constexpr int GP = 2;
  const long long npairs = j.nrows >> 1, nw = 4ll * nriders, wv = 4ll * rider + wave;
  const long long per = (npairs + nw - 1) / nw;
  const long long p0 = wv * per, p1 = p0 + per < npairs ? p0 + per : npairs;
  if (p0 >= p1) return;
  float4 ww[VPL / 4], bb[VPL / 4];
  ln_load_affine<VPL>(j.w, j.b, lane, ww, bb);
  float cur[GP][2][VPL], nxt[GP][2][VPL];
#define LN_RIDE_LOAD(BUF, p)                                                                        \
  _Pragma("unroll") for (int u = 0; u < GP; ++u) {                                                  \
    const long long r_ = j.row0 + 2 * ((p) + u < p1 ? (p) + u : p1 - 1);   /* past the range: re-read its last pair (never stored) */ \
    load_row<VPL>(j.x + r_ * j.ldx, lane, BUF[u][0]);                                               \
    load_row<VPL>(j.x + (r_ + 1) * j.ldx, lane, BUF[u][1]);                                         \
  }
  LN_RIDE_LOAD(cur, p0);
  for (long long p = p0; p < p1; p += GP) {
    LN_RIDE_LOAD(nxt, p + GP);                    // (unconditional: straight-line loads keep hipcc's waits counted)
#pragma unroll
    for (int u = 0; u < GP; ++u) {
      if (p + u < p1) {
        normalize<VPL>(cur[u][0], j.eps, j.mode);
        normalize<VPL>(cur[u][1], j.eps, j.mode);
        if (j.f16) ln_panel2_store<VPL, true, true>(cur[u][0], cur[u][1], ww, bb, j.y, j.rows, j.row0 + 2 * (p + u), true, lane, j.ysc);
        else ln_panel2_store<VPL, false, false>(cur[u][0], cur[u][1], ww, bb, j.y, j.rows, j.row0 + 2 * (p + u), true, lane);
      }
    }
#pragma unroll
    for (int u = 0; u < GP; ++u)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < VPL; ++i) cur[u][h][i] = nxt[u][h][i];
  }
#undef LN_RIDE_LOAD
}
