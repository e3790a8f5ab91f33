// acx_attention -- exact-f32 multi-head attention for head dim 64: attn_kernel (short sequences, <= 224, causal or not) and
// attn16_kernel (the ViT sequence, 129 <= L <= 1024)
// (included by acx_attn.hip inside its anonymous namespace)
//
// attn_kernel, CDNA4 design (one workgroup = one (sequence, head), 4 wavefronts, one per SIMD):
//   * K and V of the head are staged ONCE in LDS as f32 (L=197: 2 x 224 x 64 x 4 B = 112 KiB of
//     the CU's 160 KiB).  K rows are padded to 272 B so the 16-lane groups of ds_read_b128 hit
//     16 distinct 16-B slots; V is read with ds_read_b32 (32 consecutive floats per half-wave).
//   * each wave owns 32-query blocks.  Scores are computed TRANSPOSED, S^T = K Q^T, with
//     v_mfma_f32_32x32x2_f32 (exact f32): in the 32x32 C layout a lane then holds one QUERY
//     column (col = lane&31) and 16 keys per tile, so the softmax row reduction is in-register
//     plus ONE cross-half exchange, and P^T registers are directly the A operand of the P.V MFMA
//     (lane half h of register r holds key (r&3)+8(r>>2)+4h -- the V row each half fetches).
//   * K-permutation trick as in acx_gemm: one ds_read_b128 of K feeds four MFMAs.
constexpr int KROW = 68;   // floats per K row in LDS (64 + 4 pad = 272 B)
constexpr int VROW = 64;

template <int NT, int NW>
__global__ __launch_bounds__(NW * 64, NW / 4) void attn_kernel(const float* __restrict__ qkv, int64_t ldqkv,
                                                      float* __restrict__ out, int64_t ldo, int L, int heads,
                                                      int causal) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sK = reinterpret_cast<float*>(smem);
  float* sV = sK + NT * 32 * KROW;
  float* sL = sV + NT * 32 * VROW;   // [NW waves][32] row sums
  int* vflag = reinterpret_cast<int*>(sL + NW * 32);   // STAGGER: number of waves that have finished staging V

  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int W = heads * 64;
  const float* base = qkv + (int64_t)b * L * ldqkv + h * 64;
  const int t = threadIdx.x;

  // ---- stage K, V (rows >= L zero-filled): ALL global loads are issued before the first LDS write so the
  // staging costs one memory round trip, not one per iteration.
  // STAGGER (8 waves, one query block each): only K is staged up front; the second wave of every SIMD (waves 4-7)
  // then stages V while the first (waves 0-3) is already in QK^T, and one barrier in front of P.V publishes V.
  // The two waves of a SIMD thereby run out of phase -- one's softmax (VALU) under the other's MFMAs -- instead of
  // both doing QK^T, then both softmax with the matrix pipe idle, then both P.V.  V is published through an LDS
  // counter, not a barrier, so the phase shift survives until the end of the block.
  constexpr bool STAGGER = NW == 8;
  constexpr int NSTG = (NT * 32 * 16 + NW * 64 - 1) / (NW * 64);
  {
    float4 stk[NSTG], stv[NSTG];
#pragma unroll
    for (int j = 0; j < NSTG; ++j) {
      const int i = t + j * NW * 64;
      const int row = i >> 4, c4 = i & 15;
      stk[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      stv[j] = stk[j];
      if (i < NT * 32 * 16 && row < L) {
        const float* p = base + (int64_t)row * ldqkv + 4 * c4;
        stk[j] = *reinterpret_cast<const float4*>(p + W);
        if constexpr (!STAGGER) stv[j] = *reinterpret_cast<const float4*>(p + 2 * W);
      }
    }
#pragma unroll
    for (int j = 0; j < NSTG; ++j) {
      const int i = t + j * NW * 64;
      const int row = i >> 4, c4 = i & 15;
      if (i < NT * 32 * 16) {
        *reinterpret_cast<float4*>(sK + row * KROW + 4 * c4) = stk[j];
        if constexpr (!STAGGER) *reinterpret_cast<float4*>(sV + row * VROW + 4 * c4) = stv[j];
      }
    }
  }
  if constexpr (STAGGER) { if (t == 0) *vflag = 0; }
  __syncthreads();
  if constexpr (STAGGER) {
    if (t >= 256) {
      constexpr int NSV = (NT * 32 * 16 + 255) / 256;
      float4 stv[NSV];
#pragma unroll
      for (int j = 0; j < NSV; ++j) {
        const int i = (t - 256) + j * 256;
        const int row = i >> 4, c4 = i & 15;
        stv[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < NT * 32 * 16 && row < L) stv[j] = *reinterpret_cast<const float4*>(base + (int64_t)row * ldqkv + 4 * c4 + 2 * W);
      }
#pragma unroll
      for (int j = 0; j < NSV; ++j) {
        const int i = (t - 256) + j * 256;
        if (i < NT * 32 * 16) *reinterpret_cast<float4*>(sV + (i >> 4) * VROW + 4 * (i & 15)) = stv[j];
      }
      // publish (LDS ops of a wave complete in order; the counter is bumped after this wave's V writes) and
      // fall behind the first wave of this SIMD by about one QK^T phase
      __threadfence_block();
      if ((t & 63) == 0) atomicAdd(vflag, 1);
      __builtin_amdgcn_s_sleep(100);     // ~6.4k cycles; measured optimum (0 / 6.4k / 12.8k / 19.2k: -2.5 / -3.9 / -2.4 / 0 %)
    }
  }

  const int lane = t & 63, wave = t >> 6;
  const int li = lane & 31, hh = lane >> 5;
  const int nqb = (L + 31) / 32;

  for (int qb = wave; qb < (STAGGER ? NW : nqb); qb += NW) {      // STAGGER: exactly one trip per wave (nqb <= 8)
    const bool has = qb < nqb;
    const int q0 = qb * 32;
    // ---- Q fragment (B operand of S^T = K.Q^T): lane (q=li, half hh) holds chunks (2c+hh)
    float4 qf[8];
    {
      const int q = q0 + li;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < L) v = *reinterpret_cast<const float4*>(base + (int64_t)q * ldqkv + (2 * c + hh) * 4);
        v.x *= 0.125f; v.y *= 0.125f; v.z *= 0.125f; v.w *= 0.125f;   // 64^-0.5, exact
        qf[c] = v;
      }
    }
    const int t_hi = !has ? 0 : (causal ? min(NT, (q0 + 31) / 32 + 1) : NT);   // key tiles that can be visible (none: idle wave)

    f32x16 st[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) st[kt][e] = 0.f;
      if (kt < t_hi) {
        const float* kp = sK + (kt * 32 + li) * KROW + hh * 4;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float4 kf = *reinterpret_cast<const float4*>(kp + c * 8);
          st[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[c].x, st[kt], 0, 0, 0);
          st[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[c].y, st[kt], 0, 0, 0);
          st[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[c].z, st[kt], 0, 0, 0);
          st[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[c].w, st[kt], 0, 0, 0);
        }
      }
    }
    // ---- softmax over keys for query (q0 + li): keys live in registers (kt, r) and lane half hh
    const int qglob = q0 + li;
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        const bool ok = key < L && (!causal || key <= qglob) && kt < t_hi;
        st[kt][r] = ok ? st[kt][r] : -INFINITY;
        mx = fmaxf(mx, st[kt][r]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = __expf(st[kt][r] - mx);   // exp(-inf) = 0 for masked keys
        st[kt][r] = p;
        sum += p;
      }
    }
    sum += __shfl_xor(sum, 32, 64);
    if (hh == 0) sL[wave * 32 + li] = sum;

    if constexpr (STAGGER) {                     // V (staged by waves 4-7 meanwhile) is complete: no barrier, the waves stay out of phase
      while (*reinterpret_cast<volatile int*>(vflag) < 4) __builtin_amdgcn_s_sleep(2);
    }
    // ---- O = P.V : A operand = P^T registers as they are, B operand = V rows from LDS
    f32x16 o[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { o[0][e] = 0.f; o[1][e] = 0.f; }
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      if (kt < t_hi) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
          const float v0 = sV[key * VROW + li];
          const float v1 = sV[key * VROW + 32 + li];
          o[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(st[kt][r], v0, o[0], 0, 0, 0);
          o[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(st[kt][r], v1, o[1], 0, 0, 0);
        }
      }
    }
    // ---- normalise and store: o[dt] C layout: col = d = 32*dt + li, row = query (r&3)+8(r>>2)+4hh
    // (sL written by this wave above; same-wave LDS ops are ordered, no barrier needed)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ql = (r & 3) + 8 * (r >> 2) + 4 * hh;
      const int q = q0 + ql;
      if (q < L) {
        const float inv = 1.f / sL[wave * 32 + ql];
        float* op = out + ((int64_t)b * L + q) * ldo + h * 64 + li;
        op[0] = o[0][r] * inv;
        op[32] = o[1][r] * inv;
      }
    }
  }
}


// =====================================================================================================
// attn16_kernel -- exact-f32 attention for the ViT sequence (non-causal, 129 <= L <= 1024; L = 197 for ViT-B/16, 257 / 577 for
// ViT-L/14 at 224 / 336 pixels).
//
// What limited attn_kernel<7,8> (0.43 of the f32 MFMA roof): 197 tokens padded to 7 x 32 (29 % padded MFMA work),
// 7 query blocks on 4 SIMDs, and ONE 112 KiB workgroup per CU, so nothing overlaps a workgroup's K/V staging,
// softmax or store phases.  This kernel
//   * tiles with v_mfma_f32_16x16x4_f32: 197 -> 13 x 16 = 208 (11 % padding); a wave owns TWO 16-query tiles (one
//     K / V fragment read feeds both), 7 waves per (frame, head) workgroup;
//   * streams K and V through LDS in 32-key chunks (16 KB per stage, two stages) by LDS-DMA (global_load_lds_dwordx4,
//     bank swizzle of K on the SOURCE address), flash-style online softmax in between -- 32 KB of LDS and <= 128 VGPRs,
//     so TWO workgroups share a CU: one workgroup's DMA waits, barriers, softmax VALU work and output stores sit
//     under the other's MFMAs;
//   * keeps the transposed-score trick: S^T = K Q^T puts a lane's QUERY in the MFMA column (lane & 15), so row
//     max / sum are per-lane scalars (+ two cross-row exchanges, v_permlane16/32_swap: no LDS), P^T registers are
//     directly the B operand of O^T = V^T P^T, and with the output-column permutation d = 4 i + e (MFMA e of a group
//     computes output tile e) one ds_read_b128 of V feeds four MFMAs per query tile and a lane ends up with 16
//     CONTIGUOUS floats of its query's output row.
// Online softmax changes the summation order and the scaling sequence only (exp(s - m) rescaled by exp(m - m')):
// differences to the two-pass form are f32 round-off (tests: 3e-6 against fp64).
#ifndef ACX_A16_KT
#define ACX_A16_KT 2
#endif
constexpr int A16_KT = ACX_A16_KT;                  // 16-key tiles per staged chunk
constexpr int A16_CHUNK = 16 * A16_KT;              // keys per staged chunk
constexpr int A16_OP_B = A16_CHUNK * 256;           // one operand chunk: rows of 64 f32
constexpr int A16_STAGE_B = 2 * A16_OP_B;           // K | V

typedef __attribute__((address_space(3))) void a16_lds_t;

// max / sum over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48): v_permlane16_swap exchanges odd rows of
// its first operand with even rows of the second, v_permlane32_swap the upper half of the first with the lower half
// of the second; with both operands = x the two results hold x of this row pair's even and odd member.
typedef unsigned a16_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float a16_rowmax(float x) {
  a16_u2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float a16_rowsum(float x) {
  a16_u2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  x = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// One wave's share of a workgroup's items.  HB: the wave owns two query tiles (ta, tb) or one (ta).
// x3plane > 0: the output is written as three bf16 planes hi | mid | lo (ACX_BF16X3; plane p at (u16*)out + p * x3plane): the A
// operand of the out-projection in ACX_PREC_F32X6 mode
// prows > 0: the planes are in K-panel layout (ACX_BF16X3P: [ldo / 32][prows][32])
__device__ __forceinline__ void a16_store4(float* out, int64_t row, int col, int64_t ldo, int64_t x3plane, int64_t prows, float a, float b,
                                           float c, float d) {
  const int64_t off = prows > 0 ? ((int64_t)(col >> 5) * prows + row) * 32 + (col & 31) : row * ldo + col;
  if (x3plane > 0) {
    const float ov[4] = {a, b, c, d};
    u16 hh[4], mm[4], ll[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hh[k] = f2bf(ov[k]);
      const float r1 = ov[k] - bf2f(hh[k]);
      mm[k] = f2bf(r1);
      ll[k] = f2bf(r1 - bf2f(mm[k]));
    }
    u16* o3 = reinterpret_cast<u16*>(out) + off;
    uint2 pk;
    pk.x = (uint32_t)hh[0] | ((uint32_t)hh[1] << 16); pk.y = (uint32_t)hh[2] | ((uint32_t)hh[3] << 16);
    *reinterpret_cast<uint2*>(o3) = pk;
    pk.x = (uint32_t)mm[0] | ((uint32_t)mm[1] << 16); pk.y = (uint32_t)mm[2] | ((uint32_t)mm[3] << 16);
    *reinterpret_cast<uint2*>(o3 + x3plane) = pk;
    pk.x = (uint32_t)ll[0] | ((uint32_t)ll[1] << 16); pk.y = (uint32_t)ll[2] | ((uint32_t)ll[3] << 16);
    *reinterpret_cast<uint2*>(o3 + 2 * x3plane) = pk;
  } else {
    *reinterpret_cast<float4*>(out + off) = make_float4(a, b, c, d);
  }
}

// QB: items are (query block, sequence, head), query block major: block qb of a sequence owns the 16-query tiles
// [qb qsz + min(qb, qrem), + qsz + (qb < qrem)) (ta / tb count from there); the wave visits items item0, item0 + gridDim.x, ... < nitems.
// !QB: items are (sequence, head), the block is the whole sequence, item0 = blockIdx.x.
template <bool HB, int NW, bool QB = false>
__device__ __forceinline__ void a16_run(const float* __restrict__ qkv, int64_t ldqkv, float* __restrict__ out, int64_t ldo,
                                        int L, int heads, int nitems, char* smem, int ta, int tb, int64_t x3plane, int64_t prows,
                                        int item0 = 0, int nbh = 1, int qsz = 0, int qrem = 0) {
  const int W = heads * 64;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  constexpr int nw = NW;                            // waves per workgroup
  const int qi = lane & 15, g = lane >> 4;
  const int nkt = (L + 15) >> 4;                    // 16-key tiles ( = 16-query tiles)
  const int nch = (nkt + A16_KT - 1) / A16_KT;      // chunks

  // ---- DMA plan: a chunk is 8 KT wave-instructions of 1 KB (4 rows x 256 B): first the K rows, then the V rows;
  // wave w issues instructions w, w + nw, ... (8 KT instructions per chunk, nw = 8 waves).  K: LDS slot p of row r holds source slot p ^ (r & 15).
  // The DMA goes through inline asm: hipcc (ROCm 7.2) treats a global_load_lds it can see as a pending LDS write that may
  // alias EVERY later ds_read and drains it (s_waitcnt vmcnt(0)) in front of the first fragment read of the same
  // iteration -- the next chunk's DMA would never overlap this chunk's MFMAs.  An asm statement is opaque to that
  // bookkeeping; its completion is counted by hand (vmcnt(0) + barrier at the end of each chunk; the loop has no
  // other VMEM operation).  M0 (LDS destination base, wave-uniform) is written and restored inside the statement.
  const unsigned lds0 = (unsigned)(uintptr_t)(a16_lds_t*)smem;
#define A16_DMA(gptr, ldsaddr)                                                                                   \
  do {                                                                                                           \
    unsigned keep_;                                                                                              \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep_) : "v"(gptr), "s"(ldsaddr) : "memory");                                           \
  } while (0)
#define A16_ISSUE1(stage, ch, i_)                                                                                \
  do {                                                                                                           \
    const int ii_ = (i_);                                           /* wave-uniform */                           \
    if (ii_ < 8 * A16_KT) {                                                                                      \
      const int r_ = 4 * (ii_ % (4 * A16_KT)) + g;                                                               \
      const int e_ = ii_ < 4 * A16_KT ? W + 4 * (qi ^ (r_ & 15)) : 2 * W + 4 * qi;                                \
      A16_DMA(bp_ + (int64_t)min((ch) * A16_CHUNK + r_, L - 1) * ldqkv + e_,                                     \
              lds0 + (stage) * A16_STAGE_B + ii_ * 1024);                                                        \
    }                                                                                                            \
  } while (0)
#define A16_ISSUE(bp, stage, ch)                                                                                 \
  do { const float* bp_ = (bp);                                                                                  \
       _Pragma("unroll") for (int j_ = 0; j_ < (8 * A16_KT + nw - 1) / nw; ++j_) A16_ISSUE1(stage, ch, wave + j_ * nw); } while (0)
  // K fragment address: row (tile-local key = lane & 15), slot (4 c4 + g) ^ (key & 15) = ((g ^ qi) ^ 4 c4): the four
  // slots differ by an XOR of the byte offset with 64 c4.  V: row (4 g + r), slot qi (d = 4 qi ..), linear image.
  const int ka = qi * 256 + ((g ^ qi) * 16);
  const int va = A16_OP_B + (4 * g) * 256 + qi * 16;

  // ---- persistent over (frame, head) items; the first chunk of the NEXT item is in flight while this item's output
  // is normalised and stored
  // (sequence, head) of an item and the first query row of its block
  auto bh_of = [&](int it) { return QB ? it % nbh : it; };
  auto q0_of = [&](int it) { if constexpr (QB) { const int qb_ = it / nbh; return 16 * (qb_ * qsz + min(qb_, qrem)); } else { return 0; } };
  int item = QB ? item0 : (int)blockIdx.x;
  if (item < nitems) A16_ISSUE(qkv + (int64_t)(bh_of(item) / heads) * L * ldqkv + (bh_of(item) % heads) * 64, 0, 0);
  for (; item < nitems; item += gridDim.x) {
    const int b = bh_of(item) / heads, h = bh_of(item) % heads;
    const int q0 = q0_of(item);
    const float* base = qkv + (int64_t)b * L * ldqkv + h * 64;
    // ---- Q fragments (B operand of S^T = K Q^T): lane (query qi, k-group g) holds d = 16 c4 + 4 g + (0..3)
    float4 qa[4], qb[4];
    {
      const float* pa = base + (int64_t)min(q0 + 16 * ta + qi, L - 1) * ldqkv + 4 * g;
      const float* pb = base + (int64_t)min(q0 + 16 * tb + qi, L - 1) * ldqkv + 4 * g;
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        float4 v = *reinterpret_cast<const float4*>(pa + 16 * c4);
        v.x *= 0.125f; v.y *= 0.125f; v.z *= 0.125f; v.w *= 0.125f;     // 64^-0.5, exact
        qa[c4] = v;
        if constexpr (HB) {
          v = *reinterpret_cast<const float4*>(pb + 16 * c4);
          v.x *= 0.125f; v.y *= 0.125f; v.z *= 0.125f; v.w *= 0.125f;
          qb[c4] = v;
        }
      }
    }
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 oa0 = z4, oa1 = z4, oa2 = z4, oa3 = z4;                         // O^T tiles e = 0..3 (d = 16 g + 4 reg + e)
    f32x4 ob0 = z4, ob1 = z4, ob2 = z4, ob3 = z4;
    float ma = -INFINITY, la = 0.f, mb = -INFINITY, lb = 0.f;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int ch = 0; ch < nch; ++ch) {
      if (ch + 1 < nch) A16_ISSUE(base, (ch + 1) & 1, ch + 1);
      const char* sS = smem + (ch & 1) * A16_STAGE_B;
      // ---- two 16-key tiles per chunk, each: S^T tiles of the wave's query tiles -> online softmax -> O^T += V^T P^T
#define A16_QK(c4, off, toff)                                                                                   \
  do {                                                                                                           \
    const float4 k_ = *reinterpret_cast<const float4*>(sS + (ka ^ (off)) + (toff));                              \
    sa = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.x, qa[c4].x, sa, 0, 0, 0);                                       \
    if constexpr (HB) sb = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.x, qb[c4].x, sb, 0, 0, 0);                     \
    sa = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.y, qa[c4].y, sa, 0, 0, 0);                                       \
    if constexpr (HB) sb = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.y, qb[c4].y, sb, 0, 0, 0);                     \
    sa = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.z, qa[c4].z, sa, 0, 0, 0);                                       \
    if constexpr (HB) sb = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.z, qb[c4].z, sb, 0, 0, 0);                     \
    sa = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.w, qa[c4].w, sa, 0, 0, 0);                                       \
    if constexpr (HB) sb = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.w, qb[c4].w, sb, 0, 0, 0);                     \
  } while (0)
#define A16_SOFTMAX(S, M, LS, O0, O1, O2, O3)                                                                    \
  do {                                                                                                           \
    const float mx_ = a16_rowmax(fmaxf(fmaxf(S[0], S[1]), fmaxf(S[2], S[3])));                                   \
    const float mn_ = fmaxf(M, mx_);                                 /* finite: every tile holds >= 1 valid key */ \
    const float al_ = __expf(M - mn_);                               /* first tile: exp(-inf) = 0 */             \
    M = mn_;                                                                                                     \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) S[r] = __expf(S[r] - mn_);   /* exp(-inf) = 0 for masked keys */ \
    LS = LS * al_ + ((S[0] + S[1]) + (S[2] + S[3]));                                                             \
    if (!__all(al_ == 1.f)) {                                     /* x * 1 == x: skipping is bit-identical */     \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) { O0[r] *= al_; O1[r] *= al_; O2[r] *= al_; O3[r] *= al_; }  \
    }                                                                                                            \
  } while (0)
#define A16_PV(r, toff)                                                                                         \
  do {                                                                                                           \
    const float4 v_ = *reinterpret_cast<const float4*>(sS + va + (toff) + (r) * 256);                            \
    oa0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.x, sa[r], oa0, 0, 0, 0);                                        \
    if constexpr (HB) ob0 = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.x, sb[r], ob0, 0, 0, 0);                      \
    oa1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.y, sa[r], oa1, 0, 0, 0);                                        \
    if constexpr (HB) ob1 = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.y, sb[r], ob1, 0, 0, 0);                      \
    oa2 = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.z, sa[r], oa2, 0, 0, 0);                                        \
    if constexpr (HB) ob2 = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.z, sb[r], ob2, 0, 0, 0);                      \
    oa3 = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.w, sa[r], oa3, 0, 0, 0);                                        \
    if constexpr (HB) ob3 = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.w, sb[r], ob3, 0, 0, 0);                      \
  } while (0)
#define A16_TILE(toff, kbase)                                                                                    \
  do {                                                                                                           \
    f32x4 sa = z4, sb = z4;                                                                                      \
    A16_QK(0, 0, toff); A16_QK(1, 64, toff); A16_QK(2, 128, toff); A16_QK(3, 192, toff);                         \
    if ((kbase) + 16 > L) {                                           /* only the last tile holds keys >= L */   \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                            \
        const bool ok_ = (kbase) + 4 * g + r < L;                                                                \
        sa[r] = ok_ ? sa[r] : -INFINITY; sb[r] = ok_ ? sb[r] : -INFINITY;                                        \
      }                                                                                                          \
    }                                                                                                            \
    A16_SOFTMAX(sa, ma, la, oa0, oa1, oa2, oa3);                                                                 \
    if constexpr (HB) A16_SOFTMAX(sb, mb, lb, ob0, ob1, ob2, ob3);                                               \
    A16_PV(0, toff); A16_PV(1, toff); A16_PV(2, toff); A16_PV(3, toff);                                          \
  } while (0)
      A16_TILE(0, A16_CHUNK * ch);
#pragma unroll
      for (int j = 1; j < A16_KT; ++j)
        if (A16_KT * ch + j < nkt) A16_TILE(j * 16 * 256, A16_CHUNK * ch + 16 * j);
#undef A16_TILE
#undef A16_PV
#undef A16_SOFTMAX
#undef A16_QK
      // next chunk landed (this wave's DMAs) and everybody is done reading this stage
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    // every wave is past its last fragment read (barrier above): stage 0 is free for the next item's first chunk
    {
      const int nxt = item + (int)gridDim.x;
      if (nxt < nitems) A16_ISSUE(qkv + (int64_t)(bh_of(nxt) / heads) * L * ldqkv + (bh_of(nxt) % heads) * 64, 0, 0);
    }
    // ---- normalise and store: lane (query qi, g) holds O[query][16 g + 4 reg + e]
    {
      const float inv = 1.f / a16_rowsum(la);
      const int q = q0 + 16 * ta + qi;
      if (q < L) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          a16_store4(out, (int64_t)b * L + q, h * 64 + 16 * g + 4 * r, ldo, x3plane, prows, oa0[r] * inv, oa1[r] * inv, oa2[r] * inv, oa3[r] * inv);
      }
    }
    if constexpr (HB) {
      const float inv = 1.f / a16_rowsum(lb);
      const int q = q0 + 16 * tb + qi;
      if (q < L) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          a16_store4(out, (int64_t)b * L + q, h * 64 + 16 * g + 4 * r, ldo, x3plane, prows, ob0[r] * inv, ob1[r] * inv, ob2[r] * inv, ob3[r] * inv);
      }
    }
  }   // item loop
#undef A16_ISSUE
#undef A16_ISSUE1
#undef A16_DMA
}

// 8 waves per workgroup; nkt (9..16) query tiles: nd = nkt - 8 waves own two tiles, the others one (L = 197: waves 0..4
// two tiles, 5..7 one).  Measured and rejected on top of this: 13 one-tile waves at <= 64 VGPRs (spills, 0.86 ms), chunks
// of 16 / 64 keys (no change: the chunk barrier is not the limit), s_setprio around the MFMA groups, rotating the
// two-tile waves between co-resident workgroups, dealing the two-tile roles by the SIMD id the waves report (s_getreg
// HW_ID; waves w and w + 4 share a SIMD, tools/probes/wave_simd.hip) so that a CU's SIMDs carry 7/6/7/6 tiles (no
// change), and software-pipelining the softmax inside each wave (scores of key tile j + 1 issued next to the softmax
// of tile j, one 16-key tile per stage, ring of four: 0.785 ms, not faster; hipcc's scheduler clusters the MFMAs
// and sched_group_barrier patterns made it 0.81).  Timing ablations (profiles/r02_attn_ablation.txt):
// no single phase is the limit -- softmax -11 %, DMA -8 %, chunk barrier -6 %, LDS fragment reads -4 %, and with ALL of
// them removed (MFMAs, Q loads and output stores only) the kernel still takes 0.60 ms = 0.73 of the MFMA roof on its
// padded work: 13 tiles on 8 waves, single-accumulator 16x16x4 chains, item prologue / epilogue.
//
// QB (L > 256, up to 1024): the ceil(L / 16) query tiles of a sequence are split into nqb = ceil(nkt / 16) query blocks as evenly
// as possible (L = 257: 9 + 8, L = 577: 13 + 12 + 12, L = 1024: 4 x 16), and an item is (query block, sequence, head).  Every
// block streams all of K and V of its head (the restaging stays in L2); the K / V chunk loop, and so the LDS use, does not depend
// on L.  Blocks of one size share the tile-to-wave deal above; the items are ordered query block major, so the qrem larger blocks
// come first and a workgroup switches its deal at most once.  L <= 256 (!QB) keeps one block per (sequence, head).
template <bool QB>
__global__ __launch_bounds__(512, 4) void attn16_kernel(const float* __restrict__ qkv, int64_t ldqkv, float* __restrict__ out,
                                                        int64_t ldo, int L, int heads, int nitems, int64_t x3plane, int64_t prows) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nkt = (L + 15) >> 4;
  if constexpr (!QB) {
    const int nd = nkt - 8;                                               // waves with two tiles
    const bool dbl = wave < nd;
    const int ta = dbl ? 2 * wave : nd + wave;
    if (dbl) a16_run<true, 8>(qkv, ldqkv, out, ldo, L, heads, nitems, smem, ta, ta + 1, x3plane, prows);
    else a16_run<false, 8>(qkv, ldqkv, out, ldo, L, heads, nitems, smem, ta, ta, x3plane, prows);
  } else {
    const int nqb = (nkt + 15) >> 4;                                      // >= 2: every block holds 8..16 tiles
    const int qsz = nkt / nqb, qrem = nkt - qsz * nqb;
    const int nbh = nitems / nqb;
    const int G = (int)gridDim.x, g0 = (int)blockIdx.x;
    const int hi_a = qrem * nbh;                                          // items [0, hi_a): blocks of qsz + 1 tiles
    const int start_b = g0 >= hi_a ? g0 : g0 + ((hi_a - g0 + G - 1) / G) * G;
#pragma unroll 1
    for (int part = 0; part < 2; ++part) {
      const int n = part == 0 ? qsz + 1 : qsz;
      const int i0 = part == 0 ? g0 : start_b, i1 = part == 0 ? hi_a : nitems;
      if (i0 >= i1) continue;
      const int nd = n - 8;
      const bool dbl = wave < nd;
      const int ta = dbl ? 2 * wave : nd + wave;
      if (dbl) a16_run<true, 8, true>(qkv, ldqkv, out, ldo, L, heads, i1, smem, ta, ta + 1, x3plane, prows, i0, nbh, qsz, qrem);
      else a16_run<false, 8, true>(qkv, ldqkv, out, ldo, L, heads, i1, smem, ta, ta, x3plane, prows, i0, nbh, qsz, qrem);
    }
  }
}
