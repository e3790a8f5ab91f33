// attn_p3_kernel --the ViT's attention on the bf16 matrix cores at f32 accuracy (the ACX_PREC_F32X6 mode of the layer loop).
// q, k, v arrive as THREE bf16 planes each (hi | mid | lo: exact 24-bit split of the f32 values, written by the in-projection's
// epilogue in K-panel layout ACX_BF16X3P: plane = [3 W / 32][rows][32]); S = Q K^T and O = P V are six-product bf16 x 6
// products with f32 accumulation (acx_gemm_desc.pairs), the softmax runs in f32 in registers, P is split into three planes as
// it is consumed.  The f32 MFMA kernel above is bounded by the f32 pipe (1/16 of the bf16 rate): 61 GFLOP per layer at 157
// TFLOP/s = 0.39 ms at best (0.73-0.88 measured); here the same layer is 2 x 6 x 30.5 GFLOP of bf16 work = 0.15 ms of pipe time.
//   * one workgroup (8 waves, one per CU: 156 KB of LDS) per (frame, head), persistent; waves 0..6 own the seven 32-query
//     tiles of L = 197, wave 7 stages the operands: K and V of the head are copied by LDS-DMA from the panel-layout planes -- a
//     (plane, panel) block is 197 contiguous rows of 64 B, so the LDS image IS the global image (13 instructions of 1 KB per
//     block; K with the source-side bank swizzle chunk ^ ((row >> 2) & 3) of the GEMM units);
//   * phase A: S^T = K Q^T per 32-key tile (A operand = K rows from LDS by ds_read_b128, B operand = this wave's Q fragments,
//     loaded once per item from global): a lane then holds ONE query's scores (col = lane & 31), half of the keys each for the
//     two lane halves -- row max / sum are in-register plus one cross-half exchange;
//   * phase B: O^T = V^T P^T per 16-key step: the B operand is the lane's own probabilities, converted to bf16 planes in the
//     order the accumulator holds them (k-slot j of lane half hh <-> key 4 hh + (j & 3) + 8 (j >> 2) of the step: no lane
//     exchange), the A operand V^T by LDS transpose reads (ds_read_b64_tr_b16) in the SAME key order;
//   * K of item i + 1 is staged while item i is in phase B, V of item i + 1 while it is in phase A (two barriers per item).
// Output: three bf16 planes of O in K-panel layout (the out-projection's A operand), 8 bytes per lane and plane.
// (included by acx_attn.hip inside its anonymous namespace, behind acx_attn_f32.h)
#ifndef AP3_TRACE
#define AP3_TRACE 0
#endif
constexpr int AP3_ROWS = 208;                         // key rows staged per (plane, panel) block: 13 DMA instructions of 16 rows
constexpr int AP3_BLK_B = AP3_ROWS * 64;              // 13312
constexpr int AP3_LDS_B = 12 * AP3_BLK_B;             // K: 6 blocks (plane, panel), V: 6 blocks = 159744

typedef short ap3_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) ap3_s16x4 ap3_lds_s16x4;
typedef __attribute__((address_space(3))) void ap3_lds_void;

template <int F16 = 0>
__device__ __forceinline__ void ap3_split8(const float (&p)[8], bf16x8& hi, bf16x8& mid, bf16x8& lo) {
  uint32_t h[4], m[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = acx_pk2<F16>(p[2 * e], p[2 * e + 1]);
    const float r0 = p[2 * e] - acx_unpk_lo<F16>(h[e]), r1 = p[2 * e + 1] - acx_unpk_hi<F16>(h[e]);
    m[e] = acx_pk2<F16>(r0, r1);
    l[e] = f2bf2(r0 - acx_unpk_lo<F16>(m[e]), r1 - acx_unpk_hi<F16>(m[e]));
  }
  typedef uint32_t u32x4_ __attribute__((ext_vector_type(4)));
  const u32x4_ hv = {h[0], h[1], h[2], h[3]}, mv = {m[0], m[1], m[2], m[3]}, lv = {l[0], l[1], l[2], l[3]};
  hi = __builtin_bit_cast(bf16x8, hv); mid = __builtin_bit_cast(bf16x8, mv); lo = __builtin_bit_cast(bf16x8, lv);
}

// NPROD = 3 (ACX_PREC_F32X3): the three leading products of both contractions only -- (hi, mid) (mid, hi) (hi, hi); the lo planes of
// K and V are neither staged nor read, P is split into two planes, the output's lo plane is not written (its consumer does not read it)
// F16 (with NPROD = 3: ACX_PREC_F16X3): the planes are TWO fp16 planes (hi | lo of the two-plane fp16 split), the products run on
// v_mfma_f32_32x32x16_f16, P and the output are split into fp16 pairs
template <int F16>
__device__ __forceinline__ f32x16 ap3_mfma(const bf16x8 a, const bf16x8 b, const f32x16 c) {
  if constexpr (F16 != 0) {
    typedef _Float16 ap3_h8 __attribute__((ext_vector_type(8)));
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(ap3_h8, a), __builtin_bit_cast(ap3_h8, b), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
}
// the f32-input arm's staging task of a lane (attn_p3_kernel<6, 0, 1>) in wave-iteration wi of K (col0 = W + 64 h) or V (col0 = 2 W +
// 64 h) of the item whose first row is row0: 8 consecutive d of key row 8 wi + ((lane >> 2) & 7), panel lane >> 5, chunk lane & 3
__device__ __forceinline__ const float4* ap3f_src(const float* __restrict__ qkv, int64_t ld, int64_t row0, int col0, int L, int wi, int lane) {
  const int r_ = min(8 * wi + ((lane >> 2) & 7), L - 1);   // behind the sequence: a finite duplicate
  return reinterpret_cast<const float4*>(qkv + (row0 + r_) * ld + (col0 + (lane >> 5) * 32 + (lane & 3) * 8));
}
// ... split into the three planes (ap3_split8: the sequence of the in-projection's plane epilogue) and written to the LDS blocks
// blk0 + 2 p + panel; SWZ: K's chunk swizzle, applied on the LDS side
template <int SWZ>
__device__ __forceinline__ void ap3f_put(char* smem, const float4 a, const float4 b, int blk0, int wi, int lane) {
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  bf16x8 hi, mid, lo;
  ap3_split8<0>(v, hi, mid, lo);
  const int row = 8 * wi + ((lane >> 2) & 7), ch = lane & 3;
  char* dst = smem + (blk0 + (lane >> 5)) * AP3_BLK_B + row * 64 + (SWZ ? (ch ^ ((row >> 2) & 3)) : ch) * 16;
  *reinterpret_cast<bf16x8*>(dst) = hi;
  *reinterpret_cast<bf16x8*>(dst + 2 * AP3_BLK_B) = mid;
  *reinterpret_cast<bf16x8*>(dst + 4 * AP3_BLK_B) = lo;
}
// K of an item by one wave: a rolled loop of two batches of 13 wave-iterations, the batch's 26 loads in flight at once (this code
// shares the kernel's register budget)
__device__ __forceinline__ void ap3f_stage_k(char* smem, const float* __restrict__ qkv, int64_t ld, int64_t row0, int col0, int L, int lane) {
#pragma unroll 1
  for (int w0 = 0; w0 < 26; w0 += 13) {
    float4 ka_[13], kb_[13];
#pragma unroll
    for (int j = 0; j < 13; ++j) { const float4* p_ = ap3f_src(qkv, ld, row0, col0, L, w0 + j, lane); ka_[j] = p_[0]; kb_[j] = p_[1]; }
    __builtin_amdgcn_sched_barrier(0);                  // every load of the batch issued before the first split
#pragma unroll
    for (int j = 0; j < 13; ++j) ap3f_put<1>(smem, ka_[j], kb_[j], 0, w0 + j, lane);
  }
}

// measured staging variants of the f32-input arm, none faster than the default (profiles/attn_f32in_ab.txt): K(next) in batches of n
// wave-iterations, the first loaded in front of B2 and each next one while its predecessor is split (n > 5 spills); a wave's V share
// split and written between phase A's key tiles; Q split behind B1

// F32IN (with NPROD = 6, F16 = 0: acx_attention_p3f): q | k | v arrive as the in-projection's f32 rows -- `qkv3` is that [rows, ld] f32
// matrix and `plane_elems` its leading dimension ld -- and the kernel splits them itself: the LDS image of K and V, phase A, the
// softmax, phase B and the epilogue are the plane kernel's, only the producers of the image (and of the Q fragments) differ.
//   * a staging task of a lane is 8 consecutive d of one key row: two 16-byte loads, ap3_split8 (the in-projection's plane
//     epilogue sequence: the bits are the ones that epilogue would have written), three 16-byte LDS writes; a wave-iteration
//     covers 8 key rows x 64 d (lanes 0..31: panel 0, lanes 32..63: panel 1 -- every 16 lanes write 256 contiguous bytes), 26
//     wave-iterations per operand; rows behind the sequence are duplicates of row L - 1, K's swizzle is applied on the LDS side;
//   * K(next item) by the stager during phase B: two batches of 13 iterations, the batch's 26 loads in flight at once;
//   * V(item) dealt over all eight waves as in AP3_STAGE_SHARED: loads issued right behind B1, split and written behind the
//     phase's MFMAs, every wave waits for its own LDS writes (lgkmcnt) in front of B2;
//   * a query wave loads its Q fragments as f32 (8 x 16 B per lane) and splits them into qf[0..2][ks].
// O16 (with F32IN: attn_p3_o16_kernel, acx_attention_p3f16): the epilogue writes the TWO fp16 planes of oscale * o (ACX_F16X2P, the F16
// arm's pack sequence) instead of the three bf16 planes of o; oscale, a power of two, folds into the normaliser -- exact.  Everything
// before the epilogue is the F32IN arm's six-product bf16 code.  The body is shared and inlined into the kernels below:
// attn_p3_kernel keeps its name, its arguments and its code.
// O16 with F16 (attn_p3_h16_kernel, acx_attention_p3h16): the F16 arm -- two fp16 planes per operand by LDS-DMA, three fp16 products, fp16
// pair planes out -- on planes that hold s * (q | k | v) and for an output of s_att * o: the scores come out multiplied by s^2, which
// folds into the exponent's factor (sscale = 1 / s^2), the output by s, which folds into the normaliser (oscale = s_att / s).  Powers
// of two, so both folds are exact.
template <int NPROD, int F16, int F32IN, int O16>
__device__ __forceinline__ void attn_p3_body(const u16* __restrict__ qkv3, int64_t plane_elems, int64_t rows_total,
                                             u16* __restrict__ out3, int64_t out_plane_elems, int L, int heads, int nitems,
                                             long long* __restrict__ trace, float oscale, float sscale = 1.f) {
  static_assert(O16 == 0 || (F32IN != 0 && F16 == 0 && NPROD == 6) || (F32IN == 0 && F16 != 0 && NPROD == 3),
                "scaled fp16 output planes: behind bf16 products the f32-rows arm, behind fp16 products the planes arm");
  constexpr int NPL = NPROD == 3 ? 2 : 3;               // planes of K / V / Q / the output in use
  constexpr int OF = (F16 != 0 || O16 != 0) ? 1 : 0;    // the output planes' format: fp16 pairs or bf16 triples
  constexpr int ONPL = O16 ? 2 : NPL;                   // ... and their number
  // development timeline (-DAP3_TRACE=1 builds + ACX_TRACE_PTR): workgroup 0's waves stamp s_memrealtime (100 MHz) at the phase
  // boundaries of their first AP3_TRACE_ITEMS items: trace[(item_ordinal * 8 + wave) * 8 + point]
#if AP3_TRACE
#ifndef AP3_TRACE_FIRST
#define AP3_TRACE_FIRST 0
#endif
#define AP3_STAMP(ord, pt) do { if (trace && blockIdx.x == 0 && (ord) >= AP3_TRACE_FIRST && (ord) < AP3_TRACE_FIRST + 16 && lane == 0) trace[(((ord) - AP3_TRACE_FIRST) * 8 + wave) * 8 + (pt)] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define AP3_STAMP(ord, pt) do { (void)(ord); } while (0)
#endif
  int ord = 0;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int li = lane & 31, hh = lane >> 5;
  const int W = heads * 64;
  const int np = W / 32;                                // panels of q (k: + np, v: + 2 np)
  const unsigned lds0 = (unsigned)(uintptr_t)(ap3_lds_void*)smem;
  // one LDS-DMA instruction: 64 lanes x 16 B from (uniform base + per-lane 32-bit offset) to LDS [m0 .. + 1 KB)
#define AP3_GLDS(base, voff, ldsaddr)                                                              \
  do {                                                                                             \
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2" : : "v"(voff), "s"(ldsaddr), "s"(base) : "memory"); \
  } while (0)
  // the stager (wave 7: the seven query tiles belong to waves 0..6): the 6 blocks (plane p, panel c) of K (which = 1) or V
  // (which = 2) of item `it` -> LDS blocks `blk0 + 2 p + c`.  Rolled loops: this code shares the kernel's register budget.
#define AP3_STAGE(it, which, blk0, SWZ)                                                            \
  do {                                                                                             \
    const int b_ = (it) / heads, h_ = (it) - b_ * heads;                                           \
    const unsigned vc_ = (unsigned)(((SWZ) ? ((lane & 3) ^ ((lane >> 4) & 3)) : (lane & 3)) * 16); \
    _Pragma("unroll 1") for (int pc = 0; pc < 2 * NPL; ++pc) {                                     \
      const u16* src_ = qkv3 + (int64_t)(pc >> 1) * plane_elems + ((int64_t)((which) * np + 2 * h_ + (pc & 1)) * rows_total + (int64_t)b_ * L) * 32; \
      _Pragma("unroll 1") for (int j = 0; j < 13; ++j) {                                           \
        const unsigned r_ = min(16u * (unsigned)j + (unsigned)(lane >> 2), (unsigned)(L - 1));   /* behind the sequence: a finite duplicate */ \
        AP3_GLDS(src_, r_ * 64u + vc_, lds0 + (unsigned)(((blk0) + pc) * AP3_BLK_B + j * 1024));   \
      }                                                                                            \
    }                                                                                              \
  } while (0)

  // the same 78 instructions dealt over all eight waves (V: phase A is short -- 168 MFMAs per wave -- and one wave needs longer
  // than that just to ISSUE 78 LDS-DMA instructions; every wave waits for its own share before the barrier that ends the phase)
#define AP3_STAGE_SHARED(it, which, blk0, SWZ)                                                     \
  do {                                                                                             \
    const int b_ = (it) / heads, h_ = (it) - b_ * heads;                                           \
    const unsigned vc_ = (unsigned)(((SWZ) ? ((lane & 3) ^ ((lane >> 4) & 3)) : (lane & 3)) * 16); \
    _Pragma("unroll 1") for (int idx = wave; idx < 26 * NPL; idx += 8) {                           \
      const int pc = idx / 13, j = idx - 13 * pc;                                                  \
      const u16* src_ = qkv3 + (int64_t)(pc >> 1) * plane_elems + ((int64_t)((which) * np + 2 * h_ + (pc & 1)) * rows_total + (int64_t)b_ * L) * 32; \
      const unsigned r_ = min(16u * (unsigned)j + (unsigned)(lane >> 2), (unsigned)(L - 1));       \
      AP3_GLDS(src_, r_ * 64u + vc_, lds0 + (unsigned)(((blk0) + pc) * AP3_BLK_B + j * 1024));     \
    }                                                                                              \
  } while (0)

  const float* qf32 = reinterpret_cast<const float*>(qkv3);   // F32IN: the f32 rows, leading dimension plane_elems

  int item = blockIdx.x;
  if (item >= nitems) return;
  const float sc0 = 0.125f * 1.44269504088896340736f;   // 1 / sqrt(64) and log2(e): p = exp2((s - max) sc)
  const float sc = (O16 != 0 && F16 != 0) ? sc0 * sscale : sc0;
  if (wave == 7) {
    // ================================================================ the stager
    if constexpr (F32IN) ap3f_stage_k(smem, qf32, plane_elems, (int64_t)(item / heads) * L, W + (item % heads) * 64, L, lane); else
    AP3_STAGE(item, 1, 0, 1);                           // K of the first item
    for (; item < nitems; item += (int)gridDim.x) {
      AP3_STAMP(ord, 0);
      if constexpr (F32IN) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // K(item) written
      else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // K(item) landed
      AP3_STAMP(ord, 1);
      __builtin_amdgcn_s_barrier();                     // B1: ... and everybody is done with V(previous item)
      AP3_STAMP(ord, 2);
      const int nxt = item + (int)gridDim.x, nxb = nxt / heads;   // the next item and its sequence (the division: in front of B2)
      if constexpr (F32IN) {
        asm volatile("" ::: "memory");
#pragma unroll 1
        for (int wi = 7; wi < 26; wi += 8) {
          const float4* p_ = ap3f_src(qf32, plane_elems, (int64_t)(item / heads) * L, 2 * W + (item % heads) * 64, L, wi, lane);
          ap3f_put<0>(smem, p_[0], p_[1], 6, wi, lane);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      } else {
      AP3_STAGE_SHARED(item, 2, 6, 0);                  // this wave's share of V(item): needed after phase A
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      AP3_STAMP(ord, 3);
      __builtin_amdgcn_s_barrier();                     // B2: V(item) landed, everybody is done with K(item)
      AP3_STAMP(ord, 4);
      if constexpr (F32IN) {
        asm volatile("" ::: "memory");
        if (nxt < nitems) ap3f_stage_k(smem, qf32, plane_elems, (int64_t)nxb * L, W + (nxt % heads) * 64, L, lane);
      } else
      if (nxt < nitems) AP3_STAGE(nxt, 1, 0, 1);        // K(next item) during this item's phase B
      AP3_STAMP(ord, 5);
      ++ord;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // no DMA may still be writing this workgroup's LDS at exit
    return;
  }
  // ================================================================== the seven query tiles
  // V^T fragment addresses (ds_read_b64_tr_b16: every 16 lanes read a [4 keys][16 d] block): lane i of the group supplies
  // key (4 hh + 8 r + (i >> 2)) of the 16-key step, d = 16 ((lane >> 4) & 1) + 4 (i & 3) of the 32-d panel
  const int i16 = lane & 15;
  // every LDS address below = one of six per-lane base registers + an immediate < 64 KB (LDS offsets beyond the 16-bit
  // immediate would each cost a hoisted address register: the blocks of the lo planes get bases of their own)
  int va = 6 * AP3_BLK_B + (4 * hh + (i16 >> 2)) * 64 + (16 * ((lane >> 4) & 1) + 4 * (i16 & 3)) * 2;     // V hi / mid planes
  int va2 = va + 4 * AP3_BLK_B;                                                                         // V lo plane
  const int swk = (li >> 2) & 3;
  int ka0 = li * 64 + ((0 + hh) ^ swk) * 16, ka1 = li * 64 + ((2 + hh) ^ swk) * 16;                     // K hi / mid planes, d step parity
  int ka0l = ka0 + 4 * AP3_BLK_B, ka1l = ka1 + 4 * AP3_BLK_B;                                           // K lo plane
  asm volatile("" : "+v"(va), "+v"(va2), "+v"(ka0), "+v"(ka1), "+v"(ka0l), "+v"(ka1l));
  const int qrow = min(32 * wave + li, L - 1);
  for (; item < nitems; item += (int)gridDim.x) {
    const int b = item / heads, h = item - b * heads;
    // ---------------------------------------------------------------- phase A: S^T = K Q^T
    bf16x8 qf[3][4];
    if constexpr (F32IN) {                              // d = 16 ks + 8 hh .. + 7 of the query row
      const float4* qp = reinterpret_cast<const float4*>(qf32 + ((int64_t)b * L + qrow) * plane_elems + (h * 64 + 8 * hh));
      float4 qa[4], qb[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) { qa[ks] = qp[4 * ks]; qb[ks] = qp[4 * ks + 1]; }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const float qv[8] = {qa[ks].x, qa[ks].y, qa[ks].z, qa[ks].w, qb[ks].x, qb[ks].y, qb[ks].z, qb[ks].w};
        ap3_split8<0>(qv, qf[0][ks], qf[1][ks], qf[2][ks]);
      }
    } else
#pragma unroll
    for (int p = 0; p < NPL; ++p)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        qf[p][ks] = *reinterpret_cast<const bf16x8*>(qkv3 + (int64_t)p * plane_elems +
                                                     ((int64_t)(2 * h + (ks >> 1)) * rows_total + (int64_t)b * L + qrow) * 32 + ((ks & 1) * 2 + hh) * 8);
    AP3_STAMP(ord, 0);
    __builtin_amdgcn_s_barrier();                       // B1
    AP3_STAMP(ord, 1);
    float4 sva[4], svb[4];                              // F32IN: this wave's share of V(item): wave-iterations wave + 8 z < 26
    if constexpr (F32IN) {
      asm volatile("" ::: "memory");
#pragma unroll
      for (int z = 0; z < 4; ++z) {
        sva[z] = svb[z] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (z < 3 || wave < 2) {
          const float4* p_ = ap3f_src(qf32, plane_elems, (int64_t)b * L, 2 * W + h * 64, L, wave + 8 * z, lane);
          sva[z] = p_[0]; svb[z] = p_[1];
        }
      }
      __builtin_amdgcn_sched_barrier(0);                // the loads fly during phase A
    } else
    AP3_STAGE_SHARED(item, 2, 6, 0);                    // this wave's share of V(item)
    AP3_STAMP(ord, 2);
    f32x16 sacc[7];
#pragma unroll
    for (int kt = 0; kt < 7; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[kt][e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int cst = (ks >> 1) * AP3_BLK_B + 32 * kt * 64;        // panel of the d step, key tile (swizzle: row bits 2..3 = li's)
        const bf16x8 kh = *reinterpret_cast<const bf16x8*>(smem + ((ks & 1) ? ka1 : ka0) + cst);
        const bf16x8 km = *reinterpret_cast<const bf16x8*>(smem + ((ks & 1) ? ka1 : ka0) + 2 * AP3_BLK_B + cst);
        // smallest cross terms first: (hi,lo) (mid,mid) (lo,hi) (hi,mid) (mid,hi) (hi,hi)
        if constexpr (NPROD == 6) {
        const bf16x8 kl = *reinterpret_cast<const bf16x8*>(smem + ((ks & 1) ? ka1l : ka0l) + cst);
        sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, qf[2][ks], sacc[kt], 0, 0, 0);
        sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(km, qf[1][ks], sacc[kt], 0, 0, 0);
        sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kl, qf[0][ks], sacc[kt], 0, 0, 0);
        }
        sacc[kt] = ap3_mfma<F16>(kh, qf[1][ks], sacc[kt]);
        sacc[kt] = ap3_mfma<F16>(km, qf[0][ks], sacc[kt]);
        sacc[kt] = ap3_mfma<F16>(kh, qf[0][ks], sacc[kt]);
      }
      __builtin_amdgcn_sched_barrier(0);                // keep the tiles' fragment loads from piling up (register budget)
    }
    AP3_STAMP(ord, 3);
    if constexpr (F32IN) {
#pragma unroll
      for (int z = 0; z < 4; ++z)
        if (z < 3 || wave < 2) ap3f_put<0>(smem, sva[z], svb[z], 6, wave + 8 * z, lane);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's share of V(item) written
    } else
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // this wave's share of V(item) landed
    __builtin_amdgcn_s_barrier();                       // B2
    AP3_STAMP(ord, 4);
    // ---------------------------------------------------------------- phase B: softmax, O^T = V^T P^T
    // (measured in round 6: the softmax moved IN FRONT of this barrier -- it needs neither K nor V, and the two waves of a SIMD leave
    // phase A 2-3 us apart, the older one winning the matrix pipe -- shortens the traced critical path by ~2 us per item and changes
    // the kernel's time by nothing: profiles/r06_attention_notes.txt)
    // lane (query li, half hh) holds the scores of keys 32 kt + (e & 3) + 8 (e >> 2) + 4 hh
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 7; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (kt == 6) {                                  // 192 < L <= 208: only the last tile is cut
          const int key = 192 + (e & 3) + 8 * (e >> 2) + 4 * hh;
          sacc[kt][e] = key < L ? sacc[kt][e] : -INFINITY;
        }
        mx = fmaxf(mx, sacc[kt][e]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mxs = mx * sc;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 7; ++kt)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        sacc[kt][e] = __builtin_amdgcn_exp2f(fmaf(sacc[kt][e], sc, -mxs));      // v_exp_f32: 2^x, exp2(-inf) = 0
        sum += sacc[kt][e];
      }
    sum += __shfl_xor(sum, 32, 64);
    AP3_STAMP(ord, 5);                                  // softmax done
    f32x16 oacc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { oacc[0][e] = 0.f; oacc[1][e] = 0.f; }
#pragma unroll
    for (int st = 0; st < 13; ++st) {                   // 16-key steps; keys >= 208 are all masked
      const int kt = st >> 1, u = st & 1;
      const float pv[8] = {sacc[kt][8 * u], sacc[kt][8 * u + 1], sacc[kt][8 * u + 2], sacc[kt][8 * u + 3],
                           sacc[kt][8 * u + 4], sacc[kt][8 * u + 5], sacc[kt][8 * u + 6], sacc[kt][8 * u + 7]};
      bf16x8 ph, pm, pl;
      ap3_split8<F16>(pv, ph, pm, pl);                  // (NPROD == 3: pl is dead code)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        bf16x8 vf[3];
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
          const char* vb = smem + (p == 2 ? va2 : va) + ((p == 2 ? 0 : 2 * p) + dt) * AP3_BLK_B + (16 * st) * 64;
          const ap3_s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ap3_lds_s16x4*)(vb));
          const ap3_s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ap3_lds_s16x4*)(vb + 8 * 64));
          typedef short s16x8_ __attribute__((ext_vector_type(8)));
          const s16x8_ v8 = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
          vf[p] = __builtin_bit_cast(bf16x8, v8);
        }
        if constexpr (NPROD == 6) {
        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[2], ph, oacc[dt], 0, 0, 0);
        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[1], pm, oacc[dt], 0, 0, 0);
        oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[0], pl, oacc[dt], 0, 0, 0);
        }
        oacc[dt] = ap3_mfma<F16>(vf[1], ph, oacc[dt]);
        oacc[dt] = ap3_mfma<F16>(vf[0], pm, oacc[dt]);
        oacc[dt] = ap3_mfma<F16>(vf[0], ph, oacc[dt]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    AP3_STAMP(ord, 6);                                  // P V done
    // normalise, split into planes, store: lane (query li, hh) holds d = 32 dt + (e & 3) + 8 (e >> 2) + 4 hh, i.e. for every
    // group g4 of four registers an 8-byte piece of its row; v_permlane32_swap pairs the pieces of the two lane halves -- half
    // 0 ends up with d = 16 gp .. + 7, half 1 with d = 16 gp + 8 .. + 15 of the row: 16-byte stores, 12 per wave and item
    const float inv = O16 ? (1.f / sum) * oscale : 1.f / sum;
    const int q = 32 * wave + li;
    const bool st_ok = q < L;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int gp = 0; gp < 2; ++gp) {
        uint2 pl_[2][3];                                  // [g4 = 2 gp + {0, 1}][plane]
#pragma unroll
        for (int z = 0; z < 2; ++z) {
          const int g4 = 2 * gp + z;
          const float ov[4] = {oacc[dt][4 * g4] * inv, oacc[dt][4 * g4 + 1] * inv, oacc[dt][4 * g4 + 2] * inv, oacc[dt][4 * g4 + 3] * inv};
          uint2 ph2, pm2, pl2;
          ph2.x = acx_pk2<OF>(ov[0], ov[1]); ph2.y = acx_pk2<OF>(ov[2], ov[3]);
          const float r0 = ov[0] - acx_unpk_lo<OF>(ph2.x), r1 = ov[1] - acx_unpk_hi<OF>(ph2.x);
          const float r2 = ov[2] - acx_unpk_lo<OF>(ph2.y), r3 = ov[3] - acx_unpk_hi<OF>(ph2.y);
          pm2.x = acx_pk2<OF>(r0, r1); pm2.y = acx_pk2<OF>(r2, r3);
          pl2.x = f2bf2(r0 - __uint_as_float(pm2.x << 16), r1 - __uint_as_float(pm2.x & 0xffff0000u));
          pl2.y = f2bf2(r2 - __uint_as_float(pm2.y << 16), r3 - __uint_as_float(pm2.y & 0xffff0000u));
          pl_[z][0] = ph2; pl_[z][1] = pm2; pl_[z][2] = pl2;
        }
#pragma unroll
        for (int p = 0; p < ONPL; ++p) {
          // swap(X = piece of g4 = 2 gp, Y = piece of g4 = 2 gp + 1): half 0 gets (own X, partner's X), half 1 (partner's Y, own Y)
          typedef unsigned ap3_u2 __attribute__((ext_vector_type(2)));
          const ap3_u2 w0 = __builtin_amdgcn_permlane32_swap(pl_[0][p].x, pl_[1][p].x, false, false);
          const ap3_u2 w1 = __builtin_amdgcn_permlane32_swap(pl_[0][p].y, pl_[1][p].y, false, false);
          // half 0: w0[0], w1[0] = own X (d 0..3), w0[1], w1[1] = partner's X (d 4..7); half 1: [0] = partner's Y (d 0..3), [1] = own Y
          const uint4 v16 = make_uint4(w0[0], w1[0], w0[1], w1[1]);
          if (st_ok) {
            u16* dst = out3 + (int64_t)p * out_plane_elems + ((int64_t)(2 * h + dt) * rows_total + (int64_t)b * L + q) * 32 + 8 * (2 * gp + hh);
            *reinterpret_cast<uint4*>(dst) = v16;
          }
        }
      }
    AP3_STAMP(ord, 7);
    ++ord;
  }
#undef AP3_STAMP
#undef AP3_STAGE_SHARED
#undef AP3_STAGE
#undef AP3_GLDS
}

template <int NPROD, int F16 = 0, int F32IN = 0>
__global__ __launch_bounds__(512, 2) void attn_p3_kernel(const u16* __restrict__ qkv3, int64_t plane_elems, int64_t rows_total,
                                                         u16* __restrict__ out3, int64_t out_plane_elems, int L, int heads, int nitems,
                                                         long long* __restrict__ trace) {
  attn_p3_body<NPROD, F16, F32IN, 0>(qkv3, plane_elems, rows_total, out3, out_plane_elems, L, heads, nitems, trace, 1.f);
}

// f32 rows in, six bf16 products, the two fp16 planes of oscale * o out (O16)
__global__ __launch_bounds__(512, 2) void attn_p3_o16_kernel(const u16* __restrict__ qkv3, int64_t plane_elems, int64_t rows_total,
                                                             u16* __restrict__ out3, int64_t out_plane_elems, int L, int heads, int nitems,
                                                             long long* __restrict__ trace, float oscale) {
  attn_p3_body<6, 0, 1, 1>(qkv3, plane_elems, rows_total, out3, out_plane_elems, L, heads, nitems, trace, oscale);
}

// two fp16 planes of s * (q | k | v) in, three fp16 products, the two fp16 planes of s_att * o out: sscale = 1 / s^2, oscale = s_att / s
__global__ __launch_bounds__(512, 2) void attn_p3_h16_kernel(const u16* __restrict__ qkv3, int64_t plane_elems, int64_t rows_total,
                                                             u16* __restrict__ out3, int64_t out_plane_elems, int L, int heads, int nitems,
                                                             long long* __restrict__ trace, float oscale, float sscale) {
  attn_p3_body<3, 1, 0, 1>(qkv3, plane_elems, rows_total, out3, out_plane_elems, L, heads, nitems, trace, oscale, sscale);
}
