// attn_s16_kernel -- the fp16 planes attention (the F16 arm of attn_p3_kernel: two fp16 planes per operand, products hi.hi, hi.lo, lo.hi
// on v_mfma_f32_32x32x16_f16, fp16 pair planes out) as a STREAMING kernel: any sequence length up to 1024, LDS use independent of L.
//   * an item is (query block, sequence, head), larger blocks first, on a persistent grid of two workgroups per CU (the order of
//     attn16_kernel<true>); a workgroup is four waves, a wave owns one 32-query tile: the ceil(L / 32) tiles of a sequence are dealt
//     as evenly as possible over ceil(tiles / 4) blocks (L = 257: 3 + 3 + 3, L = 577: 4 + 4 + 4 + 4 + 3, L = 50: one block of 2); a wave
//     without a tile only stages;
//   * the keys arrive in chunks of AS16_C = 64: in K-panel layout a (plane, panel) block of one sequence is L contiguous rows of 64 B,
//     so a chunk is 64 x 64 contiguous bytes of each of the 4 blocks of K and of V -- 32 LDS-DMA instructions of 1 KB, eight per wave
//     (wave w: rows 16 w .. + 15 of every block; K with the source-side swizzle chunk ^ ((row >> 2) & 3) of attn_p3_kernel).  Two
//     buffers of 32 KB: chunk g + 1 (the next chunk of the item, or the first of the workgroup's next item) is issued right behind
//     the barrier that releases chunk g -- every wave waits for its own DMA (vmcnt) in front of that barrier and reads behind it; the
//     buffer being refilled was last read in front of it.  One barrier per chunk;
//   * rows behind the sequence's end are read as duplicates of its last row (finite, inside the buffer) and their scores are set to
//     -inf: p = 0 exactly, times a finite v;
//   * per chunk: S^T = K Q^T (two 32-key tiles), running max m and sum in f32 (p = exp2((s - m) sc), the accumulator and the sum
//     rescaled by exp2((m_old - m) sc) -- skipped while no lane of the wave moved its max), P split into an fp16 pair in accumulator
//     order, O^T += V^T P^T with V^T by ds_read_b64_tr_b16: phase A / phase B / the epilogue are attn_p3_kernel's F16 arm, fragment
//     for fragment.
// Planes of in_scale * (q | k | v) in, of out_scale * o out: sscale = 1 / in_scale^2 folds into the exponent's factor, oscale =
// out_scale / in_scale into the normaliser (powers of two: exact).
// (included by acx_attn.hip inside its anonymous namespace, behind acx_attn_p3.h)
constexpr int AS16_C = 64;                             // keys per chunk
constexpr int AS16_NW = 4;                             // waves = 32-query tiles per block
constexpr int AS16_BLK_B = AS16_C * 64;                // a (plane, panel) block of a chunk: 4096
constexpr int AS16_BUF_B = 8 * AS16_BLK_B;             // K: 4 blocks (2 plane + panel), V: 4 blocks = 32768
constexpr int AS16_LDS_B = 2 * AS16_BUF_B;             // 65536, whatever L

__global__ __launch_bounds__(AS16_NW * 64, 2) void attn_s16_kernel(const u16* __restrict__ qkv3, int64_t plane_elems, int64_t rows_total,
                                                                   u16* __restrict__ out3, int64_t out_plane_elems, int L, int heads,
                                                                   int nbh, int nitems, float oscale, float sscale) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int li = lane & 31, hh = lane >> 5;
  const int np = 2 * heads;                             // panels of q (k: + np, v: + 2 np)
  const unsigned lds0 = (unsigned)(uintptr_t)(ap3_lds_void*)smem;
  const int nt = (L + 31) >> 5, nqb = (nt + AS16_NW - 1) / AS16_NW, tbase = nt / nqb, trem = nt - tbase * nqb;
  const int nch = (L + AS16_C - 1) / AS16_C;
  int item = blockIdx.x;
  if (item >= nitems) return;

  // this wave's eight LDS-DMA instructions of chunk c of (sequence b_, head h_) -> buffer buf_
  const unsigned vck = (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 16), vcv = (unsigned)((lane & 3) * 16);
#define AS16_STAGE(b_, h_, c_, buf_)                                                               \
  do {                                                                                             \
    const unsigned r_ = (unsigned)min((c_) * AS16_C + 16 * wave + (lane >> 2), L - 1);             \
    _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) {                                             \
      const u16* src_ = qkv3 + (int64_t)((j_ >> 1) & 1) * plane_elems +                            \
                        ((int64_t)(((j_ >> 2) + 1) * np + 2 * (h_) + (j_ & 1)) * rows_total + (int64_t)(b_) * L) * 32; \
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2"                 \
                   : : "v"(r_ * 64u + (j_ < 4 ? vck : vcv)), "s"(lds0 + (unsigned)((buf_) * AS16_BUF_B + j_ * AS16_BLK_B + wave * 1024)), "s"(src_) \
                   : "memory");                                                                    \
    }                                                                                              \
  } while (0)

  // fragment addresses inside a buffer (attn_p3_kernel's): K rows by ds_read_b128, V^T by ds_read_b64_tr_b16
  const int i16 = lane & 15;
  const int va = 4 * AS16_BLK_B + (4 * hh + (i16 >> 2)) * 64 + (16 * ((lane >> 4) & 1) + 4 * (i16 & 3)) * 2;
  const int swk = (li >> 2) & 3;
  const int ka0 = li * 64 + ((0 + hh) ^ swk) * 16, ka1 = li * 64 + ((2 + hh) ^ swk) * 16;
  const float sc = 0.125f * 1.44269504088896340736f * sscale;   // 1 / sqrt(64), log2(e), 1 / in_scale^2: p = exp2((s - max) sc)

  int qb = item / nbh, bh = item - qb * nbh, b = bh / heads, h = bh - b * heads;
  int g = 0;                                            // chunks this workgroup has consumed: buffer g & 1 holds the current one
  AS16_STAGE(b, h, 0, 0);
  for (; item < nitems; item += (int)gridDim.x) {
    const int ntile = tbase + (qb < trem ? 1 : 0), tile = qb * tbase + min(qb, trem) + wave;
    const bool active = wave < ntile;
    const int q = 32 * tile + li, qrow = min(q, L - 1);
    // the next item of this workgroup
    const int nxt = item + (int)gridDim.x;
    const int nqb_ = nxt / nbh, nbh_ = nxt - nqb_ * nbh, nb_ = nbh_ / heads, nh_ = nbh_ - nb_ * heads;
    bf16x8 qf[2][4];
    if (active) {
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          qf[p][ks] = *reinterpret_cast<const bf16x8*>(qkv3 + (int64_t)p * plane_elems +
                                                       ((int64_t)(2 * h + (ks >> 1)) * rows_total + (int64_t)b * L + qrow) * 32 + ((ks & 1) * 2 + hh) * 8);
    }
    float mx = -INFINITY, sum = 0.f;
    f32x16 oacc[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) { oacc[0][e] = 0.f; oacc[1][e] = 0.f; }
#pragma unroll 1
    for (int c = 0; c < nch; ++c, ++g) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of chunk g landed
      __builtin_amdgcn_s_barrier();                     // ... everybody's; and everybody is done with chunk g - 1
      asm volatile("" ::: "memory");
      if (c + 1 < nch) AS16_STAGE(b, h, c + 1, (g + 1) & 1);
      else if (nxt < nitems) AS16_STAGE(nb_, nh_, 0, (g + 1) & 1);
      if (!active) continue;
      const char* kb = smem + (g & 1) * AS16_BUF_B;
      // -------------------------------------------------------------- phase A: S^T = K Q^T, 2 key tiles
      f32x16 sacc[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
        for (int e = 0; e < 16; ++e) sacc[kt][e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int cst = (ks >> 1) * AS16_BLK_B + 32 * kt * 64;       // panel of the d step, key tile
          const bf16x8 kh = *reinterpret_cast<const bf16x8*>(kb + ((ks & 1) ? ka1 : ka0) + cst);
          const bf16x8 kl = *reinterpret_cast<const bf16x8*>(kb + ((ks & 1) ? ka1 : ka0) + 2 * AS16_BLK_B + cst);
          sacc[kt] = ap3_mfma<1>(kh, qf[1][ks], sacc[kt]);
          sacc[kt] = ap3_mfma<1>(kl, qf[0][ks], sacc[kt]);
          sacc[kt] = ap3_mfma<1>(kh, qf[0][ks], sacc[kt]);
        }
      }
      // lane (query li, half hh) holds the scores of keys 64 c + 32 kt + (e & 3) + 8 (e >> 2) + 4 hh
      if ((c + 1) * AS16_C > L) {                       // the sequence ends inside this chunk
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int key = c * AS16_C + 32 * kt + (e & 3) + 8 * (e >> 2) + 4 * hh;
            sacc[kt][e] = key < L ? sacc[kt][e] : -INFINITY;
          }
      }
      float cm = sacc[0][0];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) cm = fmaxf(cm, sacc[kt][e]);
      cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
      const float mnew = fmaxf(mx, cm);                 // finite: key 64 c of every chunk is inside the sequence
      const float alpha = __builtin_amdgcn_exp2f((mx - mnew) * sc);   // first chunk: exp2(-inf) = 0 on a zero accumulator
      const float mns = mnew * sc;
      mx = mnew;
      float cs = 0.f;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          sacc[kt][e] = __builtin_amdgcn_exp2f(fmaf(sacc[kt][e], sc, -mns));   // v_exp_f32: exp2(-inf) = 0
          cs += sacc[kt][e];
        }
      sum = fmaf(sum, alpha, cs);
      if (__any(alpha != 1.f)) {
#pragma unroll
        for (int e = 0; e < 16; ++e) { oacc[0][e] *= alpha; oacc[1][e] *= alpha; }
      }
      // -------------------------------------------------------------- phase B: O^T += V^T P^T, 16-key steps
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int kt = st >> 1, u = st & 1;
        const float pv[8] = {sacc[kt][8 * u], sacc[kt][8 * u + 1], sacc[kt][8 * u + 2], sacc[kt][8 * u + 3],
                             sacc[kt][8 * u + 4], sacc[kt][8 * u + 5], sacc[kt][8 * u + 6], sacc[kt][8 * u + 7]};
        bf16x8 ph, pl, unused_;
        ap3_split8<1>(pv, ph, pl, unused_);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          bf16x8 vf[2];
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const char* vb = kb + va + (2 * p + dt) * AS16_BLK_B + (16 * st) * 64;
            const ap3_s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ap3_lds_s16x4*)(vb));
            const ap3_s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ap3_lds_s16x4*)(vb + 8 * 64));
            typedef short s16x8_ __attribute__((ext_vector_type(8)));
            const s16x8_ v8 = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
            vf[p] = __builtin_bit_cast(bf16x8, v8);
          }
          oacc[dt] = ap3_mfma<1>(vf[1], ph, oacc[dt]);
          oacc[dt] = ap3_mfma<1>(vf[0], pl, oacc[dt]);
          oacc[dt] = ap3_mfma<1>(vf[0], ph, oacc[dt]);
        }
      }
    }
    if (active) {
      // normalise, split into the fp16 pair, store (attn_p3_kernel's epilogue): lane (query li, hh) holds d = 32 dt + (e & 3) +
      // 8 (e >> 2) + 4 hh; v_permlane32_swap pairs the 8-byte pieces of the two lane halves into 16-byte stores
      sum += __shfl_xor(sum, 32, 64);
      const float inv = (1.f / sum) * oscale;
      const bool st_ok = q < L;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
          uint2 pl_[2][2];                                // [g4 = 2 gp + {0, 1}][plane]
#pragma unroll
          for (int z = 0; z < 2; ++z) {
            const int g4 = 2 * gp + z;
            const float ov[4] = {oacc[dt][4 * g4] * inv, oacc[dt][4 * g4 + 1] * inv, oacc[dt][4 * g4 + 2] * inv, oacc[dt][4 * g4 + 3] * inv};
            uint2 ph2, pm2;
            ph2.x = acx_pk2<1>(ov[0], ov[1]); ph2.y = acx_pk2<1>(ov[2], ov[3]);
            const float r0 = ov[0] - acx_unpk_lo<1>(ph2.x), r1 = ov[1] - acx_unpk_hi<1>(ph2.x);
            const float r2 = ov[2] - acx_unpk_lo<1>(ph2.y), r3 = ov[3] - acx_unpk_hi<1>(ph2.y);
            pm2.x = acx_pk2<1>(r0, r1); pm2.y = acx_pk2<1>(r2, r3);
            pl_[z][0] = ph2; pl_[z][1] = pm2;
          }
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            typedef unsigned ap3_u2 __attribute__((ext_vector_type(2)));
            const ap3_u2 w0 = __builtin_amdgcn_permlane32_swap(pl_[0][p].x, pl_[1][p].x, false, false);
            const ap3_u2 w1 = __builtin_amdgcn_permlane32_swap(pl_[0][p].y, pl_[1][p].y, false, false);
            const uint4 v16 = make_uint4(w0[0], w1[0], w0[1], w1[1]);
            if (st_ok) {
              u16* dst = out3 + (int64_t)p * out_plane_elems + ((int64_t)(2 * h + dt) * rows_total + (int64_t)b * L + q) * 32 + 8 * (2 * gp + hh);
              *reinterpret_cast<uint4*>(dst) = v16;
            }
          }
        }
    }
    qb = nqb_; b = nb_; h = nh_;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // no DMA may still be writing this workgroup's LDS at exit
#undef AS16_STAGE
}
