// acx_attention_hd / _x3_hd / _cls_hd -- exact-f32 multi-head attention at a head dimension that is NOT 64: attn_hd_kernel<HD>
// (non-causal, 1 <= L <= 1024) and attn_cls_hd_kernel<HD> (the CLS row only), instantiated for HD = 80 (open_clip's ViT-H-14:
// width 1280, 16 heads of 80).
// (included by acx_attn.hip inside its anonymous namespace, after acx_attn_f32.h: a16_rowmax / a16_rowsum / a16_store4 are shared)
//
// attn_hd_kernel is attn16_kernel's arithmetic family: v_mfma_f32_16x16x4_f32, transposed scores S^T = K Q^T (a lane's QUERY is the
// MFMA column, so row max / sum are per-lane scalars), flash-style online softmax, K and V streamed through LDS in chunks of 32
// keys by LDS-DMA (two stages), P^T registers directly the B operand of O^T = V^T P^T, a wave owns one 16-query tile,
// 8 waves per workgroup, persistent over (query block, sequence, head) items.  What a head dimension of 80 changes:
//   * HD / 4 = 20 k-steps for the scores (five ds_read_b128 of K per key tile, four MFMAs each) and HD / 16 = 5 output tiles;
//   * the scale HD^-0.5 is not a power of two: q is multiplied by its f32 rounding (one extra rounding per q element);
//   * a K row is 320 bytes.  attn16_kernel's image -- rows of 256 bytes, 16-byte slot p of row r holding source slot p ^ (r & 15) --
//     needs a power-of-two row; with plain 320-byte rows keys 4 apart start on the same banks (320 = 256 + 64), and no row padding
//     fixes the read.  (This paragraph is REASONING from the documented lane groups and bank rule of ds_read_b128, not a counter
//     measurement: no SQ_LDS_BANK_CONFLICT run of a padded variant was made.)  A ds_read_b128 is served in four groups of 16 lanes
//     that mix two k-groups g (lanes 0-3, 12-15 with 20-27),
//     so for a row stride of s slots the lanes (key a, g) and (key b, g + 1) meet whenever s (a - b) = 1 mod 16, and every odd s
//     has such a pair inside a group.
//     The layout chosen instead uses that an LDS-DMA instruction (global_load_lds_dwordx4) writes 64 CONTIGUOUS 16-byte slots, one
//     per lane, while each lane's SOURCE address is free: the image is FRAGMENT-major.  One 16-key tile is ten 1 KB blocks,
//       K  block c (0..4):   slot 16 g + key     = K[key][16 c + 4 g .. + 3]      -- the A fragment of k-steps 4 c .. 4 c + 3 for
//                                                                                   lane 16 g + key: the wave reads the block linearly
//       V4 block 5 + j:      slot 16 r + i       = V[4 j + r][4 i .. + 3]         -- attn16_kernel's linear V image (d < 64)
//       V1 block 9:          float 64 r + 16 g + i = V[4 g + r][64 + i]           -- the fifth output tile, read with ds_read_b32
//     Every fragment read of a wave is one contiguous 1 KB (b128) or 256 B (b32) range: conflict-free in every lane grouping by
//     the same rule (again by construction, not by counter), with no swizzle and no padding.  The price is on the global side: a K block gathers 64-byte pieces of 16 rows (the rows come
//     from L2 -- every query block of a head streams the same K and V).
//   * output tile e < 4 holds d = 4 i + e (one V4 read feeds four MFMAs), tile 4 holds d = 64 + i: a lane (query, g) ends up with
//     O[query][16 g + 4 r + (0..3)] for r < 4 and O[query][64 + 4 g + (0..3)] -- five aligned 4-column groups, so a16_store4
//     writes f32 rows, row-major planes and K-panel planes alike.  A head starts at column 80 h, 16 columns into a 32-column panel
//     for odd h; a 4-column group at a multiple of 4 never crosses a panel.
// LDS: 2 stages x 2 tiles x 10 KB = 40 KB per workgroup whatever L.  Registers and occupancy: the build's resource table
// (libacx.resources.tsv; DESIGN.md section 4 quotes it).
//
// L <= 128: one item per (sequence, head).  L > 128: query blocks of at most 8 tiles (attn_hd_kernel below).
constexpr int AHD_KT = 2;                            // 16-key tiles per staged chunk
constexpr int AHD_CHUNK = 16 * AHD_KT;

template <int HD>
struct AhdGeom {
  static_assert(HD > 64 && HD < 128 && HD % 64 == 16, "one V4 image (d < 64) and one 16-column V1 image");
  static constexpr int NC4 = HD / 16;                // K blocks per tile = ds_read_b128 per lane and key tile
  static constexpr int NI = NC4 + 5;                 // DMA instructions (1 KB blocks) per tile
  static constexpr int V4_B = NC4 * 1024, V1_B = V4_B + 4096;
  static constexpr int TILE_B = NI * 1024, STAGE_B = AHD_KT * TILE_B;
  static constexpr int LDS_B = 2 * STAGE_B;
};

__device__ __forceinline__ void ahd_softmax(f32x4& S, float& M, float& LS, f32x4 (&O)[5]) {
  const float mx = a16_rowmax(fmaxf(fmaxf(S[0], S[1]), fmaxf(S[2], S[3])));
  const float mn = fmaxf(M, mx);                     // finite: every tile visited holds >= 1 valid key
  const float al = __expf(M - mn);                   // first tile: exp(-inf) = 0
  M = mn;
#pragma unroll
  for (int r = 0; r < 4; ++r) S[r] = __expf(S[r] - mn);   // exp(-inf) = 0 for masked keys
  LS = LS * al + ((S[0] + S[1]) + (S[2] + S[3]));
  if (!__all(al == 1.f)) {                           // x * 1 == x: skipping is bit-identical
#pragma unroll
    for (int e = 0; e < 5; ++e)
#pragma unroll
      for (int r = 0; r < 4; ++r) O[e][r] *= al;
  }
}

// One wave's share of a workgroup's items.  Items are (query block, sequence, head), query block major; block qb of a sequence owns
// the 16-query tiles [qb qsz + min(qb, qrem), + qsz + (qb < qrem)), wave w tile w of them.  A wave without a tile in an item (blocks
// hold 1..8 tiles) only takes part in the staging and the barriers.  The workgroup visits items blockIdx.x, + gridDim.x, ... < nitems.
// x3plane, prows: a16_store4's (row-major or K-panel bf16 planes instead of f32 rows).
template <int HD>
__device__ __forceinline__ void ahd_run(const float* __restrict__ qkv, int64_t ldqkv, float* __restrict__ out, int64_t ldo, int L, int heads,
                                        int nitems, char* smem, int64_t x3plane, int64_t prows, int nbh, int qsz, int qrem) {
  using G = AhdGeom<HD>;
  constexpr int NC4 = G::NC4, NI = G::NI;
  const float scale = 1.f / sqrtf((float)HD);        // (a constant: folded at compile time)
  const int W = heads * HD;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  constexpr int nw = 8;
  const int qi = lane & 15, g = lane >> 4;
  const int nkt = (L + 15) >> 4;
  const int nch = (nkt + AHD_KT - 1) / AHD_KT;

  // ---- DMA plan: a chunk is AHD_KT NI wave-instructions of 1 KB; wave w issues instructions w, w + 8, ...  Instruction ii fills block
  // ii % NI of tile ii / NI; the source of lane 16 g + qi is chosen per block (the header).  Rows past L re-read row L - 1 (masked).
  // The asm statement, M0 and the hand-counted completion: see a16_run.
  const unsigned lds0 = (unsigned)(uintptr_t)(a16_lds_t*)smem;
#define AHD_DMA(gptr, ldsaddr)                                                                                   \
  do {                                                                                                           \
    unsigned keep_;                                                                                              \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" \
                 : "=&s"(keep_) : "v"(gptr), "s"(ldsaddr) : "memory");                                           \
  } while (0)
#define AHD_ISSUE1(stage, ch, i_)                                                                                \
  do {                                                                                                           \
    const int ii_ = (i_);                                           /* wave-uniform */                           \
    if (ii_ < AHD_KT * NI) {                                                                                     \
      const int k_ = ii_ % NI;                                                                                   \
      const int key_ = k_ < NC4 ? qi : k_ < NC4 + 4 ? 4 * (k_ - NC4) + g : 4 * (qi >> 2) + g;                    \
      const int e_ = k_ < NC4 ? W + 16 * k_ + 4 * g : k_ < NC4 + 4 ? 2 * W + 4 * qi : 2 * W + 64 + 4 * (qi & 3);  \
      AHD_DMA(bp_ + (int64_t)min((ch) * AHD_CHUNK + 16 * (ii_ / NI) + key_, L - 1) * ldqkv + e_,                 \
              lds0 + (stage) * G::STAGE_B + ii_ * 1024);                                                         \
    }                                                                                                            \
  } while (0)
#define AHD_ISSUE(bp, stage, ch)                                                                                 \
  do { const float* bp_ = (bp);                                                                                  \
       _Pragma("unroll") for (int j_ = 0; j_ < (AHD_KT * NI + nw - 1) / nw; ++j_) AHD_ISSUE1(stage, ch, wave + j_ * nw); } while (0)
  const int ka = lane * 16;                                      // K block: slot = lane
  const int va = G::V4_B + (4 * g) * 256 + qi * 16;              // V4: row 4 g + r, slot qi
  const int v1a = G::V1_B + (16 * g + qi) * 4;                   // V1: float 64 r + 16 g + qi

  auto bh_of = [&](int it) { return it % nbh; };
  int item = (int)blockIdx.x;
  if (item < nitems) AHD_ISSUE(qkv + (int64_t)(bh_of(item) / heads) * L * ldqkv + (bh_of(item) % heads) * HD, 0, 0);
  for (; item < nitems; item += gridDim.x) {
    const int b = bh_of(item) / heads, h = bh_of(item) % heads;
    const int qblk = item / nbh;
    const int q0 = 16 * (qblk * qsz + min(qblk, qrem)) + 16 * wave;      // this wave's tile
    const bool active = wave < qsz + (qblk < qrem ? 1 : 0);              // wave-uniform
    const float* base = qkv + (int64_t)b * L * ldqkv + h * HD;
    // ---- Q fragments (B operand of S^T = K Q^T): lane (query qi, k-group g) holds d = 16 c + 4 g + (0..3), scaled
    float4 qa[NC4];
    if (active) {
      const float* pa = base + (int64_t)min(q0 + qi, L - 1) * ldqkv + 4 * g;
#pragma unroll
      for (int c = 0; c < NC4; ++c) {
        float4 v = *reinterpret_cast<const float4*>(pa + 16 * c);
        v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
        qa[c] = v;
      }
    }
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 oa[5] = {z4, z4, z4, z4, z4};                                  // O^T tiles: e < 4: d = 16 g + 4 reg + e; 4: d = 64 + 4 g + reg
    float ma = -INFINITY, la = 0.f;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int ch = 0; ch < nch; ++ch) {
      if (ch + 1 < nch) AHD_ISSUE(base, (ch + 1) & 1, ch + 1);
      if (active) {
        const char* sS = smem + (ch & 1) * G::STAGE_B;
#pragma unroll
        for (int j = 0; j < AHD_KT; ++j) {
          const int kbase = AHD_CHUNK * ch + 16 * j;
          if (j > 0 && AHD_KT * ch + j >= nkt) break;                   // (the chunk's last tile lies past the sequence)
          const char* sT = sS + j * G::TILE_B;
          // scores: two accumulators (even / odd K blocks), added below: the 20 MFMAs are two chains
          f32x4 sa = z4, sa1 = z4;
#pragma unroll
          for (int c = 0; c < NC4; ++c) {
            const float4 k_ = *reinterpret_cast<const float4*>(sT + c * 1024 + ka);
            f32x4& ua = (c & 1) ? sa1 : sa;
            ua = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.x, qa[c].x, ua, 0, 0, 0);
            ua = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.y, qa[c].y, ua, 0, 0, 0);
            ua = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.z, qa[c].z, ua, 0, 0, 0);
            ua = __builtin_amdgcn_mfma_f32_16x16x4f32(k_.w, qa[c].w, ua, 0, 0, 0);
          }
          sa += sa1;
          if (kbase + 16 > L) {                                          // only the last tile holds keys >= L
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const bool ok_ = kbase + 4 * g + r < L;
              sa[r] = ok_ ? sa[r] : -INFINITY;
            }
          }
          ahd_softmax(sa, ma, la, oa);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float4 v_ = *reinterpret_cast<const float4*>(sT + va + r * 256);
            const float v1_ = *reinterpret_cast<const float*>(sT + v1a + r * 256);
            oa[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.x, sa[r], oa[0], 0, 0, 0);
            oa[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.y, sa[r], oa[1], 0, 0, 0);
            oa[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.z, sa[r], oa[2], 0, 0, 0);
            oa[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(v_.w, sa[r], oa[3], 0, 0, 0);
            oa[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1_, sa[r], oa[4], 0, 0, 0);
          }
        }
      }
      // next chunk landed (this wave's DMAs) and everybody is done reading this stage
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    // every wave is past its last fragment read (barrier above): stage 0 is free for the next item's first chunk
    {
      const int nxt = item + (int)gridDim.x;
      if (nxt < nitems) AHD_ISSUE(qkv + (int64_t)(bh_of(nxt) / heads) * L * ldqkv + (bh_of(nxt) % heads) * HD, 0, 0);
    }
    // ---- normalise and store: lane (query qi, g) holds O[query][16 g + 4 r + e] (e < 4) and O[query][64 + 4 g + r]
    if (active) {
      const float inv = 1.f / a16_rowsum(la);
      const int q = q0 + qi;
      if (q < L) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          a16_store4(out, (int64_t)b * L + q, h * HD + 16 * g + 4 * r, ldo, x3plane, prows, oa[0][r] * inv, oa[1][r] * inv, oa[2][r] * inv, oa[3][r] * inv);
        a16_store4(out, (int64_t)b * L + q, h * HD + 64 + 4 * g, ldo, x3plane, prows, oa[4][0] * inv, oa[4][1] * inv, oa[4][2] * inv, oa[4][3] * inv);
      }
    }
  }   // item loop
#undef AHD_ISSUE
#undef AHD_ISSUE1
#undef AHD_DMA
}

// 8 waves, one 16-query tile each; two workgroups per CU (<= 128 VGPRs, 40 KB of LDS).  A sequence's ceil(L / 16) query tiles are
// split into nqb = ceil(tiles / 8) query blocks as evenly as possible (L = 257: 6 + 6 + 5, L = 577: 8 + 8 + 7 + 7 + 7); every block
// streams all of K and V of its head.  Two tiles per wave -- attn16_kernel's deal, which halves the blocks -- were COMPILED, never
// run: hipcc's kernel-resource-usage remark gave that variant 156 VGPRs under __launch_bounds__(512, 2) (one workgroup per CU) and
// 128 VGPRs with 132-144 bytes of scratch per lane under (512, 4); the 20 Q and 20 O registers of a second tile are the difference.
// What one tile per wave costs against attn16_kernel is measured in profiles/h14_bench.txt.
template <int HD>
__global__ __launch_bounds__(512, 4) void attn_hd_kernel(const float* __restrict__ qkv, int64_t ldqkv, float* __restrict__ out, int64_t ldo,
                                                         int L, int heads, int nitems, int nqb, int64_t x3plane, int64_t prows) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int nkt = (L + 15) >> 4;
  const int qsz = nkt / nqb, qrem = nkt - qsz * nqb;
  ahd_run<HD>(qkv, ldqkv, out, ldo, L, heads, nitems, smem, x3plane, prows, nitems / nqb, qsz, qrem);
}

// CLS-row attention (the pruned last layer): attn_cls_kernel at head dimension HD.  One wavefront per (sequence, head): lanes own
// keys for the scores (blocks of 256 keys, running max and sum), then output dims for the weighted sum of V: d = lane, and
// d = 64 + (lane & 15) (every lane sums it, lanes < HD - 64 store it).
template <int HD>
__global__ __launch_bounds__(256) void attn_cls_hd_kernel(const float* __restrict__ qkv, int64_t ldqkv, float* __restrict__ out, int64_t ldo,
                                                          int batch, int L, int heads) {
  static_assert(HD > 64 && HD <= 80 && HD % 4 == 0, "d = lane and d = 64 + (lane & 15)");
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= (int64_t)batch * heads) return;
  const int b = (int)(idx / heads), h = (int)(idx % heads);
  const int W = heads * HD;
  const float scale = 1.f / sqrtf((float)HD);
  const float* base = qkv + (int64_t)b * L * ldqkv + h * HD;
  float q[HD];
#pragma unroll
  for (int c = 0; c < HD / 4; ++c) {
    const float4 v = *reinterpret_cast<const float4*>(base + 4 * c);
    q[4 * c] = v.x * scale; q[4 * c + 1] = v.y * scale; q[4 * c + 2] = v.z * scale; q[4 * c + 3] = v.w * scale;
  }
  float mx = -INFINITY, sum = 0.f, o = 0.f, o1 = 0.f;
  const int d1 = 64 + (lane & 15);
  for (int k0 = 0; k0 < L; k0 += 256) {
    float sc[4];
    float bm = -INFINITY;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = k0 + lane + 64 * u;
      float acc = -INFINITY;
      if (j < L) {
        const float* kp = base + (int64_t)j * ldqkv + W;
        acc = 0.f;
#pragma unroll
        for (int c = 0; c < HD / 4; ++c) {
          const float4 v = *reinterpret_cast<const float4*>(kp + 4 * c);
          acc += q[4 * c] * v.x + q[4 * c + 1] * v.y + q[4 * c + 2] * v.z + q[4 * c + 3] * v.w;
        }
      }
      sc[u] = acc;
      bm = fmaxf(bm, acc);
    }
    const float mn = fmaxf(mx, wave_max(bm));
    const float al = __expf(mx - mn);
    mx = mn;
    float bs = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) { sc[u] = __expf(sc[u] - mn); bs += sc[u]; }
    sum = sum * al + wave_sum(bs);
    o *= al; o1 *= al;
    const int k1 = min(L, k0 + 256);
    for (int j = k0; j < k1; ++j) {
      const int u_ = (j - k0) >> 6;
      const float mine = u_ == 0 ? sc[0] : (u_ == 1 ? sc[1] : (u_ == 2 ? sc[2] : sc[3]));
      const float p = __shfl(mine, j & 63, 64);
      const float* vp = base + (int64_t)j * ldqkv + 2 * W;
      o += p * vp[lane];
      o1 += p * vp[d1];
    }
  }
  float* op = out + (int64_t)b * ldo + h * HD;
  op[lane] = o / sum;
  if (lane < HD - 64) op[d1] = o1 / sum;
}
