// acx_attention_bf16 --the same attention with bf16 operands (bf16 mode of the ViT, not a parity path):
// qkv and the output are bf16 in global memory, QK^T and PV run on v_mfma_f32_32x32x16_bf16, softmax in f32.
//   * K of the head in LDS as bf16 rows of 128 B padded to 144 B (conflict-free ds_read_b128 A fragments);
//     V as two 32-column panels of 64-byte rows (16-byte LDS writes, like K); the bf16 MFMA packs 8 contraction indices
//     (keys) per lane, so the V^T fragments come out of LDS by transpose reads (ds_read_b64_tr_b16: every 16 lanes read a
//     [4 keys][16 d] block) -- round 4 transposed while staging with 2-byte LDS writes: eight ds_write_b16 per 16 bytes and
//     the kernel's only LDS bank conflicts (6.8 M cycles per launch).
//     K + V = 61 KB -> two workgroups per CU (the f32 kernel needs 112 KB and runs one).
//   * S^T = K Q^T exactly as in the f32 kernel (lane = query column, registers = keys), so softmax is
//     in-register + one cross-half exchange, and register group 8c..8c+7 of a key tile, packed to bf16, IS the
//     B operand of O^T = V^T P^T for key chunk c.  The keys a lane half holds there are
//     {16c + 4h + (0..3)} u {16c + 8 + 4h + (0..3)}: the V^T fragment is two transpose reads, eight rows apart.
//   * O^T's C layout has lane = query again: 1/rowsum is a per-lane scalar and a lane stores 4 x 8 bytes per
//     32-wide slice of its row.
// (included by acx_attn.hip inside its anonymous namespace)
constexpr int BK_ROWB = 144;      // bytes per K row in LDS
constexpr int BV_PANEL_B = 224 * 64 + 64;   // one 32-column panel of V: 224 rows of 64 B (+ 64: the two panels' rows on different banks)
typedef short ab_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) ab_s16x4 ab_lds_s16x4;

__device__ __forceinline__ uint32_t pack2_bf16(float a, float b) { return f2bf2(a, b); }
typedef float f32x2v __attribute__((ext_vector_type(2)));

template <int NT>
__global__ __launch_bounds__(256, 2) void attn_bf16_kernel(const u16* __restrict__ qkv, int64_t ldqkv, u16* __restrict__ out,
                                                          int64_t ldo, int L, int heads) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;                                  // [NT*32][144 B]
  char* sV = smem + NT * 32 * BK_ROWB;              // [2 panels][224 rows][64 B]
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int W = heads * 64;
  const u16* base = qkv + (int64_t)b * L * ldqkv + h * 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int li = lane & 31, hh = lane >> 5;

  // ---- stage K (row copy) and V (transposed); 8 lanes cover one 128-byte row; rows >= L are zero
  constexpr int NP = NT * 32 * 8;                   // 16-byte pieces per operand
  constexpr int NSTG = (NP + 255) / 256;
  uint4 stk[NSTG], stv[NSTG];
#pragma unroll
  for (int j = 0; j < NSTG; ++j) {
    const int i = t + j * 256;
    const int row = i >> 3, pc = i & 7;
    stk[j] = make_uint4(0, 0, 0, 0);
    stv[j] = stk[j];
    if (i < NP && row < L) {
      const u16* p = base + (int64_t)row * ldqkv + 8 * pc;
      stk[j] = *reinterpret_cast<const uint4*>(p + W);
      stv[j] = *reinterpret_cast<const uint4*>(p + 2 * W);
    }
  }
  // ---- Q fragments (B operand) of this wave's (at most two: NT <= 8) query blocks, requested BEHIND the K / V loads so that the
  // whole workgroup waits for memory once: query row qb*32 + li, d = 8*(2kk + hh) .. +7.  (Loaded at the head of each query
  // block they cost a second and a third exposed round trip per workgroup: 16.7 us of lifetime for ~3.5 us of arithmetic.)
  uint4 qpre[2][4];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int q = min((wave + 4 * it) * 32 + li, L - 1);
    const u16* qp = base + (int64_t)q * ldqkv + 8 * hh;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qpre[it][kk] = *reinterpret_cast<const uint4*>(qp + 16 * kk);
  }
#pragma unroll
  for (int j = 0; j < NSTG; ++j) {
    const int i = t + j * 256;
    const int row = i >> 3, pc = i & 7;
    if (i < NP) {
      *reinterpret_cast<uint4*>(sK + row * BK_ROWB + pc * 16) = stk[j];
      *reinterpret_cast<uint4*>(sV + (pc >> 2) * BV_PANEL_B + row * 64 + (pc & 3) * 16) = stv[j];
    }
  }
  __syncthreads();

  const int nqb = (L + 31) / 32;
  const int vtr = (4 * hh + ((lane & 15) >> 2)) * 64 + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;   // transpose-read offset inside a 16-key step
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int qb = wave + 4 * it;
    if (qb >= nqb) break;
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = *reinterpret_cast<const bf16x8*>(&qpre[it][kk]);
    // ---- S^T tiles: keys x queries
    f32x16 st[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) st[kt][e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(sK + (kt * 32 + li) * BK_ROWB + (2 * kk + hh) * 16);
        st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], st[kt], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);     // one key tile of fragments in flight, not all 28 (register spills)
    }
    // ---- softmax over the keys of this lane's query: register r of tile kt is key kt*32 + (r&3) + 8(r>>2) + 4hh.
    // At the bf16 MFMA rate this VALU work weighs more than the MFMAs (SQ_ACTIVE_INST_VALU 35 % vs MFMA busy 18 %): the
    // maximum is taken over the RAW scores (the scale is positive), only the last key tile holds keys >= L, and scale,
    // shift and the base change are ONE (packed) fma in front of v_exp_f32: p = 2^((s - m) * 0.125 * log2 e).
    {
      constexpr int kt = NT - 1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
        st[kt][r] = key < L ? st[kt][r] : -3.0e38f;
      }
    }
    float m = -3.0e38f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int r = 0; r < 16; r += 2) m = fmaxf(m, fmaxf(st[kt][r], st[kt][r + 1]));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float sc_ = 0.125f * 1.4426950408889634f, nmc = -m * sc_;
    f32x2v sum2 = {0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int r = 0; r < 16; r += 2) {
        const f32x2v s2 = {st[kt][r], st[kt][r + 1]};
        const f32x2v a2 = __builtin_elementwise_fma(s2, (f32x2v){sc_, sc_}, (f32x2v){nmc, nmc});
        const f32x2v p2 = {__builtin_amdgcn_exp2f(a2[0]), __builtin_amdgcn_exp2f(a2[1])};
        st[kt][r] = p2[0]; st[kt][r + 1] = p2[1];
        sum2 += p2;
      }
    float sum = sum2[0] + sum2[1];
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
    // ---- O^T = V^T P^T : two 32-wide e tiles
    f32x16 o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        uint4 pk;
        pk.x = pack2_bf16(st[kt][8 * c + 0], st[kt][8 * c + 1]);
        pk.y = pack2_bf16(st[kt][8 * c + 2], st[kt][8 * c + 3]);
        pk.z = pack2_bf16(st[kt][8 * c + 4], st[kt][8 * c + 5]);
        pk.w = pack2_bf16(st[kt][8 * c + 6], st[kt][8 * c + 7]);
        const bf16x8 pf = *reinterpret_cast<const bf16x8*>(&pk);
        // lane i of a 16-lane group supplies key 4 hh + (i >> 2) (+ 8: second read) of the 16-key step, d = 16 ((lane >> 4) & 1) + 4 (i & 3)
        const char* v0 = sV + vtr + (kt * 32 + 16 * c) * 64;
        typedef short s16x8_ __attribute__((ext_vector_type(8)));
        bf16x8 vf[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const ab_s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ab_lds_s16x4*)(v0 + dt * BV_PANEL_B));
          const ab_s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ab_lds_s16x4*)(v0 + dt * BV_PANEL_B + 8 * 64));
          const s16x8_ v8 = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
          vf[dt] = __builtin_bit_cast(bf16x8, v8);
        }
        o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[0], pf, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[1], pf, o1, 0, 0, 0);
      }
    // ---- store: lane = query, register r of tile et is column e = et*32 + (r&3) + 8(r>>2) + 4hh
    const int qrow = qb * 32 + li;
    if (qrow < L) {
      u16* op = out + ((int64_t)b * L + qrow) * ldo + h * 64 + 4 * hh;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        uint2 w0, w1;
        w0.x = pack2_bf16(o0[4 * g4] * inv, o0[4 * g4 + 1] * inv); w0.y = pack2_bf16(o0[4 * g4 + 2] * inv, o0[4 * g4 + 3] * inv);
        w1.x = pack2_bf16(o1[4 * g4] * inv, o1[4 * g4 + 1] * inv); w1.y = pack2_bf16(o1[4 * g4 + 2] * inv, o1[4 * g4 + 3] * inv);
        *reinterpret_cast<uint2*>(op + 8 * g4) = w0;
        *reinterpret_cast<uint2*>(op + 32 + 8 * g4) = w1;
      }
    }
  }
}
