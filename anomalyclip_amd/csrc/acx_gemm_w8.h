// acx_gemm -- 8-wave f32 kernel (FAST problems and the implicit-GEMM 3x3 convolutions)
// (included by acx_gemm.hip inside its anonymous namespace; shares Args / tile constants / helpers defined there)
// =====================================================================================================
// f32 GEMM, 8 waves per 128x128 tile (FAST problems only: identity rows, K % 32 == 0, f32 in / out)
//
// Same LDS image, K-permutation and K-step schedule as gemm_kernel, but the tile is shared by 8 waves of 64 x 32
// instead of 4 waves of 64 x 64: two co-resident blocks then put FOUR waves on every SIMD (<= 128 VGPRs each), so
// a wave that sits at the K-step barrier or on an LDS round trip leaves three others to feed the matrix pipe
// instead of one.  Costs 1.5x the LDS fragment reads per flop (still < 10 % of the LDS port).
// CONV = 1: the implicit-GEMM 3x3 convolution of the axial feed-forwards (A rows are token rows shifted by the tap of
// the current K-step, zero outside the (gn, gl) grid; cin % 32 == 0 so a K-step never straddles two taps).
#ifndef ACX_SUPERTILE
#define ACX_SUPERTILE 1      /* measured: fabric reads -43 % (qkv) / -55 % (fc) / -11 % (N = 768), L2 hit 0.65 -> 0.77, time +-1 % */
#endif
// Super-tile order for full rectangular grids (nwg = tiles_m x tiles_n one-tile blocks, block b on XCD b % 8):
// XCD x owns a band of whole tile ROWS; inside the band the blocks walk column groups of width sn (<= 8, groups of equal
// width up to rounding), row-major inside a group -- the ~64 tiles an XCD has in flight then form an ~(64/sn) x sn
// rectangle, so every A / W K-slice is wanted by sn / (64/sn) tiles at about the same time and the XCD's L2 serves all but
// the first.  Bands hold nr_x * tiles_n tiles, XCDs run qq (+1) blocks: the few surplus blocks of some XCDs take the tail
// tiles of the bands that are longer than their XCD's block count (bijective by construction).
__device__ __forceinline__ void w8_band_tile(int r0, int nr, int tiles_n, int idx, int& tm, int& tn) {
  const int ncg = (tiles_n + 7) >> 3, sn = (tiles_n + ncg - 1) / ncg;
  const int full = nr * sn;                                  // tiles per full-width column group
  int cg = idx / full;
  if (cg >= ncg) cg = ncg - 1;
  const int c0 = cg * sn, cw = min(sn, tiles_n - c0);
  const int jg = idx - c0 * nr;
  tm = r0 + jg / cw;
  tn = c0 + jg % cw;
}
__device__ __forceinline__ bool w8_supertile_map(int bid, int nwg, int tiles_n, int& tm, int& tn) {
  const int tiles_m = nwg / tiles_n;
  if (tiles_m * tiles_n != nwg || tiles_m < 8) return false;
  const int x = bid & 7, jl = bid >> 3;
  const int qq = nwg >> 3, rr = nwg & 7, qm = tiles_m >> 3, rm = tiles_m & 7;
  int r0 = 0, my_r0 = 0, my_nr = 0, my_T = 0, before = 0;
  // pass 1: this XCD's band, and how many surplus blocks the XCDs before it have
  for (int y = 0; y < 8; ++y) {
    const int nr = qm + (y < rm ? 1 : 0), T = nr * tiles_n, nb = qq + (y < rr ? 1 : 0);
    if (y == x) { my_r0 = r0; my_nr = nr; my_T = T; }
    if (y < x) before += max(0, nb - T);
    r0 += nr;
  }
  if (jl < my_T) { w8_band_tile(my_r0, my_nr, tiles_n, jl, tm, tn); return true; }
  // surplus block: take the E-th leftover tile (tiles of bands longer than their XCD's block count, in XCD order)
  int E = before + (jl - my_T);
  r0 = 0;
  for (int y = 0; y < 8; ++y) {
    const int nr = qm + (y < rm ? 1 : 0), T = nr * tiles_n, nb = qq + (y < rr ? 1 : 0);
    const int left = max(0, T - nb);
    if (E < left) { w8_band_tile(r0, nr, tiles_n, nb + E, tm, tn); return true; }
    E -= left;
    r0 += nr;
  }
  return false;
}

#ifndef ACX_W8_VEC_EPILOGUE
#define ACX_W8_VEC_EPILOGUE 1
#endif
template <int ACT, int RES, int CONV>
__global__ __launch_bounds__(512, 2) void gemm_f32_w8_kernel(const Args g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const acx_gemm_desc& d = g.d;
  const int nwg = gridDim.x;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
  const int jl = bid >> 3;
#if ACX_SUPERTILE
  int tm, tn;
  if (!w8_supertile_map(bid, nwg, g.tiles_n, tm, tn)) {
    const int wg_ = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + jl;
    tm = wg_ / g.tiles_n; tn = wg_ % g.tiles_n;
  }
#else
  const int wg = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + jl;
  const int tm = wg / g.tiles_n, tn = wg % g.tiles_n;
#endif
  const int m0 = tm * BM, n0 = tn * BN;

  const int t = threadIdx.x;
  const int chunk = t & 7, rbase = t >> 3;                  // 64 staged rows per pass, 2 passes per operand
  const float* pa0 = (const float*)d.A + (size_t)min(m0 + rbase, d.M - 1) * d.lda + chunk * 4;
  const float* pa1 = (const float*)d.A + (size_t)min(m0 + rbase + 64, d.M - 1) * d.lda + chunk * 4;
  const float* pw0 = (const float*)d.W + (size_t)min(n0 + rbase, d.N - 1) * d.ldw + chunk * 4;
  const float* pw1 = (const float*)d.W + (size_t)min(n0 + rbase + 64, d.N - 1) * d.ldw + chunk * 4;
  float4 ra0, ra1, rw0, rw1;
  // conv: grid coordinates of the two staged token rows, base row of their tile, validity of the staged taps
  int cn0 = 0, cl0 = 0, cn1 = 0, cl1 = 0;
  long cb0 = 0, cb1 = 0;
  bool ok0 = true, ok1 = true;
  if constexpr (CONV != 0) {
    const int gsz = d.gn * d.gl;
    const int r0_ = min(m0 + rbase, d.M - 1), r1_ = min(m0 + rbase + 64, d.M - 1);
    const int t0_ = r0_ / gsz, t1_ = r1_ / gsz;
    cb0 = (long)t0_ * gsz; cb1 = (long)t1_ * gsz;
    cn0 = (r0_ - t0_ * gsz) / d.gl; cl0 = (r0_ - t0_ * gsz) - cn0 * d.gl;
    cn1 = (r1_ - t1_ * gsz) / d.gl; cl1 = (r1_ - t1_ * gsz) - cn1 * d.gl;
  }
  // conv: the tap of a K-step (k0 / cin) changes every cin / 32 steps -- the shifted source rows, their validity and the
  // pointers are recomputed only then; in between a load is pointer + running offset (K-steps arrive in order)
  const float *cs0 = nullptr, *cs1 = nullptr;
  int ctap = 0, ckin = 0;
#define W8_TAP()                                                                                   \
  do {                                                                                             \
    const int dn_ = ctap / 3 - 1, dl_ = ctap - (ctap / 3) * 3 - 1;                                 \
    const int n0_ = cn0 + dn_, l0_ = cl0 + dl_, n1_ = cn1 + dn_, l1_ = cl1 + dl_;                   \
    ok0 = (unsigned)n0_ < (unsigned)d.gn && (unsigned)l0_ < (unsigned)d.gl;                        \
    ok1 = (unsigned)n1_ < (unsigned)d.gn && (unsigned)l1_ < (unsigned)d.gl;                        \
    const long s0_ = cb0 + (long)min(max(n0_, 0), d.gn - 1) * d.gl + min(max(l0_, 0), d.gl - 1);   \
    const long s1_ = cb1 + (long)min(max(n1_, 0), d.gn - 1) * d.gl + min(max(l1_, 0), d.gl - 1);   \
    cs0 = (const float*)d.A + (size_t)s0_ * d.lda + chunk * 4;                                     \
    cs1 = (const float*)d.A + (size_t)s1_ * d.lda + chunk * 4;                                     \
  } while (0)
#define W8_LOAD(k0)                                                                                \
  do {                                                                                             \
    if constexpr (CONV != 0) {                                                                     \
      if (ckin == d.cin) { ckin = 0; ++ctap; W8_TAP(); }          /* uniform */                    \
      ra0 = ld4(cs0 + ckin);                                                                       \
      ra1 = ld4(cs1 + ckin);                                                                       \
      ckin += 32;                                                                                  \
    } else {                                                                                       \
      ra0 = ld4(pa0 + (k0)); ra1 = ld4(pa1 + (k0));                                                \
    }                                                                                              \
    rw0 = ld4(pw0 + (k0)); rw1 = ld4(pw1 + (k0));                                                  \
  } while (0)
#define W8_STORE(stage, r)                                                             \
  do {                                                                                 \
    char* sA_ = smem + (stage) * 2 * TILE_B;                                           \
    const int off_ = (rbase + 64 * (r)) * ROWB + chunk * 16;                           \
    float4 va_ = ra##r;                                                                \
    if constexpr (CONV != 0) { if (!ok##r) va_ = make_float4(0.f, 0.f, 0.f, 0.f); }    \
    *reinterpret_cast<float4*>(sA_ + off_) = va_;                                      \
    *reinterpret_cast<float4*>(sA_ + TILE_B + off_) = rw##r;                           \
  } while (0)

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  const int lane = t & 63, wave = t >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int li = lane & 31, hh = lane >> 5;
  const int a_off = (wm * 64 + li) * ROWB + hh * 16;
  const int w_off = (wn * 32 + li) * ROWB + hh * 16;
  float4 xa0, xa1, xb, ya0, ya1, yb;
#define W8_RD(SET, stage, q)                                                                              \
  do {                                                                                                    \
    const char* sA_ = smem + (stage) * 2 * TILE_B;                                                        \
    SET##a0 = *reinterpret_cast<const float4*>(sA_ + a_off + (q) * 32);                                   \
    SET##a1 = *reinterpret_cast<const float4*>(sA_ + a_off + 32 * ROWB + (q) * 32);                       \
    SET##b = *reinterpret_cast<const float4*>(sA_ + TILE_B + w_off + (q) * 32);                           \
  } while (0)
#define W8_MM(SET)                                                                                        \
  do {                                                                                                    \
    const float a0_[4] = {SET##a0.x, SET##a0.y, SET##a0.z, SET##a0.w};                                    \
    const float a1_[4] = {SET##a1.x, SET##a1.y, SET##a1.z, SET##a1.w};                                    \
    const float b_[4] = {SET##b.x, SET##b.y, SET##b.z, SET##b.w};                                         \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                       \
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0_[j], b_[j], acc[0], 0, 0, 0);                      \
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1_[j], b_[j], acc[1], 0, 0, 0);                      \
    }                                                                                                     \
  } while (0)

  // split-K (skinny problems): gridDim.y splits of kchunk K-steps; raw partial tiles, epilogue in splitk_reduce_kernel
  const int nk_total = d.K / 32;
  const int kbeg = (g.ksplit > 1 ? (int)blockIdx.y * g.kchunk : 0) * 32;
  const int nk = g.ksplit > 1 ? min(g.kchunk, nk_total - (int)blockIdx.y * g.kchunk) : nk_total;
  if constexpr (CONV != 0) {
    ctap = kbeg / d.cin;
    ckin = kbeg - ctap * d.cin;
    W8_TAP();
  }
  W8_LOAD(kbeg);
  W8_STORE(0, 0); W8_STORE(0, 1);
  __syncthreads();
  if (nk > 1) W8_LOAD(kbeg + 32);
  W8_RD(x, 0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1, nxt = cur ^ 1;
    const bool more = kt + 1 < nk;
    W8_RD(y, cur, 1);
    W8_MM(x);                                    // phase 0
    W8_RD(x, cur, 2);
    if (more) W8_STORE(nxt, 0);
    W8_MM(y);                                    // phase 1
    W8_RD(y, cur, 3);
    if (more) W8_STORE(nxt, 1);
    W8_MM(x);                                    // phase 2
    __syncthreads();                             // next tile complete in LDS; everyone holds its phase-3 fragments
    if (kt + 2 < nk) W8_LOAD(kbeg + (kt + 2) * 32);
    if (more) W8_RD(x, nxt, 0);
    W8_MM(y);                                    // phase 3
  }
#undef W8_MM
#undef W8_RD
#undef W8_STORE
#undef W8_LOAD
#undef W8_TAP

  const int col = n0 + wn * 32 + li;
  const bool cok = col < d.N;
  // (only the convolutions are ever split: keeping the branch out of the plain instantiations keeps the ViT's residual GEMMs at
  // their round-3 register allocation -- with it compiled in, out-proj / proj lost 4-6 %)
  if (CONV != 0 && g.ksplit > 1) {
    float* P = g.partial + (size_t)blockIdx.y * d.M * d.N;
    if (!g.counters) {                 // partial tiles for splitk_reduce_kernel (second launch)
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm * 64 + mi * 32 + 4 * hh + (r & 3) + 8 * (r >> 2);
          if (cok && row < d.M) P[(size_t)row * d.N + col] = acc[mi][r];
        }
      return;
    }
    // In-kernel reduction, no second launch: the K pieces publish their raw tiles with agent-scope (write-through) stores --
    // no release fence, which would write back the XCD's whole L2 --, bump the tile's relaxed arrival counter, and the LAST
    // piece to arrive adds the pieces in piece order and falls through into the normal epilogue.  The counter returns to zero.
    __shared__ bool last_piece;
    // lane-constant 32-bit element offset of (row 0 of the lane's tile rows, its column); the 32 tile rows of a lane are
    // wave-uniform multiples of N further on: one address register for all of them
    const int rbase = m0 + wm * 64 + 4 * hh;
    const unsigned loff = (unsigned)rbase * (unsigned)d.N + (unsigned)col;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ro = mi * 32 + (r & 3) + 8 * (r >> 2);
        float* rowp = P + (size_t)ro * d.N;                                // wave-uniform
        if (cok && rbase + ro < d.M) __hip_atomic_store(rowp + loff, acc[mi][r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      ACX_HANDOFF_RELEASE();
      last_piece = __hip_atomic_fetch_add(g.counters + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)g.ksplit - 1;
    }
    __syncthreads();
    if (!last_piece) return;
    ACX_HANDOFF_ACQUIRE();
    // every piece -- this block's own included: it was published like the others -- is read back in piece order ((0 + p0) + p1
    // + ..., the reduce kernel's order, bit for bit)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;
#pragma unroll 1
    for (int q = 0; q < g.ksplit; ++q) {
      const float* Pq = g.partial + (size_t)q * d.M * d.N;
      float pv[2][16];                                                     // a whole piece in flight: one memory latency per piece
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ro = mi * 32 + (r & 3) + 8 * (r >> 2);
          const float* rowp = Pq + (size_t)ro * d.N;                       // wave-uniform
          pv[mi][r] = (cok && rbase + ro < d.M) ? __hip_atomic_load(rowp + loff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
        }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mi][r] += pv[mi][r];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (threadIdx.x == 0) __hip_atomic_store(g.counters + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // ---- vector epilogue.  In the 32x32 C layout a lane holds ONE column and 16 rows, so the natural store is 32 x
  // global_store_dword per lane (64 instructions of 2 x 128 B per wave and tile, plus as many residual loads): the store
  // tail is instruction-issue bound and costs ~1.3 K-steps per tile.  Each wave instead transposes its two 32x32
  // accumulator tiles through a private 4.5 KB slice of the (now idle) staging LDS and goes to memory with 16-byte
  // accesses: 8 rows x 128 B per instruction, 4 stores + 4 residual loads per accumulator tile.
  // (every LDS read of the K loop completed before its last barrier; the slices are wave-private)
  if (ACX_W8_VEC_EPILOGUE && d.N % 4 == 0 && d.ldc % 4 == 0 && !((uintptr_t)d.C & 15) && !((uintptr_t)d.bias & 15) &&
      (RES == 0 || (d.ldr % 4 == 0 && !((uintptr_t)d.residual & 15)))) {
    float* sT = reinterpret_cast<float*>(smem) + wave * (32 * 36);
    const int tr = lane >> 3, tc = 4 * (lane & 7);
    const int gcol = n0 + wn * 32 + tc;
    const bool gok = gcol < d.N;
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d.bias && gok) b4 = ld4(d.bias + gcol);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sT[(4 * hh + (r & 3) + 8 * (r >> 2)) * 36 + li] = acc[mi][r];
      const int grow0 = m0 + wm * 64 + mi * 32 + tr;
      float4 rs[4], ov[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        rs[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (RES != 0) {
          const int row = min(grow0 + 8 * i, d.M - 1);
          rs[i] = ld4(d.residual + (size_t)row * d.ldr + (gok ? gcol : 0));
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 a4 = *reinterpret_cast<const float4*>(sT + (tr + 8 * i) * 36 + tc);
        float v[4] = {a4.x + b4.x, a4.y + b4.y, a4.z + b4.z, a4.w + b4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if constexpr (ACT == ACX_ACT_QUICKGELU) v[e] = acx_quickgelu(v[e]);
          if constexpr (ACT == ACX_ACT_GELU) v[e] = acx_gelu(v[e]);
          if constexpr (ACT == ACX_ACT_LEAKYRELU) v[e] = v[e] > 0.f ? v[e] : 0.01f * v[e];
          if constexpr (ACT == ACX_ACT_RELU) v[e] = fmaxf(v[e], 0.f);
        }
        ov[i] = make_float4(rs[i].x + v[0], rs[i].y + v[1], rs[i].z + v[2], rs[i].w + v[3]);
        if constexpr (ACT == ACX_ACT_RESRELU)
          ov[i] = make_float4(fmaxf(ov[i].x, 0.f), fmaxf(ov[i].y, 0.f), fmaxf(ov[i].z, 0.f), fmaxf(ov[i].w, 0.f));
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(ov[i].x), "+v"(ov[i].y), "+v"(ov[i].z), "+v"(ov[i].w));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = grow0 + 8 * i;
        if (gok && row < d.M) *reinterpret_cast<float4*>((float*)d.C + (size_t)row * d.ldc + gcol) = ov[i];
      }
    }
    return;
  }
  // ---- scalar epilogue (structure of gemm_kernel's: everything computed, then stored)
  const int colc = cok ? col : d.N - 1;
  float bias = 0.f;
  if (d.bias) bias = d.bias[colc];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int rowb = m0 + wm * 64 + mi * 32 + 4 * hh;
    float outv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) outv[r] = 0.f;
    if constexpr (RES != 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = min(rowb + (r & 3) + 8 * (r >> 2), d.M - 1);
        outv[r] = d.residual[(size_t)row * d.ldr + colc];
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = acc[mi][r] + bias;
      if constexpr (ACT == ACX_ACT_QUICKGELU) v = acx_quickgelu(v);
      if constexpr (ACT == ACX_ACT_GELU) v = acx_gelu(v);
      if constexpr (ACT == ACX_ACT_LEAKYRELU) v = v > 0.f ? v : 0.01f * v;
      if constexpr (ACT == ACX_ACT_RELU) v = fmaxf(v, 0.f);
      outv[r] += v;
      if constexpr (ACT == ACX_ACT_RESRELU) outv[r] = fmaxf(outv[r], 0.f);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(outv[r]));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rowb + (r & 3) + 8 * (r >> 2);
      if (cok && row < d.M) ((float*)d.C)[(size_t)row * d.ldc + col] = outv[r];
    }
  }
}


// =====================================================================================================
// f32 GEMM for SMALL problems (text tower: M = classes x 77 rows): 64 x 64 tiles, 4 waves of 32 x 32, 36 KB of
// LDS -> four blocks (16 waves) per CU.  A 1309 x 512 output is 44 tiles of 128 x 128 -- a sixth of the chip, which
// split-K fills only by adding partial-sum traffic and a reduce launch -- but 168 tiles of 64 x 64.  Same LDS row
// format, K-permutation and K-step schedule as gemm_f32_w8_kernel; FAST problems only.
constexpr int TILE_S = 64 * ROWB;          // 9216 B per operand image
template <int ACT, int RES>
__global__ __launch_bounds__(256, 4) void gemm_f32_s64_kernel(const Args g) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const acx_gemm_desc& d = g.d;
  const int tiles_n = (d.N + 63) / 64;
  const int nwg = gridDim.x;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
  const int wg = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
  const int tm = wg / tiles_n, tn = wg % tiles_n;
  const int m0 = tm * 64, n0 = tn * 64;
  const int t = threadIdx.x;
  const int chunk = t & 7, rbase = t >> 3;                  // 32 staged rows per pass, 2 passes per operand
  // split-K (long-K problems that fill less than the chip: N = 512, K = 2048 at 1078 rows is 136 tiles): blockIdx.y takes
  // K-steps [y * kchunk, ...) and leaves a raw partial tile for splitk_reduce_kernel
  const int nk_total = d.K / 32;
  const int kbeg = g.ksplit > 1 ? (int)blockIdx.y * g.kchunk * 32 : 0;
  const int nk = g.ksplit > 1 ? min(g.kchunk, nk_total - (int)blockIdx.y * g.kchunk) : nk_total;
  const float* pa0 = (const float*)d.A + (size_t)min(m0 + rbase, d.M - 1) * d.lda + chunk * 4 + kbeg;
  const float* pa1 = (const float*)d.A + (size_t)min(m0 + rbase + 32, d.M - 1) * d.lda + chunk * 4 + kbeg;
  const float* pw0 = (const float*)d.W + (size_t)min(n0 + rbase, d.N - 1) * d.ldw + chunk * 4 + kbeg;
  const float* pw1 = (const float*)d.W + (size_t)min(n0 + rbase + 32, d.N - 1) * d.ldw + chunk * 4 + kbeg;
  float4 ra0, ra1, rw0, rw1;
#define S64_LOAD(k0) do { ra0 = ld4(pa0 + (k0)); ra1 = ld4(pa1 + (k0)); rw0 = ld4(pw0 + (k0)); rw1 = ld4(pw1 + (k0)); } while (0)
#define S64_STORE(stage, r)                                                            \
  do {                                                                                 \
    char* sA_ = smem + (stage) * 2 * TILE_S;                                           \
    const int off_ = (rbase + 32 * (r)) * ROWB + chunk * 16;                           \
    *reinterpret_cast<float4*>(sA_ + off_) = ra##r;                                    \
    *reinterpret_cast<float4*>(sA_ + TILE_S + off_) = rw##r;                           \
  } while (0)
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, hh = lane >> 5;
  const int a_off = (wm * 32 + li) * ROWB + hh * 16;
  const int w_off = TILE_S + (wn * 32 + li) * ROWB + hh * 16;
  float4 xa, xb, ya, yb;
#define S64_RD(SET, stage, q)                                                                             \
  do {                                                                                                    \
    const char* sA_ = smem + (stage) * 2 * TILE_S;                                                        \
    SET##a = *reinterpret_cast<const float4*>(sA_ + a_off + (q) * 32);                                    \
    SET##b = *reinterpret_cast<const float4*>(sA_ + w_off + (q) * 32);                                    \
  } while (0)
#define S64_MM(SET)                                                                                       \
  do {                                                                                                    \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(SET##a.x, SET##b.x, acc, 0, 0, 0);                         \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(SET##a.y, SET##b.y, acc, 0, 0, 0);                         \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(SET##a.z, SET##b.z, acc, 0, 0, 0);                         \
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(SET##a.w, SET##b.w, acc, 0, 0, 0);                         \
  } while (0)
  S64_LOAD(0);
  S64_STORE(0, 0); S64_STORE(0, 1);
  __syncthreads();
  if (nk > 1) S64_LOAD(32);
  S64_RD(x, 0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1, nxt = cur ^ 1;
    const bool more = kt + 1 < nk;
    S64_RD(y, cur, 1);
    S64_MM(x);
    S64_RD(x, cur, 2);
    if (more) S64_STORE(nxt, 0);
    S64_MM(y);
    S64_RD(y, cur, 3);
    if (more) S64_STORE(nxt, 1);
    S64_MM(x);
    __syncthreads();
    if (kt + 2 < nk) S64_LOAD((kt + 2) * 32);
    if (more) S64_RD(x, nxt, 0);
    S64_MM(y);
  }
#undef S64_MM
#undef S64_RD
#undef S64_STORE
#undef S64_LOAD
  const int col = n0 + wn * 32 + li;
  const bool cok = col < d.N;
  const int colc = cok ? col : d.N - 1;
  const int rowb = m0 + wm * 32 + 4 * hh;
  if (g.ksplit > 1) {          // raw partial tile; bias / activation / residual happen in splitk_reduce_kernel
    float* P = g.partial + (size_t)blockIdx.y * d.M * d.N;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rowb + (r & 3) + 8 * (r >> 2);
      if (cok && row < d.M) P[(size_t)row * d.N + col] = acc[r];
    }
    return;
  }
  float bias = 0.f;
  if (d.bias) bias = d.bias[colc];
  float outv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) outv[r] = 0.f;
  if constexpr (RES != 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = min(rowb + (r & 3) + 8 * (r >> 2), d.M - 1);
      outv[r] = d.residual[(size_t)row * d.ldr + colc];
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = acc[r] + bias;
    if constexpr (ACT == ACX_ACT_QUICKGELU) v = acx_quickgelu(v);
    if constexpr (ACT == ACX_ACT_GELU) v = acx_gelu(v);
    if constexpr (ACT == ACX_ACT_RELU) v = fmaxf(v, 0.f);
    outv[r] += v;
    if constexpr (ACT == ACX_ACT_RESRELU) outv[r] = fmaxf(outv[r], 0.f);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(outv[r]));
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = rowb + (r & 3) + 8 * (r >> 2);
    if (cok && row < d.M) ((float*)d.C)[(size_t)row * d.ldc + col] = outv[r];
  }
}
