// acx_attention_cls, acx_attention_cls_fold -- the CLS row of the last ViT layer: attn_cls_kernel and the three cls_fold kernels
// (included by acx_attn.hip inside its anonymous namespace)
//
// CLS-only attention for the LAST ViT layer: only token 0 of every sequence is consumed downstream
// (clip/model.py:285 takes x[:, 0, :]), so only query row 0 needs softmax(q k^T) v.  One wavefront per
// (sequence, head): lanes own keys for the scores, then own output dims for the weighted sum of V.
__global__ __launch_bounds__(256) void attn_cls_kernel(const float* __restrict__ qkv, int64_t ldqkv, float* __restrict__ out,
                                                       int64_t ldo, int batch, int L, int heads) {
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= (int64_t)batch * heads) return;
  const int b = (int)(idx / heads), h = (int)(idx % heads);
  const int W = heads * 64;
  const float* base = qkv + (int64_t)b * L * ldqkv + h * 64;
  float q[64];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const float4 v = *reinterpret_cast<const float4*>(base + 4 * c);
    q[4 * c] = v.x * 0.125f; q[4 * c + 1] = v.y * 0.125f; q[4 * c + 2] = v.z * 0.125f; q[4 * c + 3] = v.w * 0.125f;
  }
  // keys in blocks of 256 (four per lane) with a running max and sum; a single block (L <= 256) is the two-pass form exactly
  // (first block: exp(-inf) = 0 scales the empty sum and output)
  float mx = -INFINITY, sum = 0.f, o = 0.f;
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
        for (int c = 0; c < 16; ++c) {
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
    o *= al;
    const int k1 = min(L, k0 + 256);
    for (int j = k0; j < k1; ++j) {
      const int u_ = (j - k0) >> 6;
      const float mine = u_ == 0 ? sc[0] : (u_ == 1 ? sc[1] : (u_ == 2 ? sc[2] : sc[3]));
      const float p = __shfl(mine, j & 63, 64);
      o += p * base[(int64_t)j * ldqkv + 2 * W + lane];
    }
  }
  out[(int64_t)b * ldo + h * 64 + lane] = o / sum;
}

// ------------------------------------------------------------------------------------------------------------------------
// CLS-row attention of the pruned last ViT layer WITHOUT the K | V product (acx_attention_cls_fold).  With one query per
// (frame, head) the projections fold into the query and the output:
//   y_j = ln_1(x_j) = n_j * g + c,  n_j = (x_j - mean_j) rstd_j
//   s_j = q_h . k_{j,h} / 8 = u_h . n_j + const,   u_h = g * W_{k,h}^T q_h / 8   (q_h . b_k and W_{k,h}^T q_h . c do not depend on j:
//                                                                                  they cancel in the softmax)
//   o_h = sum_j p_j v_{j,h} = W_{v,h} z_h + b_{v,h},  z_h = g * (sum_j p_j n_j) + c                         (sum_j p_j = 1)
// Three launches: u for all frames (the K rows of in_proj read once per 16 frames), one workgroup per frame for scores, softmax
// and z, then o for all frames (the V rows read once per 8 frames).  Every sum runs in a fixed order over one frame's data only: a
// frame's result does not depend on the batch or on the frame's place in it.

constexpr int CF_UF = 16;   // frames per workgroup of cls_fold_u_kernel
constexpr int CF_OF = 8;    // frames per workgroup of cls_fold_o_kernel

// u [batch, H, W]: grid (H, ceil(batch / CF_UF)); a thread owns columns c = tid + 256 i and sums the head's 64 rows of W_k in order
__global__ __launch_bounds__(256) void cls_fold_u_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ wk,
                                                         const float* __restrict__ lnw, float* __restrict__ u, int batch, int W) {
  __shared__ __attribute__((aligned(16))) float qs[64][CF_UF];
  const int h = blockIdx.x, H = gridDim.x, f0 = blockIdx.y * CF_UF;
  for (int i = threadIdx.x; i < 64 * CF_UF; i += 256) {
    const int f = i >> 6, d = i & 63;
    const int fb = f0 + f < batch ? f0 + f : batch - 1;                          // (past the batch: a copy of its last frame, never stored)
    qs[d][f] = q[(int64_t)fb * ldq + h * 64 + d];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < W; c += 256) {
    float acc[CF_UF];
#pragma unroll
    for (int f = 0; f < CF_UF; ++f) acc[f] = 0.f;
    const float* wp = wk + (int64_t)h * 64 * W + c;
#pragma unroll 4
    for (int d = 0; d < 64; ++d) {
      const float w = wp[(int64_t)d * W];
#pragma unroll
      for (int f4 = 0; f4 < CF_UF / 4; ++f4) {
        const float4 qv = *reinterpret_cast<const float4*>(&qs[d][4 * f4]);
        acc[4 * f4] += qv.x * w; acc[4 * f4 + 1] += qv.y * w; acc[4 * f4 + 2] += qv.z * w; acc[4 * f4 + 3] += qv.w * w;
      }
    }
    const float g = lnw[c] * 0.125f;
#pragma unroll
    for (int f = 0; f < CF_UF; ++f)
      if (f0 + f < batch) u[((int64_t)(f0 + f) * H + h) * W + c] = acc[f] * g;
  }
}

// One workgroup (4 waves) per frame.  Dynamic LDS: u [H][W] | scores, then softmax weights times rstd [L][HP] | (mean, rstd) [L].
//   pass 1: a wave normalises R rows in registers (layernorm_kernel's row layout and sums) and writes their H scores
//   softmax over L per head (one wave per head)
//   pass 2: a thread owns columns c = tid + 256 k for all heads and sums the rows in order (re-read: L2 / MALL)
template <int VPL>
__global__ __launch_bounds__(256) void cls_fold_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                       const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                       float* __restrict__ z, int L, float eps) {
  constexpr int W = 64 * VPL, H = VPL, HP = (H + 3) & ~3, R = 4, CP = (VPL + 3) / 4;
  constexpr float invD = 1.f / W;
  extern __shared__ __attribute__((aligned(16))) float cf_smem[];
  float* us = cf_smem;
  float* sc = us + H * W;
  float2* st = reinterpret_cast<float2*>(sc + (size_t)L * HP);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* xb = x + (int64_t)blockIdx.x * L * W;
  const float* ub = u + (int64_t)blockIdx.x * H * W;
  for (int i = 4 * tid; i < H * W; i += 1024) *reinterpret_cast<float4*>(us + i) = *reinterpret_cast<const float4*>(ub + i);
  __syncthreads();

  for (int j0 = wave * R; j0 < L; j0 += 4 * R) {
    float v[R][VPL], rs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) load_row<VPL>(xb + (int64_t)(j0 + r < L ? j0 + r : L - 1) * W, lane, v[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) s += v[r][i];
      const float mean = wave_sum(s) * invD;
      float qq = 0.f;
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        v[r][i] -= mean;
        qq += v[r][i] * v[r][i];
      }
      rs[r] = 1.f / sqrtf(wave_sum(qq) * invD + eps);
      if (lane == 0 && j0 + r < L) st[j0 + r] = make_float2(mean, rs[r]);
    }
#pragma unroll 1
    for (int h = 0; h < H; ++h) {
      float uu[VPL];
      load_row<VPL>(us + h * W, lane, uu);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < VPL; ++i) d += v[r][i] * uu[i];
        d = wave_sum(d) * rs[r];
        if (lane == 0 && j0 + r < L) sc[(j0 + r) * HP + h] = d;
      }
    }
  }
  __syncthreads();

  for (int h = wave; h < H; h += 4) {
    float m = -INFINITY;
    for (int j = lane; j < L; j += 64) m = fmaxf(m, sc[j * HP + h]);
    m = wave_max(m);
    float s = 0.f;
    for (int j = lane; j < L; j += 64) {
      const float e = expf(sc[j * HP + h] - m);
      sc[j * HP + h] = e;
      s += e;
    }
    const float inv = 1.f / wave_sum(s);
    for (int j = lane; j < L; j += 64) sc[j * HP + h] *= inv * st[j].y;
  }
  __syncthreads();

  float acc[CP][H];
#pragma unroll
  for (int k = 0; k < CP; ++k)
#pragma unroll
    for (int h = 0; h < H; ++h) acc[k][h] = 0.f;
#define CF_ROWS(NJ)                                                                                 \
  {                                                                                                 \
    float xv[NJ][CP];                                                                               \
    _Pragma("unroll") for (int t = 0; t < NJ; ++t)                                                  \
      _Pragma("unroll") for (int k = 0; k < CP; ++k)                                                \
        xv[t][k] = tid + 256 * k < W ? xb[(int64_t)(j + t) * W + tid + 256 * k] : 0.f;              \
    _Pragma("unroll") for (int t = 0; t < NJ; ++t) {                                                \
      const float mean = st[j + t].x;                                                               \
      float a[HP];                                                                                  \
      _Pragma("unroll") for (int h4 = 0; h4 < HP / 4; ++h4) {                                       \
        const float4 a4 = *reinterpret_cast<const float4*>(sc + (j + t) * HP + 4 * h4);             \
        a[4 * h4] = a4.x; a[4 * h4 + 1] = a4.y; a[4 * h4 + 2] = a4.z; a[4 * h4 + 3] = a4.w;         \
      }                                                                                             \
      _Pragma("unroll") for (int k = 0; k < CP; ++k) {                                              \
        const float d = xv[t][k] - mean;                                                            \
        _Pragma("unroll") for (int h = 0; h < H; ++h) acc[k][h] += a[h] * d;                        \
      }                                                                                             \
    }                                                                                               \
  }
  int j = 0;
  for (; j + 4 <= L; j += 4) CF_ROWS(4)
  for (; j < L; ++j) CF_ROWS(1)
#undef CF_ROWS
  float* zb = z + (int64_t)blockIdx.x * H * W;
#pragma unroll
  for (int k = 0; k < CP; ++k) {
    const int c = tid + 256 * k;
    if (c < W) {
      const float g = lnw[c], b0 = lnb[c];
#pragma unroll
      for (int h = 0; h < H; ++h) zb[h * W + c] = acc[k][h] * g + b0;
    }
  }
}

// out [batch, 64 H]: grid (H, ceil(batch / CF_OF)); a wave owns 16 of the head's 64 output elements, its lanes stride the columns
__global__ __launch_bounds__(256) void cls_fold_o_kernel(const float* __restrict__ z, const float* __restrict__ wv,
                                                         const float* __restrict__ bv, float* __restrict__ out, int64_t ldo,
                                                         int batch, int W) {
  __shared__ __attribute__((aligned(16))) float zs[CF_OF * 1024];
  const int h = blockIdx.x, H = gridDim.x, f0 = blockIdx.y * CF_OF;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int f = 0; f < CF_OF; ++f) {
    const int fb = f0 + f < batch ? f0 + f : batch - 1;
    const float* zp = z + ((int64_t)fb * H + h) * W;
    for (int c = threadIdx.x; c < W; c += 256) zs[f * W + c] = zp[c];
  }
  __syncthreads();
  for (int e = wave; e < 64; e += 4) {
    const float* wr = wv + (int64_t)(h * 64 + e) * W;
    float acc[CF_OF];
#pragma unroll
    for (int f = 0; f < CF_OF; ++f) acc[f] = 0.f;
    for (int c = lane; c < W; c += 64) {
      const float w = wr[c];
#pragma unroll
      for (int f = 0; f < CF_OF; ++f) acc[f] += w * zs[f * W + c];
    }
    const float b0 = bv[h * 64 + e];
#pragma unroll
    for (int f = 0; f < CF_OF; ++f) {
      const float o = wave_sum(acc[f]) + b0;
      if (lane == f && f0 + f < batch) out[(int64_t)(f0 + f) * ldo + h * 64 + e] = o;
    }
  }
}
