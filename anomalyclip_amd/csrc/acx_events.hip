// Anomaly events of unlabeled videos (include/acx.h acx_score_events): per-frame scores -> per video the list of events
// (start, end, class, votes, hot frames, peak frame; peak, mean), on the device.  The per-frame decision is the reference's
// (anomaly_clip_module.py:537-547: normal when abnormal_score < threshold, else the arg-max class); the step from decisions to
// events (hysteresis, gap merging, length filter) is this file's.
//
// Two launches.
//  events_bounds_kernel   one workgroup per video walks it in passes of EV_CHUNK frames (4 consecutive frames per thread) and
//                         finds the kept events' (start, end).  Everything is a forward scan, so a pass needs only a carry:
//                           LC[t] / LH[t]  last cold / last hot frame at or before t      (max-scans)
//                           a warm run ENDS at t (frame t + 1 is cold or past the video); it is a raw event iff LH[t] > LC[t]
//                                          -- the hot frame may lie passes before t -- and starts at LC[t] + 1
//                           PE[t]          end of the last raw event before t             (max-scan): the gap to it decides whether
//                                          the raw event at t heads a new chain
//                           CS[t]          start of the chain that was open before t      (max-scan of the heads' starts)
//                         The chain (CS, PE) is CLOSED by the head that follows it, or by the video's end; the closed events that
//                         pass the length filter are numbered by a sum-scan and written in that order.  The carry between passes is
//                         (LC, LH, PE, CS, events so far): the three things that cross a pass boundary -- a run's hot flag, gap
//                         lengths, open events -- are these five integers.
//  events_stats_kernel    one wave per (video, slot): the event's frames in lane-strided order, per-lane f64 sums / first maxima /
//                         counts joined by a fixed butterfly, votes in an LDS histogram of integer atomics.  Slots without an
//                         event are filled with -1 / NaN here, so the launch sequence needs no memset.
// No float atomics, every join in a fixed order: run-to-run identical.
#include "acx_internal.h"

constexpr int EV_THREADS = 256;
constexpr int EV_ITEMS = 4;
constexpr int EV_CHUNK = EV_THREADS * EV_ITEMS;     // frames per workgroup pass (ops.SCORE_EVENTS_CHUNK)
constexpr int EV_WAVES = EV_THREADS / 64;
constexpr int EV_MAX_C1 = 63;                       // acx_test_counts: 6 <= C <= 64
constexpr int EV_SLOT_GROUPS = 8;                   // workgroups of the stats launch per video
static_assert(EV_CHUNK == 1024 && EV_WAVES == 4, "four waves, four frames per thread");

struct EvMax { __device__ static int id() { return -1; } __device__ static int op(int a, int b) { return a > b ? a : b; } };
struct EvSum { __device__ static int id() { return 0; }  __device__ static int op(int a, int b) { return a + b; } };

// exclusive scan of one value per thread over the workgroup, in thread order; total = all 256 joined.  sh: EV_WAVES ints
template <typename OP>
__device__ __forceinline__ int ev_block_excl(int v, int* sh, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc = OP::op(u, inc);
  }
  int exc = __shfl_up(inc, 1, 64);
  if (lane == 0) exc = OP::id();
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  int pre = OP::id(), tot = OP::id();
#pragma unroll
  for (int w = 0; w < EV_WAVES; ++w) {
    const int x = sh[w];
    if (w < wave) pre = OP::op(pre, x);
    tot = OP::op(tot, x);
  }
  __syncthreads();                                   // sh is free for the next scan
  total = tot;
  return OP::op(pre, exc);
}

__global__ __launch_bounds__(EV_THREADS) void events_bounds_kernel(const float* __restrict__ scores,
                                                                   const long long* __restrict__ row_off, long long n, float hi,
                                                                   float lo, int max_gap, int min_len, int E,
                                                                   int* __restrict__ count, int* __restrict__ events) {
  __shared__ int sh[EV_WAVES];
  const int v = blockIdx.x;
  const long long r0 = row_off[v], r1 = row_off[v + 1];
  if (r0 < 0 || r1 < r0 || r1 > n) {                 // not a range of the n rows: reported, nothing of it is read
    if (threadIdx.x == 0) count[v] = -1;
    return;
  }
  const int T = (int)(r1 - r0);                      // < 2^31 (n is)
  const float* __restrict__ sc = scores + r0;
  int* __restrict__ ev = events + (size_t)v * E * 6;
  int cLC = -1, cLH = -1, cPE = -1, cCS = -1, cN = 0;               // the carry
  for (long long base = 0; base < T; base += EV_CHUNK) {
    const int t0 = (int)base + (int)threadIdx.x * EV_ITEMS;         // <= 2^31 - 4: the pass starts below T
    bool warm[EV_ITEMS + 1], hot[EV_ITEMS];
#pragma unroll
    for (int i = 0; i <= EV_ITEMS; ++i) {
      const bool in = t0 <= T - 1 - i;               // t0 + i < T without overflow
      const float s = in ? sc[t0 + i] : 0.f;
      warm[i] = in && !(s < lo);
      if (i < EV_ITEMS) hot[i] = in && !(s < hi);
    }
    // ---- last cold / last hot frame at or before each frame (frames past the video count as cold: nothing follows them)
    int aC = -1, aH = -1;
#pragma unroll
    for (int i = 0; i < EV_ITEMS; ++i) {
      if (!warm[i]) aC = t0 + i;
      if (hot[i]) aH = t0 + i;
    }
    int totC, totH;
    int lc = EvMax::op(cLC, ev_block_excl<EvMax>(aC, sh, totC));
    int lh = EvMax::op(cLH, ev_block_excl<EvMax>(aH, sh, totH));
    bool raw[EV_ITEMS];
    int rs[EV_ITEMS];
    int aE = -1;
#pragma unroll
    for (int i = 0; i < EV_ITEMS; ++i) {
      if (!warm[i]) lc = t0 + i;
      if (hot[i]) lh = t0 + i;
      raw[i] = warm[i] && !warm[i + 1] && lh > lc;   // a warm run with a hot frame ends here
      rs[i] = lc + 1;
      if (raw[i]) aE = t0 + i;
    }
    // ---- end of the raw event before each frame -> chain heads
    int totE;
    int pe = EvMax::op(cPE, ev_block_excl<EvMax>(aE, sh, totE));
    bool head[EV_ITEMS];
    int pend[EV_ITEMS];
    int aS = -1;
#pragma unroll
    for (int i = 0; i < EV_ITEMS; ++i) {
      pend[i] = pe;
      head[i] = raw[i] && (pe < 0 || rs[i] - pe - 1 > max_gap);
      if (head[i]) aS = rs[i];
      if (raw[i]) pe = t0 + i;
    }
    // ---- start of the chain open before each frame; a head closes it
    int totS;
    int cs = EvMax::op(cCS, ev_block_excl<EvMax>(aS, sh, totS));
    bool keep[EV_ITEMS];
    int st[EV_ITEMS];
    int aK = 0;
#pragma unroll
    for (int i = 0; i < EV_ITEMS; ++i) {
      st[i] = cs;
      keep[i] = head[i] && pend[i] >= 0 && pend[i] - cs + 1 >= min_len;
      if (keep[i]) ++aK;
      if (head[i]) cs = rs[i];
    }
    int totK;
    int k = cN + ev_block_excl<EvSum>(aK, sh, totK);
#pragma unroll
    for (int i = 0; i < EV_ITEMS; ++i) {
      if (keep[i]) {
        if (k < E) { ev[k * 6] = st[i]; ev[k * 6 + 1] = pend[i]; }
        ++k;
      }
    }
    cLC = EvMax::op(cLC, totC); cLH = EvMax::op(cLH, totH); cPE = EvMax::op(cPE, totE); cCS = EvMax::op(cCS, totS);
    cN += totK;
  }
  if (threadIdx.x == 0) {                            // the video's end closes the open chain
    if (cPE >= 0 && cPE - cCS + 1 >= min_len) {
      if (cN < E) { ev[cN * 6] = cCS; ev[cN * 6 + 1] = cPE; }
      ++cN;
    }
    count[v] = cN;
  }
}

// (peak value, its frame): the larger value, on a tie the earlier frame; frame < 0: none yet
__device__ __forceinline__ void ev_peak_join(float& pk, int& pf, float ok, int of) {
  if (of >= 0 && (pf < 0 || ok > pk || (ok == pk && of < pf))) { pk = ok; pf = of; }
}

__global__ __launch_bounds__(EV_THREADS) void events_stats_kernel(const float* __restrict__ scores, const float* __restrict__ probs,
                                                                  const long long* __restrict__ row_off, int C1, float hi,
                                                                  int normal_idx, int E, const int* __restrict__ count,
                                                                  int* __restrict__ events, double* __restrict__ stats) {
  __shared__ int hist[EV_WAVES][64];
  const int v = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cnt = count[v];
  const int have = cnt < 0 ? 0 : (cnt < E ? cnt : E);
  const long long r0 = have ? row_off[v] : 0;        // (a refused video's offsets are not used)
  int* __restrict__ ev = events + (size_t)v * E * 6;
  double* __restrict__ stv = stats + (size_t)v * E * 2;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  // every wave of the workgroup makes the same number of rounds (the barriers below), whatever its slot holds
  for (int jb = blockIdx.y * EV_WAVES; jb < E; jb += gridDim.y * EV_WAVES) {
    const int slot = jb + wave;
    const bool active = slot < have;
    hist[wave][lane] = 0;
    __syncthreads();
    int start = 0, end = -1;
    double sum = 0.0;
    int valid = 0, nhot = 0, pf = -1;
    float pk = 0.f;
    if (active) {
      start = ev[slot * 6]; end = ev[slot * 6 + 1];
      for (long long t = (long long)start + lane; t <= end; t += 64) {
        const float s = scores[r0 + t];
        if (s == s) {
          sum += (double)s;
          ++valid;
          if (pf < 0 || s > pk) { pk = s; pf = (int)t; }
        }
        if (!(s < hi)) {
          ++nhot;
          const float* __restrict__ p = probs + (size_t)(r0 + t) * C1;
          int am = 0;
          float best = -__builtin_inff();
          for (int j = 0; j < C1; ++j) {
            const float x = p[j];
            if (x > best) { best = x; am = j; }
          }
          atomicAdd(&hist[wave][am], 1);
        }
      }
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {             // fixed butterfly: every lane ends with the same bits
        sum += __shfl_xor(sum, o, 64);
        valid += __shfl_xor(valid, o, 64);
        nhot += __shfl_xor(nhot, o, 64);
        const float ok = __shfl_xor(pk, o, 64);
        const int of = __shfl_xor(pf, o, 64);
        ev_peak_join(pk, pf, ok, of);
      }
      int votes = lane < C1 ? hist[wave][lane] : -1, cls = lane;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {             // most votes, on a tie the lowest class
        const int ov = __shfl_xor(votes, o, 64), oc = __shfl_xor(cls, o, 64);
        if (ov > votes || (ov == votes && oc < cls)) { votes = ov; cls = oc; }
      }
      if (lane == 0) {
        ev[slot * 6 + 2] = cls >= normal_idx ? cls + 1 : cls;
        ev[slot * 6 + 3] = votes;
        ev[slot * 6 + 4] = nhot;
        ev[slot * 6 + 5] = pf < 0 ? start : pf;
        stv[slot * 2] = pf < 0 ? nan : (double)pk;
        stv[slot * 2 + 1] = valid ? sum / (double)valid : nan;
      }
    } else if (slot < E) {
      if (lane < 6) ev[slot * 6 + lane] = -1;
      else if (lane < 8) stv[slot * 2 + lane - 6] = nan;
    }
  }
}

extern "C" int64_t acx_score_events_workspace_bytes(int64_t n, int64_t videos, int32_t max_events) {
  if (n < 0 || n >= (1ll << 31) || videos < 0 || videos >= (1ll << 31) || max_events < 1) return -1;
  return 0;                                          // the carry lives in registers, the events in the output tables
}

extern "C" int acx_score_events(acx_ctx* ctx, const float* scores, const float* probs, const int64_t* row_off, int64_t n,
                                int64_t videos, int32_t C1, int32_t normal_idx, float hi, float lo, int32_t max_gap,
                                int32_t min_len, int32_t max_events, int32_t* count, int32_t* events, double* stats,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || n >= (1ll << 31)) return acx_fail(ctx, ACX_E_BADARG, "acx_score_events: %sn=%ld out of range", "", (long)n);
  if (videos < 0 || videos >= (1ll << 31))
    return acx_fail(ctx, ACX_E_BADARG, "acx_score_events: %svideos=%ld out of range", "", (long)videos);
  if (C1 < 5 || C1 > EV_MAX_C1 || normal_idx < 0 || normal_idx > C1)
    return acx_fail(ctx, ACX_E_BADARG, "acx_score_events: need 5 <= C1 <= 63 and 0 <= normal_idx <= C1 (acx_test_counts' classes "
                                       "without the normal column), %sgot C1=%ld, normal_idx=%ld", "", (long)C1, (long)normal_idx);
  if (!(lo <= hi)) return acx_fail(ctx, ACX_E_BADARG, "acx_score_events: lo > hi (or a NaN threshold)%s", "");
  if (max_gap < 0) return acx_fail(ctx, ACX_E_BADARG, "acx_score_events: %smax_gap=%ld < 0", "", (long)max_gap);
  if (min_len < 1) return acx_fail(ctx, ACX_E_BADARG, "acx_score_events: %smin_len=%ld < 1", "", (long)min_len);
  if (max_events < 1) return acx_fail(ctx, ACX_E_BADARG, "acx_score_events: %smax_events=%ld < 1", "", (long)max_events);
  if (videos * (int64_t)max_events >= (1ll << 31))
    return acx_fail(ctx, ACX_E_BADARG, "acx_score_events: %svideos * max_events = %ld slots, need < 2^31", "",
                    (long)(videos * (int64_t)max_events));
  if (workspace_bytes < acx_score_events_workspace_bytes(n, videos, max_events))
    return acx_fail(ctx, ACX_E_WORKSPACE, "acx_score_events: workspace too small%s", "");
  if (!ctx) return acx_fail(ctx, ACX_E_BADARG, "acx_score_events: null context%s", "");
  if (videos == 0) return ACX_OK;
  if (!row_off || !count || !events || !stats || (n > 0 && (!scores || !probs)))
    return acx_fail(ctx, ACX_E_BADARG, "acx_score_events: null buffer%s", "");
  (void)workspace;
  hipStream_t st = (hipStream_t)stream;
  AcxProfScope prof(ctx, ACX_K_OTHER, st);
  events_bounds_kernel<<<(unsigned)videos, EV_THREADS, 0, st>>>(scores, (const long long*)row_off, (long long)n, hi, lo, max_gap,
                                                                min_len, max_events, count, events);
  const int groups = (max_events + EV_WAVES - 1) / EV_WAVES;
  events_stats_kernel<<<dim3((unsigned)videos, groups < EV_SLOT_GROUPS ? groups : EV_SLOT_GROUPS), EV_THREADS, 0, st>>>(
      scores, probs, (const long long*)row_off, C1, hi, normal_idx, max_events, count, events, stats);
  ACX_CHECK_LAUNCH(ctx, "acx_score_events");
  return ACX_OK;
}
