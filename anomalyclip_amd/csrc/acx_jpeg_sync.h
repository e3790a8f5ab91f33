// The self-synchronising parallel Huffman decode of one baseline JPEG scan: the symbol-level core and the per-thread phases, as ONE
// text for the device kernel (acx_jpeg.hip, one workgroup per frame, `Shared` in LDS) and for a CPU build that emulates the
// workgroup's threads serially (tools/jpeg_device_check.cpp, under the sanitizers).  No HIP in here, no allocation, no global state.
//
// The scan arrives un-stuffed (acx_jpeg_scan_pack): a plain string of `scan_bits` bits, most significant first, read as big-endian
// 32-bit words; a read past its last bit gives zero bits, as the host decoder's reader does.  The stream is cut into subsequences of
// `sub` bits, one per thread.  A decoder's STATE is (bit position, block in the MCU, zigzag position): everything the next symbol's
// meaning depends on.  What a thread learns about a subsequence besides the state it leaves in -- the blocks it completed, the
// sum of the DC differences it met per component -- are its COUNTS.
//
//   speculate   thread t decodes subsequence t as if a block, the first of an MCU, began at its first bit, and records state + counts
//   synchronise round r: thread t decodes subsequence t + r from the state it left t + r - 1 in, compares the state it reaches with
//               the recorded one, records its own state and counts in its place, and retires if the states were equal.  Thread 0
//               is right from the start; a thread is right from its first equality with a right record on; and the last thread to
//               touch a record is the lowest-numbered that ever reached it, which entered through the final record before it.  So
//               once a round changes nothing every record is right.  At most nsub - 1 rounds: by then thread 0 has decoded
//               everything itself (the sequential worst case).
//   scan        inclusive prefix sums of the counts (the caller's: barriers on the device, a loop on the CPU)
//   write       thread t decodes subsequence t once more from record t - 1 and stores the coefficients
//
// Every loop is bounded by the bits of a subsequence (a symbol consumes at least one bit; a code no table holds skips one bit),
// by 7 code lengths in a symbol's fallback, or by the number of subsequences.
#ifndef ACX_JPEG_SYNC_H_
#define ACX_JPEG_SYNC_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define ACX_HD __host__ __device__ __forceinline__
#else
#define ACX_HD inline
#endif

namespace acx_jsync {

constexpr int kLook = 9;               // bits of the lookahead table, as in the host decoder
constexpr int kThreads = 1024;         // subsequences (threads) per frame at most
constexpr int kBad = -1;               // == ACX_E_BADARG: the one code the host entropy decoder fails with

// one frame's Huffman record as it travels (== struct acx_jpeg_huff of acx.h); table = class * 4 + index, class 0 DC, 1 AC
constexpr int kHuffPresent = 0, kHuffBits = 8, kHuffVals = 8 + 8 * 17, kHuffTd = kHuffVals + 8 * 256, kHuffTa = kHuffTd + 4;
constexpr int kHuffBytes = kHuffTa + 4;   // 2200

// zigzag position -> natural (row-major) position of a coefficient
constexpr uint8_t kNat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the smallest subsequence size, a multiple of 32 bits, with which kThreads subsequences cover a scan of `bits` bits
ACX_HD uint32_t min_sub_bits(uint64_t bits) {
  const uint64_t per = (bits + kThreads - 1) / kThreads;
  const uint64_t s = (per + 31) / 32 * 32;
  return s < 32 ? 32u : (uint32_t)s;
}

// the block grid of a frame (the tuple acx_jpeg_reconstruct takes); offsets in int16 elements of the frame's coefficients
struct Geo {
  uint32_t ncomp, hs, vs;
  uint32_t nluma, nbm;                 // luma blocks / all blocks of an MCU
  uint32_t mcus_x, bw0, bwc;           // MCUs per row; blocks per row of the luma / of a chroma plane
  uint32_t off1, nbc64;                // first chroma coefficient; coefficients of one chroma plane
  uint32_t total_blocks, coef_elems;
};

// false: not a geometry the decoder has (or too large for 32-bit element offsets)
ACX_HD bool make_geo(int64_t H, int64_t W, int64_t ncomp, int64_t hs, int64_t vs, Geo* g) {
  if (H < 1 || W < 1 || H > 65535 || W > 65535) return false;
  if (!((ncomp == 1 && hs == 1 && vs == 1) || (ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2)))))) return false;
  const uint64_t mx = (uint64_t)(W + 8 * hs - 1) / (uint64_t)(8 * hs), my = (uint64_t)(H + 8 * vs - 1) / (uint64_t)(8 * vs);
  const uint64_t nb0 = mx * hs * my * vs, nbc = ncomp == 3 ? mx * my : 0, nb = nb0 + 2 * nbc;
  if (nb * 64 > 0x7FFFFFFFull) return false;
  g->ncomp = (uint32_t)ncomp; g->hs = (uint32_t)hs; g->vs = (uint32_t)vs;
  g->nluma = (uint32_t)(hs * vs);
  g->nbm = g->nluma + (ncomp == 3 ? 2u : 0u);
  g->mcus_x = (uint32_t)mx; g->bw0 = (uint32_t)(mx * hs); g->bwc = (uint32_t)mx;
  g->off1 = (uint32_t)(nb0 * 64); g->nbc64 = (uint32_t)(nbc * 64);
  g->total_blocks = (uint32_t)nb; g->coef_elems = (uint32_t)(nb * 64);
  return true;
}

// first coefficient of block n in scan order (n < total_blocks: inside the frame whatever else is wrong)
ACX_HD uint32_t block_base(const Geo& g, uint32_t n) {
  const uint32_t m = n / g.nbm, b = n - m * g.nbm;
  const uint32_t my = m / g.mcus_x, mx = m - my * g.mcus_x;
  if (b < g.nluma) {
    const uint32_t v = b / g.hs, h = b - v * g.hs;
    return ((my * g.vs + v) * g.bw0 + mx * g.hs + h) * 64;
  }
  return g.off1 + (b - g.nluma) * g.nbc64 + (my * g.bwc + mx) * 64;
}

// one Huffman table as the decoder reads it (the host decoder's HuffTable with the symbols inside)
struct Table {
  uint16_t look[1 << kLook];           // length << 8 | symbol; 0: longer than kLook bits
  int32_t maxcode[18];
  int32_t valoff[17];
  int32_t nvals;
  uint8_t vals[256];
};

// everything a frame's threads share: LDS on the device
struct Shared {
  Table tab[8];
  uint32_t sel[2][4];                  // [0: DC, 1: AC][component] -> table
  uint32_t pos[kThreads];              // record t: the state after subsequence t ...
  uint32_t bk[kThreads];               // ... block in MCU | zigzag position << 8
  uint32_t nblk[kThreads];             // ... and its counts: blocks completed,
  uint32_t dc[3][kThreads];            // sum of DC differences per component
  int32_t err, done;                   // write pass: an error inside the frame's blocks; the last block ended inside the scan
};

// the codes of a table from the counts per length, into t->look / maxcode / valoff / nvals.  t->look must be zero and t->vals hold the
// symbols already (the device fills both with all its threads).  kBad exactly where the host decoder's derive() refuses.
ACX_HD int derive_codes(const uint8_t* bits, Table* t) {
  uint32_t n = 0, c = 0;
  for (int l = 1; l <= 16; ++l) {
    n += bits[l];
    c += bits[l];
    if (n > 256 || c > (1u << l)) return kBad;          // more symbols than a table has, more codes of a length than the length has
    c <<= 1;
  }
  t->nvals = (int32_t)n;
  uint32_t k = 0;
  c = 0;
  for (int l = 1; l <= 16; ++l) {
    const uint32_t cnt = bits[l];
    if (cnt) {
      t->valoff[l] = (int32_t)k - (int32_t)c;
      if (l <= kLook)
        for (uint32_t i = 0; i < cnt; ++i) {              // (c + i) < 2^l: the fill stays below 2^kLook
          const uint32_t first = (c + i) << (kLook - l);
          const uint16_t e = (uint16_t)((l << 8) | t->vals[k + i]);
          for (uint32_t j = 0; j < (1u << (kLook - l)); ++j) t->look[first + j] = e;
        }
      k += cnt;
      c += cnt;
      t->maxcode[l] = (int32_t)c - 1;
    } else {
      t->maxcode[l] = -1;
      t->valoff[l] = 0;
    }
    c <<= 1;
  }
  t->maxcode[0] = -1;
  t->valoff[0] = 0;
  t->maxcode[17] = 0x7FFFFFFF;
  return 0;
}

// the un-stuffed scan of one frame, and the two words a thread holds of it
struct Scan {
  const uint32_t* w;
  uint32_t bits;                       // valid bits
  uint32_t nwords;                     // words that hold them: (bits + 31) / 32
  uint32_t ci, w0, w1;                 // w0, w1: words ci, ci + 1
};

ACX_HD void scan_init(Scan* s, const uint32_t* w, uint32_t bits) {
  s->w = w;
  s->bits = bits;
  s->nwords = (bits + 31) / 32;
  s->ci = 0xFFFFFFF0u;
  s->w0 = s->w1 = 0;
}

// word i of the stream; zero bits past its end, whatever the buffer holds there
ACX_HD uint32_t scan_word(const Scan& s, uint32_t i) {
  if (i >= s.nwords) return 0u;
  uint32_t v = __builtin_bswap32(s.w[i]);
  if (i == s.nwords - 1 && (s.bits & 31)) v &= ~(0xFFFFFFFFu >> (s.bits & 31));
  return v;
}

// the 32 bits from bit `pos` on, first bit on top
ACX_HD uint32_t window(Scan& s, uint32_t pos) {
  const uint32_t i = pos >> 5, sh = pos & 31;
  if (i != s.ci) {
    s.w0 = i == s.ci + 1 ? s.w1 : scan_word(s, i);
    s.w1 = scan_word(s, i + 1);
    s.ci = i;
  }
  return sh ? (s.w0 << sh) | (s.w1 >> (32 - sh)) : s.w0;
}

// the symbol at the top of `win` and its length, or -1: the host decoder's decode_symbol
ACX_HD int decode_symbol(const Table& t, uint32_t win, uint32_t* len) {
  const uint32_t e = t.look[win >> (32 - kLook)];
  if (e) {
    *len = e >> 8;
    return (int)(e & 255);
  }
  const int32_t v = (int32_t)(win >> 16);
  int l = kLook + 1;
  while (l <= 16 && (v >> (16 - l)) > t.maxcode[l]) ++l;
  if (l > 16) return -1;
  const int idx = (v >> (16 - l)) + t.valoff[l];
  if (idx < 0 || idx >= t.nvals) return -1;
  *len = (uint32_t)l;
  return t.vals[idx];
}

// the s-bit value after a symbol of `len` bits, sign-extended the JPEG way (s in 1 .. 15, len + s <= 31)
ACX_HD int extend(uint32_t win, uint32_t len, uint32_t s) {
  const int v = (int)((win << len) >> (32 - s));
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

struct State {
  uint32_t pos, b, k;                  // bit position; block in the MCU; zigzag position (0: the DC symbol comes next)
};

struct Counts {
  uint32_t nblk;
  uint32_t dc0, dc1, dc2;              // modulo 2^32: a DC is their low 16 bits, as the host decoder truncates
};

// what the write pass carries besides: the block it is in and where that lies, the running DC sums (the counts' prefix sums, then
// the thread's own), and the frame's flags
struct Writer {
  int16_t* coef;
  uint32_t n, base;                    // block in scan order, its first coefficient (n >= total_blocks: padding, nothing is stored)
  int32_t err, done;
};

// decodes from `st` until the position reaches `end`.  WRITE: stores the coefficients of blocks below g.total_blocks; `cnt` must
// then hold the DC sums up to `st` (the predictors) on entry.
template <bool WRITE>
ACX_HD void decode_span(const Shared& S, const Geo& g, Scan& sc, State& st, uint32_t end, Counts& cnt, Writer* w) {
  while (st.pos < end) {
    const uint32_t win = window(sc, st.pos);
    const uint32_t c = st.b < g.nluma ? 0u : st.b - g.nluma + 1u;
    uint32_t len = 0;
    bool bad = false, block_done = false;
    if (st.k == 0) {
      const int s = decode_symbol(S.tab[S.sel[0][c]], win, &len);
      if (s < 0 || s > 15) {
        bad = true;
      } else {
        const int diff = s ? extend(win, len, (uint32_t)s) : 0;
        st.pos += len + (uint32_t)s;
        uint32_t pred;
        if (c == 0) pred = (cnt.dc0 += (uint32_t)diff);
        else if (c == 1) pred = (cnt.dc1 += (uint32_t)diff);
        else pred = (cnt.dc2 += (uint32_t)diff);
        if (WRITE && w->n < g.total_blocks) w->coef[w->base] = (int16_t)(uint16_t)pred;
        st.k = 1;
      }
    } else {
      const int rs = decode_symbol(S.tab[S.sel[1][c]], win, &len);
      if (rs < 0) {
        bad = true;
      } else {
        const uint32_t r = (uint32_t)rs >> 4, s = (uint32_t)rs & 15;
        if (s == 0) {
          st.pos += len;
          if (r != 15) {
            block_done = true;                           // end of block
          } else {
            st.k += 16;
            block_done = st.k >= 64;
          }
        } else if (st.k + r > 63) {
          bad = true;                                    // a run past the block's end
        } else {
          const uint32_t k = st.k + r;
          const int val = extend(win, len, s);
          st.pos += len + s;
          if (WRITE && w->n < g.total_blocks) w->coef[w->base + kNat[k]] = (int16_t)val;
          st.k = k + 1;
          block_done = st.k >= 64;
        }
      }
    }
    if (bad) {                                           // skip a bit: speculation goes on, the true path has failed the frame
      st.pos += 1;
      if (WRITE && w->n < g.total_blocks) w->err = 1;
    }
    if (block_done) {
      st.k = 0;
      st.b = st.b + 1 == g.nbm ? 0u : st.b + 1;
      ++cnt.nblk;
      if (WRITE) {
        if (w->n == g.total_blocks - 1) {                // the frame's last block: inside the scan's bits, or the stream was short
          if (st.pos > sc.bits) w->err = 1;
          else w->done = 1;
        }
        ++w->n;
        if (w->n < g.total_blocks) w->base = block_base(g, w->n);
      }
    }
  }
}

ACX_HD uint32_t pack_bk(const State& st) { return st.b | (st.k << 8); }

ACX_HD void record(Shared& S, uint32_t j, const State& st, const Counts& c) {
  S.pos[j] = st.pos;
  S.bk[j] = pack_bk(st);
  S.nblk[j] = c.nblk;
  S.dc[0][j] = c.dc0;
  S.dc[1][j] = c.dc1;
  S.dc[2][j] = c.dc2;
}

// ---- the phases of thread t (t < nsub; `st` and `active` are the thread's own between the calls)
ACX_HD void phase_speculate(Shared& S, const Geo& g, Scan& sc, uint32_t t, uint32_t sub, State& st) {
  st.pos = t * sub;
  st.b = st.k = 0;
  Counts c = {0, 0, 0, 0};
  decode_span<false>(S, g, sc, st, (t + 1) * sub, c, nullptr);
  record(S, t, st, c);
}

// round r >= 1; true: the record of subsequence t + r changed
ACX_HD bool phase_sync_round(Shared& S, const Geo& g, Scan& sc, uint32_t t, uint32_t r, uint32_t sub, uint32_t nsub, State& st,
                             bool& active) {
  const uint32_t j = t + r;
  if (!active || j >= nsub) {
    active = false;
    return false;
  }
  Counts c = {0, 0, 0, 0};
  decode_span<false>(S, g, sc, st, (j + 1) * sub, c, nullptr);
  const bool same = S.pos[j] == st.pos && S.bk[j] == pack_bk(st);
  record(S, j, st, c);                                   // the counts are this thread's even where the states agree
  if (same) active = false;
  return !same;
}

// after the inclusive scan of nblk and dc over the records
ACX_HD void phase_write(Shared& S, const Geo& g, Scan& sc, uint32_t t, uint32_t sub, int16_t* coef) {
  State st = {0, 0, 0};
  Counts c = {0, 0, 0, 0};
  Writer w = {coef, 0, 0, 0, 0};
  if (t > 0) {
    st.pos = S.pos[t - 1];
    st.b = S.bk[t - 1] & 255;
    st.k = S.bk[t - 1] >> 8;
    w.n = S.nblk[t - 1];
    c.dc0 = S.dc[0][t - 1];
    c.dc1 = S.dc[1][t - 1];
    c.dc2 = S.dc[2][t - 1];
  }
  if (st.b >= g.nbm || st.k > 63) return;                // (no record holds such a state)
  if (w.n < g.total_blocks) w.base = block_base(g, w.n);
  decode_span<true>(S, g, sc, st, (t + 1) * sub, c, &w);
  if (w.err) S.err = 1;
  if (w.done) S.done = 1;
}

}  // namespace acx_jsync
#endif  // ACX_JPEG_SYNC_H_
