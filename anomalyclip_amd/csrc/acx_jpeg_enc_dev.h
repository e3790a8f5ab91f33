// Huffman coding of baseline JPEG frames in parallel: the scan-order map, the per-block coder and the per-lane phases, as ONE text
// for the device kernels (acx_jpeg_enc.hip) and for a CPU build that runs the lanes in a loop (tools/jpeg_encode_dev_check.cpp,
// under the sanitizers).  No HIP in here, no allocation, no global state.  The file it makes is byte for byte the one
// acx_jpeg_enc_host.h's entropy_encode writes: 3 components, luma sampling 2x2, the Annex K tables, one interleaved scan.
//
// Encoding needs no speculation: the tables are fixed, and a block's code depends on the block and on the DC of the previous block
// of its component, which sits at a known place of the coefficient layout.  So:
//
//   count   lane s codes block s of the scan into a sink that only adds the lengths up -> its bits (kErrBit: a value the tables
//           cannot code)
//   scan    exclusive prefix sum of the lengths of a frame (the caller's: a workgroup's scan on the device, a loop on the CPU) ->
//           every block's bit offset, the frame's bits and, rounded up to a byte, the un-stuffed bytes U
//   write   lane s codes block s once more into a sink that shifts the bits into a 64-bit accumulator and hands every completed
//           32-bit word to the memory: a word that lies wholly inside the block is a plain store; the first word of a block that
//           begins inside a word, and the block's last partial word, are OR-merged into the ZEROED string (neighbours share them;
//           OR does not depend on the order).  The last block fills the last byte with one bits.
//   stuff   lane i owns word i of the un-stuffed string: it counts its FF bytes; sums per chunk of kChunkBytes and an exclusive
//           prefix sum of the chunks (the caller's) give every word its place in the file, where it writes its bytes and a 00
//           behind every FF.  The file is header | stuffed scan | FF D9.
//
// The string is big-endian: bit i of the scan is bit 7 - i % 8 of byte i / 8.  A word w holds bits 32 w ... 32 w + 31, first bit on
// top, and is stored byte-swapped on the little-endian machines this runs on.
//
// Loop bounds: a block is at most kMaxBlockBits = 20 + 63 * 26 bits (DC: a code of 9 and 11 extra bits; every AC a code of 16 and
// 10 extra bits); every loop runs over 64 coefficients, 3 ZRL codes, 16 code lengths, 256 symbols or the 4 bytes of a word.  No trip
// count comes from the data.
#ifndef ACX_JPEG_ENC_DEV_H_
#define ACX_JPEG_ENC_DEV_H_

#include "acx_jpeg_enc_host.h"

#if defined(__HIPCC__)
#define ACX_HD __host__ __device__ __forceinline__
#else
#define ACX_HD inline
#endif

namespace acx_jenc {

constexpr int kMaxBlockBits = 20 + 63 * 26;              // 1,658
constexpr uint32_t kErrBit = 0x80000000u;                // in a block's count: DC difference category > 11, or |AC| > 1023
constexpr uint32_t kChunkBytes = 256;                    // of the un-stuffed string: 64 lanes x one 32-bit word
constexpr int64_t kMaxFrameBits = 0x7FFFFFFFll - 64;     // blocks x kMaxBlockBits stays below this: bit offsets are 32-bit

// zigzag position -> natural (row-major) position of a coefficient
constexpr uint8_t kNat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---------------------------------------------------------------------------------------------------------------- the tables
// the Annex K tables as the coder reads them: (length << 16) | code of every symbol, 0 where the table has none
struct Tabs {
  uint32_t dc[2][16];                                    // luma, chroma; symbol = category 0 .. 11
  uint32_t ac[2][256];                                   // symbol = run << 4 | category
};

constexpr void derive(const uint8_t* bits16, const uint8_t* vals, uint32_t* out) {
  uint32_t c = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits16[l - 1]; ++i, ++k) out[vals[k]] = ((uint32_t)l << 16) | c++;
    c <<= 1;
  }
}

constexpr Tabs make_tabs() {
  Tabs t{};
  derive(acx_jpeg::kDcLumaBits, acx_jpeg::kDcVals, t.dc[0]);
  derive(acx_jpeg::kDcChromaBits, acx_jpeg::kDcVals, t.dc[1]);
  derive(acx_jpeg::kAcLumaBits, acx_jpeg::kAcLumaVals, t.ac[0]);
  derive(acx_jpeg::kAcChromaBits, acx_jpeg::kAcChromaVals, t.ac[1]);
  return t;
}

constexpr Tabs kTabs = make_tabs();

// ---------------------------------------------------------------------------------------------------------------- the scan order
// A frame of H x W, padded to whole 16 x 16 MCUs.  The interleaved scan visits MCU after MCU, row by row; in an MCU the four luma
// blocks (top left, top right, bottom left, bottom right), then Cb, then Cr: block s of the scan is block s % 6 of MCU s / 6.
// Offsets are int16 elements of the frame's coefficients (acx_jpeg_host.h's layout()).
struct Geo {
  uint32_t mx, my;                                       // MCUs per row, rows of MCUs
  uint32_t nb;                                           // blocks of the frame: 6 per MCU
  uint32_t off1, off2;                                   // the first coefficient of Cb, of Cr
};

// false: not a size a JPEG frame has, or a scan whose bit offsets could pass 32 bits
ACX_HD bool make_geo(int64_t H, int64_t W, Geo* g) {
  if (H < 1 || W < 1 || H > 65535 || W > 65535) return false;
  const int64_t mx = (W + 15) / 16, my = (H + 15) / 16, nb = mx * my * 6;
  if (nb * kMaxBlockBits > kMaxFrameBits) return false;
  g->mx = (uint32_t)mx;
  g->my = (uint32_t)my;
  g->nb = (uint32_t)nb;
  g->off1 = (uint32_t)(mx * my * 4 * 64);
  g->off2 = (uint32_t)(mx * my * 5 * 64);
  return true;
}

ACX_HD uint32_t coef_elems(const Geo& g) { return g.nb * 64u; }

// block s of the scan -> the offset of its 64 coefficients; *comp: 0 luma, 1 Cb, 2 Cr
ACX_HD uint32_t block_offset(const Geo& g, uint32_t s, uint32_t* comp) {
  const uint32_t mcu = s / 6u, k = s - mcu * 6u;
  if (k >= 4u) {
    *comp = k - 3u;
    return (k == 4u ? g.off1 : g.off2) + mcu * 64u;
  }
  const uint32_t my = mcu / g.mx, mxi = mcu - my * g.mx;
  *comp = 0;
  return ((2u * my + (k >> 1)) * (2u * g.mx) + 2u * mxi + (k & 1u)) * 64u;
}

// the other way: block (by, bx) of component comp -> its place in the scan
ACX_HD uint32_t scan_index(const Geo& g, uint32_t comp, uint32_t by, uint32_t bx) {
  if (comp == 0) return ((by >> 1) * g.mx + (bx >> 1)) * 6u + (by & 1u) * 2u + (bx & 1u);
  return (by * g.mx + bx) * 6u + 3u + comp;
}

// the block of the same component that the scan visits before block s (its DC is the predictor), or -1: the predictor is 0
ACX_HD int64_t block_pred(uint32_t s) {
  const uint32_t k = s % 6u;
  if (k >= 4u) return s >= 6u ? (int64_t)s - 6 : -1;
  if (k != 0u) return (int64_t)s - 1;
  return s != 0u ? (int64_t)s - 3 : -1;
}

ACX_HD int pred_dc(const Geo& g, const int16_t* coef, uint32_t s) {
  const int64_t p = block_pred(s);
  if (p < 0) return 0;
  uint32_t c;
  return coef[block_offset(g, (uint32_t)p, &c)];
}

// ---------------------------------------------------------------------------------------------------------------- the block coder
// the category of a value, at most `most`, and the bits that follow the symbol; *ok &= the value has a category the table codes
ACX_HD int magnitude(int v, int most, uint32_t* extra, bool* ok) {
  const int a = v < 0 ? -v : v;
  int s = a ? 32 - __builtin_clz((unsigned)a) : 0;
  if (s > most) {                                        // refused: the block keeps a length within kMaxBlockBits, its bits mean nothing
    *ok = false;
    s = most;
  }
  *extra = (uint32_t)(v < 0 ? v + (1 << s) - 1 : v) & ((1u << s) - 1u);
  return s;
}

// a block's 64 coefficients in natural order, in memory; the kernels hold them in registers instead (acx_jpeg_enc.hip)
struct PtrBlock {
  const int16_t* p;
  ACX_HD int operator()(int i) const { return p[i]; }
};

// One block (blk(i): its coefficient at natural position i) into `sink`, as entropy_encode's inner loop codes it: the DC difference's category and extra bits; per non-zero AC
// coefficient in zigzag order a ZRL for every 16 zeros before it, then the symbol run << 4 | category and the extra bits; EOB
// unless coefficient 63 is set.  sink.put(v, len) takes the low `len` <= 27 bits `v` (nothing above them set): a symbol's code and
// its extra bits in one piece.  -> false: the block holds a value the tables cannot code.
// The loop over the zigzag positions is unrolled, so that every position is a constant: a block held in registers is never
// indexed by a variable.
template <class Blk, class Sink>
ACX_HD bool encode_block(const Blk& blk, int pred, const uint32_t* dc, const uint32_t* ac, Sink& sink) {
  bool ok = true;
  uint32_t extra;
  int s = magnitude(blk(0) - pred, 11, &extra, &ok);
  uint32_t e = dc[s];
  sink.put(((e & 0xFFFFu) << s) | extra, (int)(e >> 16) + s);
  int run = 0;
#pragma unroll
  for (int k = 1; k < 64; ++k) {
    const int a = blk(kNat[k]);
    if (a == 0) {
      ++run;
      continue;
    }
    for (int z = 0; z < 3; ++z)                          // a run is at most 62
      if (run >= 16) {
        sink.put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
        run -= 16;
      }
    s = magnitude(a, 10, &extra, &ok);
    e = ac[(run << 4) | s];
    sink.put(((e & 0xFFFFu) << s) | extra, (int)(e >> 16) + s);
    run = 0;
  }
  if (run) sink.put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
  return ok;
}

struct CountSink {
  uint32_t bits;
  ACX_HD void put(uint32_t, int len) { bits += (uint32_t)len; }
};

// The writing sink.  Mem has store(w, v) and merge(w, v): word w of the frame's string becomes / is OR-ed with v (v given with the
// first bit on top: Mem swaps the bytes).  `pos` is the bit the next put begins at.
template <class Mem>
struct WordSink {
  Mem mem;
  uint64_t acc;                                          // the `fill` bits not yet handed on, at the bottom
  uint32_t pos, w;
  int fill;
  bool merge;                                            // the next word is shared with the block before

  ACX_HD void start(uint32_t bit_off) {
    pos = bit_off;
    w = bit_off >> 5;
    fill = (int)(bit_off & 31u);                         // the bits before the block: zeros here, the neighbour's in memory
    acc = 0;
    merge = fill != 0;
  }
  ACX_HD void put(uint32_t v, int len) {
    acc = (acc << len) | v;
    fill += len;
    pos += (uint32_t)len;
    if (fill >= 32) {
      const uint32_t word = (uint32_t)(acc >> (fill - 32));
      if (merge)
        mem.merge(w, word);
      else
        mem.store(w, word);
      merge = false;
      ++w;
      fill -= 32;
      acc &= (1ull << fill) - 1ull;
    }
  }
  ACX_HD void finish() {
    if (fill) mem.merge(w, (uint32_t)(acc << (32 - fill)));
    fill = 0;
  }
};

// ---------------------------------------------------------------------------------------------------------------- the lanes
// count: the bits of a block of component `comp` whose predictor is `pred`, kErrBit set where it cannot be coded
template <class Blk>
ACX_HD uint32_t count_block(const Blk& blk, int pred, uint32_t comp, const Tabs* t) {
  const uint32_t tc = comp ? 1u : 0u;
  CountSink sink = {0};
  const bool ok = encode_block(blk, pred, t->dc[tc], t->ac[tc], sink);
  return sink.bits | (ok ? 0u : kErrBit);
}

// write: the block at bit `bit_off` of the frame's zeroed string; the last block of the scan pads the last byte with ones
template <class Blk, class Mem>
ACX_HD void write_block(const Blk& blk, int pred, uint32_t comp, bool last, uint32_t bit_off, const Tabs* t, const Mem& mem) {
  const uint32_t tc = comp ? 1u : 0u;
  WordSink<Mem> sink = {mem, 0, 0, 0, 0, false};
  sink.start(bit_off);
  encode_block(blk, pred, t->dc[tc], t->ac[tc], sink);
  if (last) {
    const int pad = (int)((0u - sink.pos) & 7u);
    if (pad) sink.put((1u << pad) - 1u, pad);
  }
  sink.finish();
}

// ... of block s of the scan of the frame `coef`, read from memory
ACX_HD uint32_t count_lane(const Geo& g, const int16_t* coef, uint32_t s, const Tabs* t) {
  uint32_t c;
  const PtrBlock blk = {coef + block_offset(g, s, &c)};
  return count_block(blk, pred_dc(g, coef, s), c, t);
}

template <class Mem>
ACX_HD void write_lane(const Geo& g, const int16_t* coef, uint32_t s, uint32_t bit_off, const Tabs* t, const Mem& mem) {
  uint32_t c;
  const PtrBlock blk = {coef + block_offset(g, s, &c)};
  write_block(blk, pred_dc(g, coef, s), c, s == g.nb - 1u, bit_off, t, mem);
}

// the un-stuffed bytes of a scan of `bits` bits
ACX_HD uint32_t scan_bytes(uint32_t bits) { return (bits + 7u) >> 3; }
ACX_HD uint32_t chunks_of(uint32_t bytes) { return (bytes + kChunkBytes - 1u) / kChunkBytes; }

// stuff: `word` as loaded from bytes byte0 ... byte0 + 3 of a string of U bytes -> the FF bytes among those inside the string
ACX_HD uint32_t ff_count(uint32_t word, uint32_t byte0, uint32_t U) {
  uint32_t n = 0;
  for (uint32_t j = 0; j < 4u; ++j)
    if (byte0 + j < U && ((word >> (8u * j)) & 255u) == 255u) ++n;
  return n;
}

// ... and its bytes, a 00 behind every FF, from dst[at] on; nothing at or past dst + cap
ACX_HD void emit_word(uint32_t word, uint32_t byte0, uint32_t U, int64_t at, uint8_t* dst, int64_t cap) {
  for (uint32_t j = 0; j < 4u; ++j)
    if (byte0 + j < U) {
      const uint8_t b = (uint8_t)(word >> (8u * j));
      if (at < cap) dst[at] = b;
      ++at;
      if (b == 255u) {
        if (at < cap) dst[at] = 0;
        ++at;
      }
    }
}

// the file: header | U bytes with `ff` FF bytes among them, stuffed | FF D9
ACX_HD int64_t file_bytes(int64_t header_bytes, uint32_t U, uint32_t ff) { return header_bytes + (int64_t)U + ff + 2; }

// ---------------------------------------------------------------------------------------------------------------- the workspace
// of B frames, in bytes from a 16-byte aligned base: per frame 4 words of results, the blocks' bit counts (then offsets), the
// chunks' FF counts (then offsets) and the string at its longest -- every block kMaxBlockBits -- which no frame passes
struct Plan {
  uint64_t meta, lens, cnt, bits;                        // where each part begins
  uint64_t lens_stride, cnt_stride;                      // words per frame
  uint64_t bits_stride;                                  // bytes per frame, a multiple of 16
  uint64_t bytes;
};
constexpr int kMetaWords = 4;                            // bits, U, refused, FF bytes

ACX_HD void make_plan(const Geo& g, uint64_t B, Plan* p) {
  const uint64_t maxU = ((uint64_t)g.nb * kMaxBlockBits + 7u) / 8u;
  p->lens_stride = ((uint64_t)g.nb + 3u) & ~3ull;
  p->cnt_stride = ((maxU + kChunkBytes - 1u) / kChunkBytes + 3u) & ~3ull;
  p->bits_stride = ((maxU + 15u) & ~15ull) + 16u;
  p->meta = 0;
  p->lens = (B * kMetaWords * 4u + 255u) & ~255ull;
  p->cnt = p->lens + B * p->lens_stride * 4u;
  p->bits = p->cnt + B * p->cnt_stride * 4u;
  p->bytes = p->bits + B * p->bits_stride;
}

}  // namespace acx_jenc

#endif  // ACX_JPEG_ENC_DEV_H_
