// Host half of the baseline JPEG ENCODER: one frame's quantised coefficient blocks (the layout acx_jpeg_host.h's entropy_decode
// writes: natural order, component after component, 4:2:0) -> a complete JFIF file.  Plain C++ without HIP: the library pulls it
// in through acx_viz.hip, tools/jpeg_encode_check.cpp compiles it alone under the sanitizers.  Every write is checked against the
// caller's buffer: a buffer too small is ACX_E_WORKSPACE with nothing written past its end.  Re-entrant: no global state, no
// allocation (the derived code tables live on the caller's stack).
#ifndef ACX_JPEG_ENC_HOST_H_
#define ACX_JPEG_ENC_HOST_H_

#include "acx_jpeg_host.h"

namespace acx_jpeg {

// ISO/IEC 10918-1 Annex K.3: the typical Huffman tables (codes of each length 1 .. 16, then the symbols)
static constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static constexpr uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static constexpr uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// a Huffman table as the encoder reads it: code and length of every symbol (length 0: the table has no code for it)
struct EncTable {
  uint16_t code[256];
  uint8_t len[256];
};

static inline void enc_derive(const uint8_t* bits16, const uint8_t* vals, EncTable* t) {
  memset(t, 0, sizeof(*t));
  uint32_t c = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits16[l - 1]; ++i, ++k) {
      t->code[vals[k]] = (uint16_t)c++;
      t->len[vals[k]] = (uint8_t)l;
    }
    c <<= 1;
  }
}

// The output: bytes into dst[cap], never past it (`n` goes on counting, so that the caller learns the size that was needed);
// put() appends the low `len` bits of `v`, most significant first, and stuffs a zero byte after every FF of the scan.
struct BitWriter {
  uint8_t* dst;
  size_t cap, n;
  uint64_t acc;
  int nbits;

  inline void byte(uint8_t b) {
    if (n < cap) dst[n] = b;
    ++n;
  }
  inline void raw(const uint8_t* p, size_t len) {
    for (size_t i = 0; i < len; ++i) byte(p[i]);
  }
  inline void be16(int v) {
    byte((uint8_t)(v >> 8));
    byte((uint8_t)v);
  }
  inline void put(uint32_t v, int len) {              // len <= 26
    acc = (acc << len) | (v & ((1u << len) - 1u));
    nbits += len;
    while (nbits >= 8) {
      const uint8_t b = (uint8_t)(acc >> (nbits - 8));
      byte(b);
      if (b == 0xFF) byte(0);
      nbits -= 8;
    }
  }
  inline void flush() {                               // the last byte is filled with one bits
    if (nbits > 0) put((1u << (8 - nbits)) - 1u, 8 - nbits);
  }
};

// the category of a value (the number of bits of its magnitude) and the bits that follow the symbol
static inline int magnitude_bits(int v, uint32_t* extra) {
  const int a = v < 0 ? -v : v;
  int s = 0;
  while ((a >> s) != 0) ++s;
  *extra = (uint32_t)(v < 0 ? v + (1 << s) - 1 : v);
  return s;
}

// a size that acx_jpeg_entropy_encode never exceeds: the headers, and per block a DC code (9 + 11 bits) and 63 AC codes of
// 16 + 10 bits, every byte of them stuffed
static inline int64_t encode_bound(int32_t H, int32_t W) {
  if (H < 1 || W < 1 || H > 65535 || W > 65535) return ACX_E_BADARG;
  const int64_t mcus = (int64_t)((W + 15) / 16) * ((H + 15) / 16);
  return 1024 + mcus * 6 * 416;
}

// what stands before the scan: APP0, two DQT (entries in zigzag order), SOF0 with luma sampling 2x2, four DHT with the Annex K
// tables, SOS -- kHeaderBytes of them for every size and every pair of tables
constexpr int kHeaderBytes = 623;
static inline void write_header(BitWriter& bw, const uint16_t* qtabs, int32_t H, int32_t W) {
  static const uint8_t app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  bw.raw(app0, sizeof(app0));
  for (int t = 0; t < 2; ++t) {                                     // DQT: entries in zigzag order
    bw.be16(0xFFDB);
    bw.be16(67);
    bw.byte((uint8_t)t);
    for (int k = 0; k < 64; ++k) bw.byte((uint8_t)qtabs[t * 64 + kNatural[k]]);
  }
  bw.be16(0xFFC0);                                                  // SOF0
  bw.be16(17);
  bw.byte(8);
  bw.be16(H);
  bw.be16(W);
  bw.byte(3);
  static const uint8_t comps[] = {1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
  bw.raw(comps, sizeof(comps));
  const uint8_t* hbits[4] = {kDcLumaBits, kAcLumaBits, kDcChromaBits, kAcChromaBits};
  const uint8_t* hvals[4] = {kDcVals, kAcLumaVals, kDcVals, kAcChromaVals};
  const uint8_t hid[4] = {0x00, 0x10, 0x01, 0x11};
  for (int t = 0; t < 4; ++t) {
    int cnt = 0;
    for (int i = 0; i < 16; ++i) cnt += hbits[t][i];
    bw.be16(0xFFC4);
    bw.be16(2 + 1 + 16 + cnt);
    bw.byte(hid[t]);
    bw.raw(hbits[t], 16);
    bw.raw(hvals[t], (size_t)cnt);
  }
  static const uint8_t sos[] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  bw.raw(sos, sizeof(sos));
}

static inline bool tables_are_baseline(const uint16_t* qtabs) {
  for (int i = 0; i < 128; ++i)
    if (qtabs[i] < 1 || qtabs[i] > 255) return false;                 // baseline: 8-bit tables
  return true;
}

// the header alone, for a coder that writes the scan elsewhere: -> kHeaderBytes, or a negative ACX_E_* code
static inline int64_t encode_header(const uint16_t* qtabs, int32_t H, int32_t W, uint8_t* dst, size_t cap) {
  if (!qtabs || (!dst && cap)) return ACX_E_BADARG;
  if (H < 1 || W < 1 || H > 65535 || W > 65535) return ACX_E_BADARG;
  if (!tables_are_baseline(qtabs)) return ACX_E_BADARG;
  BitWriter bw = {dst, cap, 0, 0, 0};
  write_header(bw, qtabs, H, W);
  if (bw.n > cap) return ACX_E_WORKSPACE;
  return (int64_t)bw.n;
}

// coef: [coef_elems] int16, the frame's blocks as entropy_decode writes them for 3 components with luma sampling 2x2;
// qtabs: [2][64] in natural order (luma, chroma), entries 1 .. 255.  -> bytes written, or a negative ACX_E_* code.
static inline int64_t entropy_encode(const int16_t* coef, size_t coef_elems, const uint16_t* qtabs, int32_t H, int32_t W, uint8_t* dst,
                                     size_t cap) {
  if (!coef || !qtabs || (!dst && cap)) return ACX_E_BADARG;
  if (H < 1 || W < 1 || H > 65535 || W > 65535) return ACX_E_BADARG;
  if (!tables_are_baseline(qtabs)) return ACX_E_BADARG;
  acx_jpeg_info g;
  memset(&g, 0, sizeof(g));
  g.width = W;
  g.height = H;
  g.ncomp = 3;
  g.comp_h[0] = g.comp_v[0] = g.hmax = g.vmax = 2;
  g.comp_h[1] = g.comp_v[1] = g.comp_h[2] = g.comp_v[2] = 1;
  layout(&g);
  if ((uint64_t)g.coef_elems != coef_elems) return ACX_E_BADARG;

  BitWriter bw = {dst, cap, 0, 0, 0};
  write_header(bw, qtabs, H, W);
  EncTable tab[4];                                                  // DC luma, AC luma, DC chroma, AC chroma
  enc_derive(kDcLumaBits, kDcVals, &tab[0]);
  enc_derive(kAcLumaBits, kAcLumaVals, &tab[1]);
  enc_derive(kDcChromaBits, kDcVals, &tab[2]);
  enc_derive(kAcChromaBits, kAcChromaVals, &tab[3]);

  int pred[3] = {0, 0, 0};
  for (int my = 0; my < g.mcus_y; ++my)
    for (int mx = 0; mx < g.mcus_x; ++mx)
      for (int c = 0; c < 3; ++c) {
        const EncTable& dc = tab[c == 0 ? 0 : 2];
        const EncTable& ac = tab[c == 0 ? 1 : 3];
        for (int v = 0; v < g.comp_v[c]; ++v)
          for (int h = 0; h < g.comp_h[c]; ++h) {
            const int64_t by = (int64_t)my * g.comp_v[c] + v, bx = (int64_t)mx * g.comp_h[c] + h;
            const int16_t* blk = coef + g.coef_offset[c] + (by * g.blocks_wide[c] + bx) * 64;
            uint32_t extra;
            int s = magnitude_bits((int)blk[0] - pred[c], &extra);
            if (s > 11) return ACX_E_BADARG;                        // a DC difference the table has no code for
            pred[c] = blk[0];
            bw.put(dc.code[s], dc.len[s]);
            if (s) bw.put(extra, s);
            int run = 0;
            for (int k = 1; k < 64; ++k) {
              const int a = blk[kNatural[k]];
              if (a == 0) {
                ++run;
                continue;
              }
              for (; run >= 16; run -= 16) bw.put(ac.code[0xF0], ac.len[0xF0]);     // ZRL
              s = magnitude_bits(a, &extra);
              if (s > 10) return ACX_E_BADARG;                      // |AC| > 1023
              const int rs = (run << 4) | s;
              bw.put(ac.code[rs], ac.len[rs]);
              bw.put(extra, s);
              run = 0;
            }
            if (run) bw.put(ac.code[0], ac.len[0]);                 // EOB (none when coefficient 63 is set)
          }
      }
  bw.flush();
  bw.nbits = 0;
  bw.be16(0xFFD9);
  if (bw.n > cap) return ACX_E_WORKSPACE;
  return (int64_t)bw.n;
}

}  // namespace acx_jpeg

#endif  // ACX_JPEG_ENC_HOST_H_
