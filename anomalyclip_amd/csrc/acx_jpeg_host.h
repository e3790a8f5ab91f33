// Host half of the baseline JPEG decoder: marker parsing and Huffman (entropy) decoding into de-zigzagged, NOT dequantised
// coefficient blocks.  Plain C++ without HIP: the library pulls it in through acx_jpeg.hip, tools/jpeg_host_check.cpp compiles it
// alone under the sanitizers.  The input is untrusted: every read is checked against the end of the file, every table index against
// what DHT / DQT declared, every write against the caller's buffer; a malformed file ends in an error code.  Re-entrant: no global
// state, no allocation (the derived Huffman tables live on the caller's stack).
#ifndef ACX_JPEG_HOST_H_
#define ACX_JPEG_HOST_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/acx.h"

namespace acx_jpeg {

// zigzag position -> natural (row-major) position of a coefficient
static const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// the geometry every other field follows from: component sizes, block grids padded to whole MCUs, coefficient offsets
static inline void layout(acx_jpeg_info* o) {
  o->mcus_x = (o->width + 8 * o->hmax - 1) / (8 * o->hmax);
  o->mcus_y = (o->height + 8 * o->vmax - 1) / (8 * o->vmax);
  int64_t off = 0;
  for (int c = 0; c < o->ncomp; ++c) {
    o->comp_width[c] = (o->width * o->comp_h[c] + o->hmax - 1) / o->hmax;
    o->comp_height[c] = (o->height * o->comp_v[c] + o->vmax - 1) / o->vmax;
    o->blocks_wide[c] = o->mcus_x * o->comp_h[c];
    o->blocks_high[c] = o->mcus_y * o->comp_v[c];
    o->coef_offset[c] = off;
    off += (int64_t)o->blocks_wide[c] * o->blocks_high[c] * 64;
  }
  o->coef_elems = off;
}

static inline int parse(const uint8_t* d, size_t n, acx_jpeg_info* o) {
  if (!d || !o) return ACX_E_BADARG;
  memset(o, 0, sizeof(*o));
  if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return ACX_E_BADARG;
  size_t p = 2;
  bool have_sof = false, jfif = false;
  int adobe = -1, comp_id[4] = {0, 0, 0, 0};
  for (;;) {
    if (p + 2 > n) return ACX_E_BADARG;
    if (d[p] != 0xFF) return ACX_E_BADARG;
    while (p < n && d[p] == 0xFF) ++p;                  // fill bytes before a marker
    if (p >= n) return ACX_E_BADARG;
    const int m = d[p++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // markers without a segment
    if (m == 0xD9 || m == 0xD8 || m == 0x00) return ACX_E_BADARG;
    if (p + 2 > n) return ACX_E_BADARG;
    const size_t len = (size_t)be16(d + p);
    if (len < 2 || p + len > n) return ACX_E_BADARG;
    const uint8_t* s = d + p + 2;
    const size_t sl = len - 2;
    if (m == 0xC0 || m == 0xC1) {                        // baseline / extended sequential, Huffman
      if (have_sof || sl < 6) return ACX_E_BADARG;
      if (s[0] != 8) return ACX_E_UNSUPPORTED;           // 12-bit samples
      o->height = be16(s + 1);
      o->width = be16(s + 3);
      o->ncomp = s[5];
      if (o->height == 0) return ACX_E_UNSUPPORTED;      // the height comes in a DNL segment
      if (o->width == 0) return ACX_E_BADARG;
      if (o->ncomp != 1 && o->ncomp != 3) return o->ncomp == 0 ? ACX_E_BADARG : ACX_E_UNSUPPORTED;
      if (sl != 6 + 3 * (size_t)o->ncomp) return ACX_E_BADARG;
      for (int c = 0; c < o->ncomp; ++c) {
        comp_id[c] = s[6 + 3 * c];
        o->comp_h[c] = s[7 + 3 * c] >> 4;
        o->comp_v[c] = s[7 + 3 * c] & 15;
        o->comp_tq[c] = s[8 + 3 * c];
        if (o->comp_h[c] < 1 || o->comp_h[c] > 4 || o->comp_v[c] < 1 || o->comp_v[c] > 4 || o->comp_tq[c] > 3) return ACX_E_BADARG;
      }
      if (o->ncomp == 1) {
        o->comp_h[0] = o->comp_v[0] = 1;                 // a single-component scan is one block per MCU, whatever the factors say
      } else {
        if (o->comp_h[1] != 1 || o->comp_v[1] != 1 || o->comp_h[2] != 1 || o->comp_v[2] != 1) return ACX_E_UNSUPPORTED;
        const int hv = o->comp_h[0] * 16 + o->comp_v[0];
        if (hv != 0x11 && hv != 0x21 && hv != 0x22) return ACX_E_UNSUPPORTED;
        // libjpeg upsamples a chroma plane of one or two samples per row by replication, not with the triangle filter
        if (o->comp_h[0] == 2 && (o->width + 1) / 2 <= 2) return ACX_E_UNSUPPORTED;
      }
      o->hmax = o->comp_h[0];
      o->vmax = o->comp_v[0];
      layout(o);
      have_sof = true;
    } else if (m == 0xC4) {                              // DHT
      size_t q = 0;
      while (q < sl) {
        if (q + 17 > sl) return ACX_E_BADARG;
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 3) return ACX_E_BADARG;
        size_t cnt = 0;
        for (int i = 1; i <= 16; ++i) cnt += s[q + i];
        if (cnt > 256 || q + 17 + cnt > sl) return ACX_E_BADARG;
        o->huff_bits[tc][th][0] = 0;
        memcpy(&o->huff_bits[tc][th][1], s + q + 1, 16);
        memset(o->huff_vals[tc][th], 0, 256);
        memcpy(o->huff_vals[tc][th], s + q + 17, cnt);
        o->huff_present[tc][th] = 1;
        q += 17 + cnt;
      }
    } else if (m == 0xDB) {                              // DQT: entries in zigzag order, stored in natural order
      size_t q = 0;
      while (q < sl) {
        const int pq = s[q] >> 4, tq = s[q] & 15;
        if (pq > 1 || tq > 3) return ACX_E_BADARG;
        const size_t need = 1 + (pq ? 128 : 64);
        if (q + need > sl) return ACX_E_BADARG;
        for (int k = 0; k < 64; ++k)
          o->qtab[tq][kNatural[k]] = (uint16_t)(pq ? be16(s + q + 1 + 2 * k) : s[q + 1 + k]);
        o->qtab_present[tq] = 1;
        q += need;
      }
    } else if (m == 0xDD) {                              // DRI
      if (sl != 2) return ACX_E_BADARG;
      o->restart_interval = be16(s);
    } else if (m == 0xDA) {                              // SOS
      if (!have_sof || sl < 1) return ACX_E_BADARG;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || sl != 4 + 2 * (size_t)ns) return ACX_E_BADARG;
      if (ns != o->ncomp) return ACX_E_UNSUPPORTED;      // several scans
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != comp_id[c]) return ACX_E_UNSUPPORTED;
        o->comp_td[c] = s[2 + 2 * c] >> 4;
        o->comp_ta[c] = s[2 + 2 * c] & 15;
        if (o->comp_td[c] > 3 || o->comp_ta[c] > 3) return ACX_E_BADARG;
        if (!o->huff_present[0][o->comp_td[c]] || !o->huff_present[1][o->comp_ta[c]] || !o->qtab_present[o->comp_tq[c]])
          return ACX_E_BADARG;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return ACX_E_UNSUPPORTED;
      if (o->ncomp == 3) {                               // read as YCbCr only where libjpeg would
        if (!jfif && adobe >= 0 && adobe != 1) return ACX_E_UNSUPPORTED;
        if (adobe == 0 || adobe == 2) return ACX_E_UNSUPPORTED;
        if (!jfif && adobe < 0 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return ACX_E_UNSUPPORTED;
      }
      o->scan_offset = (int64_t)(p + len);
      return ACX_OK;
    } else if (m == 0xE0) {
      if (sl >= 5 && !memcmp(s, "JFIF", 5)) jfif = true;
    } else if (m == 0xEE) {
      if (sl >= 12 && !memcmp(s, "Adobe", 5)) adobe = s[11];
    } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {
      // APPn / COM: skipped
    } else if (m == 0xDC) {
      return ACX_E_UNSUPPORTED;                          // DNL
    } else if (m >= 0xC2 && m <= 0xCF) {
      return ACX_E_UNSUPPORTED;                          // progressive, lossless, hierarchical, arithmetic coding (SOFn, DAC, JPG)
    } else {
      return ACX_E_UNSUPPORTED;
    }
    p += len;
  }
}

// one Huffman table as the decoder reads it: a 9-bit lookahead (length << 8 | symbol, 0: longer than 9 bits) and, for the long
// codes, the largest code of each length with the offset of its symbols
constexpr int kLook = 9;
struct HuffTable {
  uint16_t look[1 << kLook];
  int32_t maxcode[18];
  int32_t valoff[17];
  int nvals;
  const uint8_t* vals;
};

static inline int derive(const uint8_t* bits, const uint8_t* vals, HuffTable* t) {
  uint8_t size[257];
  uint32_t code[256];
  int n = 0;
  for (int l = 1; l <= 16; ++l) {
    if (n + bits[l] > 256) return ACX_E_BADARG;
    for (int i = 0; i < bits[l]; ++i) size[n++] = (uint8_t)l;
  }
  size[n] = 0;
  t->nvals = n;
  t->vals = vals;
  uint32_t c = 0;
  int si = size[0], k = 0;
  while (size[k]) {
    while (size[k] == si) code[k++] = c++;
    if (c > (1u << si)) return ACX_E_BADARG;             // more codes of a length than the length has
    c <<= 1;
    ++si;
  }
  k = 0;
  for (int l = 1; l <= 16; ++l) {
    if (bits[l]) {
      t->valoff[l] = k - (int32_t)code[k];
      k += bits[l];
      t->maxcode[l] = (int32_t)code[k - 1];
    } else {
      t->maxcode[l] = -1;
      t->valoff[l] = 0;
    }
  }
  t->maxcode[17] = 0x7FFFFFFF;
  memset(t->look, 0, sizeof(t->look));
  k = 0;
  for (int l = 1; l <= kLook; ++l)
    for (int i = 0; i < bits[l]; ++i, ++k) {
      const uint32_t first = code[k] << (kLook - l);
      for (uint32_t j = 0; j < (1u << (kLook - l)); ++j) t->look[first + j] = (uint16_t)((l << 8) | vals[k]);
    }
  return ACX_OK;
}

// The entropy-coded segment as a stream of bits, most significant first.  `buf` holds `bits` valid bits at its top.  FF 00 is the
// byte FF; at a marker or at the end of the file the reader feeds zero bits and counts them in `fake`: they always sit at the tail
// of the buffer, so the stream was overrun exactly when fewer than `fake` bits are left.
struct BitReader {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t buf;
  int bits;
  int fake;
  int marker;      // the marker the reader stopped at (0: none yet)

  inline void fill() {
    while (bits <= 56) {
      uint64_t b = 0;
      if (marker == 0 && p < end) {
        b = *p;
        if (b != 0xFF) {
          ++p;
        } else if (p + 1 >= end) {
          p = end;
          marker = 0xD9;                                 // a lone FF at the end: the stream is over
          b = 0;
          fake += 8;
        } else if (p[1] == 0) {
          p += 2;
        } else if (p[1] == 0xFF) {
          ++p;                                           // a fill byte
          continue;
        } else {
          marker = p[1];
          p += 2;
          b = 0;
          fake += 8;
        }
      } else {
        if (marker == 0) marker = 0xD9;
        fake += 8;
      }
      buf |= b << (56 - bits);
      bits += 8;
    }
  }
  inline bool overrun() const { return bits < fake; }
  inline uint32_t peek(int n) const { return (uint32_t)(buf >> (64 - n)); }
  inline void drop(int n) {
    buf <<= n;
    bits -= n;
  }
};

// the next symbol of table t, or -1
static inline int decode_symbol(BitReader& br, const HuffTable& t) {
  const uint32_t e = t.look[br.peek(kLook)];
  if (e) {
    br.drop((int)(e >> 8));
    return (int)(e & 255);
  }
  const int32_t v = (int32_t)br.peek(16);
  int l = kLook + 1;
  while (l <= 16 && (v >> (16 - l)) > t.maxcode[l]) ++l;
  if (l > 16) return -1;
  const int idx = (v >> (16 - l)) + t.valoff[l];
  if (idx < 0 || idx >= t.nvals) return -1;
  br.drop(l);
  return t.vals[idx];
}

// the s-bit value that follows a symbol, sign-extended the JPEG way (s in 1 .. 15)
static inline int receive_extend(BitReader& br, int s) {
  const int v = (int)br.peek(s);
  br.drop(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

static inline int entropy_decode(const uint8_t* d, size_t n, const acx_jpeg_info* o, int16_t* coef, size_t coef_elems) {
  if (!d || !o || !coef) return ACX_E_BADARG;
  if (o->ncomp != 1 && o->ncomp != 3) return ACX_E_BADARG;
  if (o->scan_offset < 2 || (uint64_t)o->scan_offset > n) return ACX_E_BADARG;
  acx_jpeg_info g;                                       // the layout is recomputed from the sizes: `o` came through a caller
  memset(&g, 0, sizeof(g));
  g.width = o->width;
  g.height = o->height;
  g.ncomp = o->ncomp;
  if (g.width < 1 || g.width > 65535 || g.height < 1 || g.height > 65535) return ACX_E_BADARG;
  for (int c = 0; c < g.ncomp; ++c) {
    g.comp_h[c] = o->comp_h[c];
    g.comp_v[c] = o->comp_v[c];
    if (g.comp_h[c] < 1 || g.comp_h[c] > 2 || g.comp_v[c] < 1 || g.comp_v[c] > 2) return ACX_E_BADARG;
    if (c > 0 && (g.comp_h[c] != 1 || g.comp_v[c] != 1)) return ACX_E_BADARG;
    if ((unsigned)o->comp_td[c] > 3 || (unsigned)o->comp_ta[c] > 3) return ACX_E_BADARG;
    if (!o->huff_present[0][o->comp_td[c]] || !o->huff_present[1][o->comp_ta[c]]) return ACX_E_BADARG;
  }
  if (g.ncomp == 1 && (g.comp_h[0] != 1 || g.comp_v[0] != 1)) return ACX_E_BADARG;
  g.hmax = g.comp_h[0];
  g.vmax = g.comp_v[0];
  layout(&g);
  if ((uint64_t)g.coef_elems > coef_elems) return ACX_E_BADARG;

  HuffTable tab[2][4];
  bool built[2][4] = {{false, false, false, false}, {false, false, false, false}};
  for (int c = 0; c < g.ncomp; ++c) {
    const int idx[2] = {o->comp_td[c], o->comp_ta[c]};
    for (int k = 0; k < 2; ++k)
      if (!built[k][idx[k]]) {
        const int rc = derive(o->huff_bits[k][idx[k]], o->huff_vals[k][idx[k]], &tab[k][idx[k]]);
        if (rc != ACX_OK) return rc;
        built[k][idx[k]] = true;
      }
  }

  BitReader br;
  br.p = d + o->scan_offset;
  br.end = d + n;
  br.buf = 0;
  br.bits = br.fake = br.marker = 0;
  int pred[4] = {0, 0, 0, 0};
  const int ri = o->restart_interval;
  int togo = ri, next_rst = 0;
  for (int my = 0; my < g.mcus_y; ++my) {
    for (int mx = 0; mx < g.mcus_x; ++mx) {
      if (ri > 0 && togo == 0) {                         // a restart marker: byte-align, reset the predictors
        if (br.overrun()) return ACX_E_BADARG;
        if (br.marker == 0) {                            // not reached by the look-ahead: it must come next
          const uint8_t* q = br.p;
          while (q + 1 < br.end && q[0] == 0xFF && q[1] == 0xFF) ++q;
          if (q + 2 > br.end || q[0] != 0xFF) return ACX_E_BADARG;
          br.marker = q[1];
          br.p = q + 2;
        }
        if (br.marker != 0xD0 + next_rst) return ACX_E_BADARG;
        next_rst = (next_rst + 1) & 7;
        br.buf = 0;
        br.bits = br.fake = br.marker = 0;
        pred[0] = pred[1] = pred[2] = pred[3] = 0;
        togo = ri;
      }
      for (int c = 0; c < g.ncomp; ++c) {
        const HuffTable& dc = tab[0][o->comp_td[c]];
        const HuffTable& ac = tab[1][o->comp_ta[c]];
        for (int v = 0; v < g.comp_v[c]; ++v)
          for (int h = 0; h < g.comp_h[c]; ++h) {
            const int64_t by = (int64_t)my * g.comp_v[c] + v, bx = (int64_t)mx * g.comp_h[c] + h;
            const int64_t base = g.coef_offset[c] + (by * g.blocks_wide[c] + bx) * 64;
            if (base < 0 || (uint64_t)base + 64 > coef_elems) return ACX_E_BADARG;
            int16_t* blk = coef + base;
            if (br.bits < 32) br.fill();
            int s = decode_symbol(br, dc);
            if (s < 0 || s > 15) return ACX_E_BADARG;
            if (s) pred[c] = (int16_t)(pred[c] + receive_extend(br, s));
            blk[0] = (int16_t)pred[c];
            for (int k = 1; k < 64;) {
              if (br.bits < 32) br.fill();
              const int rs = decode_symbol(br, ac);
              if (rs < 0) return ACX_E_BADARG;
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;                      // end of block
                k += 16;
                continue;
              }
              k += r;
              if (k > 63) return ACX_E_BADARG;
              blk[kNatural[k]] = (int16_t)receive_extend(br, s);
              ++k;
            }
          }
      }
      if (br.overrun()) return ACX_E_BADARG;             // the stream ended inside this MCU
      --togo;
    }
  }
  return ACX_OK;
}

// The scan un-stuffed for the device decoder: the bytes BitReader::fill would feed, in its order -- FF 00 is FF, an FF before an FF
// is a fill byte, anything else after an FF (or an FF that ends the file) ends the stream -- then zero bytes up to a multiple of
// ACX_JPEG_SCAN_ALIGN.  A restart interval is left to entropy_decode.
static inline int scan_pack(const uint8_t* d, size_t n, const acx_jpeg_info* o, uint8_t* dst, size_t cap, int64_t* payload,
                            acx_jpeg_huff* huff) {
  if (!d || !o || !dst || !payload) return ACX_E_BADARG;
  *payload = 0;
  if (o->ncomp != 1 && o->ncomp != 3) return ACX_E_BADARG;
  if (o->scan_offset < 2 || (uint64_t)o->scan_offset > n) return ACX_E_BADARG;
  for (int c = 0; c < o->ncomp; ++c) {
    if ((unsigned)o->comp_td[c] > 3 || (unsigned)o->comp_ta[c] > 3) return ACX_E_BADARG;
    if (!o->huff_present[0][o->comp_td[c]] || !o->huff_present[1][o->comp_ta[c]]) return ACX_E_BADARG;
  }
  if (o->restart_interval != 0) return ACX_E_UNSUPPORTED;
  size_t p = (size_t)o->scan_offset, len = 0;
  while (p < n) {
    const uint8_t b = d[p];
    if (b != 0xFF) {
      ++p;
    } else if (p + 1 >= n) {
      break;                                             // a lone FF at the end
    } else if (d[p + 1] == 0) {
      p += 2;
    } else if (d[p + 1] == 0xFF) {
      ++p;                                               // a fill byte
      continue;
    } else {
      break;                                             // a marker
    }
    if (len >= cap) return ACX_E_BADARG;
    dst[len++] = b;
  }
  const size_t padded = (len + ACX_JPEG_SCAN_ALIGN - 1) / ACX_JPEG_SCAN_ALIGN * ACX_JPEG_SCAN_ALIGN;
  if (padded > cap) return ACX_E_BADARG;
  memset(dst + len, 0, padded - len);
  *payload = (int64_t)len;
  if (huff) {
    memset(huff, 0, sizeof(*huff));
    memcpy(huff->present, o->huff_present, sizeof(huff->present));
    memcpy(huff->bits, o->huff_bits, sizeof(huff->bits));
    memcpy(huff->vals, o->huff_vals, sizeof(huff->vals));
    for (int c = 0; c < o->ncomp; ++c) {
      huff->td[c] = (uint8_t)o->comp_td[c];
      huff->ta[c] = (uint8_t)o->comp_ta[c];
    }
  }
  return ACX_OK;
}

}  // namespace acx_jpeg

#endif  // ACX_JPEG_HOST_H_
