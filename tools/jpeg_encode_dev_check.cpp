// Stand-alone check of the device JPEG entropy ENCODER's text (anomalyclip_amd/csrc/acx_jpeg_enc_dev.h) for a sanitizer build, on
// the CPU:
//
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_encode_dev_check.cpp -o jpeg_encode_dev_check
//   ./jpeg_encode_dev_check
//
// It needs no file.  The four phases -- count, scan, write, stuff -- run as loops over the lanes the kernels of acx_jpeg_enc.hip
// give them to, in an order that is NOT the scan's (the write pass from the last block to the first: the merged words must not
// depend on it), from heap buffers of EXACTLY the bytes each phase may touch, so a word or a byte past them is the sanitizer's to
// report.  The file must equal acx_jpeg::entropy_encode's byte by byte, with `cap` exact and one byte short (ACX_E_WORKSPACE, the
// needed size still reported, the first cap bytes written); a frame the tables cannot code must be refused as that function
// refuses it.  The scan-order map is compared with the loop nest of entropy_encode.  Exit status 0: every case held.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../anomalyclip_amd/csrc/acx_jpeg_enc_dev.h"

namespace J = acx_jenc;

static int failures = 0;

static void check(bool ok, const char* what, int H, int W, const char* name) {
  if (!ok) {
    fprintf(stderr, "%dx%d %s: %s\n", W, H, name, what);
    ++failures;
  }
}

// the frame's string: exactly the words of its U bytes
struct HostMem {
  uint32_t* words;
  void store(uint32_t w, uint32_t v) const { words[w] = __builtin_bswap32(v); }
  void merge(uint32_t w, uint32_t v) const { words[w] |= __builtin_bswap32(v); }
};

// -> the frame's status; *need: the size its file needs (0 for a refused frame); dst[cap] receives the file
static int encode_emulated(const std::vector<int16_t>& coef, const uint8_t* header, int header_bytes, const J::Geo& g, uint8_t* dst,
                           int64_t cap, int64_t* need) {
  const J::Tabs tabs = J::kTabs;
  // count
  uint32_t* lens = (uint32_t*)malloc(sizeof(uint32_t) * g.nb);
  for (uint32_t s = g.nb; s-- > 0;) lens[s] = J::count_lane(g, coef.data(), s, &tabs);
  // scan
  uint32_t bits = 0, refused = 0;
  for (uint32_t s = 0; s < g.nb; ++s) {
    const uint32_t v = lens[s] & ~J::kErrBit;
    refused |= lens[s] & J::kErrBit;
    if (v > (uint32_t)J::kMaxBlockBits) ++failures;
    lens[s] = bits;
    bits += v;
  }
  const uint32_t U = J::scan_bytes(bits), nwords = (U + 3) / 4, nch = J::chunks_of(U);
  // write, the last block first
  uint32_t* words = (uint32_t*)calloc(nwords ? nwords : 1, sizeof(uint32_t));
  const HostMem mem = {words};
  for (uint32_t s = g.nb; s-- > 0;) J::write_lane(g, coef.data(), s, lens[s], &tabs, mem);
  free(lens);
  // stuff: the FF bytes of every chunk, their exclusive sums, the bytes
  uint32_t* cnt = (uint32_t*)malloc(sizeof(uint32_t) * (nch ? nch : 1));
  for (uint32_t c = 0; c < nch; ++c) {
    uint32_t n = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint32_t byte0 = c * J::kChunkBytes + lane * 4;
      n += J::ff_count(byte0 < U ? words[byte0 >> 2] : 0u, byte0, U);
    }
    cnt[c] = n;
  }
  uint32_t ff = 0;
  for (uint32_t c = 0; c < nch; ++c) {
    const uint32_t n = cnt[c];
    cnt[c] = ff;
    ff += n;
  }
  int status = ACX_OK;
  *need = 0;
  if (refused) {
    status = ACX_E_BADARG;
  } else {
    *need = J::file_bytes(header_bytes, U, ff);
    if (*need > cap) status = ACX_E_WORKSPACE;
    for (int64_t i = 0; i < header_bytes && i < cap; ++i) dst[i] = header[i];
    for (int k = 0; k < 2; ++k) {
      const int64_t at = (int64_t)header_bytes + U + ff + k;
      if (at < cap) dst[at] = k ? 0xD9 : 0xFF;
    }
    for (uint32_t c = nch; c-- > 0;) {
      uint32_t before = cnt[c];
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint32_t byte0 = c * J::kChunkBytes + lane * 4;
        const uint32_t w = byte0 < U ? words[byte0 >> 2] : 0u;
        J::emit_word(w, byte0, U, (int64_t)header_bytes + byte0 + before, dst, cap);
        before += J::ff_count(w, byte0, U);
      }
    }
  }
  free(cnt);
  free(words);
  return status;
}

static void compare(const std::vector<int16_t>& coef, const uint16_t* qt, int H, int W, const char* name, bool* stuffed) {
  J::Geo g;
  check(J::make_geo(H, W, &g) && J::coef_elems(g) == coef.size(), "geometry", H, W, name);
  uint8_t header[acx_jpeg::kHeaderBytes];
  check(acx_jpeg::encode_header(qt, H, W, header, sizeof(header)) == acx_jpeg::kHeaderBytes, "header", H, W, name);
  check(acx_jpeg::encode_header(qt, H, W, header, sizeof(header) - 1) == ACX_E_WORKSPACE, "header one byte short", H, W, name);
  std::vector<uint8_t> want((size_t)acx_jpeg::encode_bound(H, W));
  const int64_t n = acx_jpeg::entropy_encode(coef.data(), coef.size(), qt, H, W, want.data(), want.size());
  check(n > acx_jpeg::kHeaderBytes, "the host coder failed", H, W, name);
  if (n <= 0) return;
  check(memcmp(want.data(), header, sizeof(header)) == 0, "the header is not the file's prefix", H, W, name);
  int64_t need = -1;
  uint8_t* exact = (uint8_t*)malloc((size_t)n);                    // exactly n bytes
  check(encode_emulated(coef, header, sizeof(header), g, exact, n, &need) == ACX_OK, "exact-size slot refused", H, W, name);
  check(need == n, "the size differs from the host coder's", H, W, name);
  check(memcmp(exact, want.data(), (size_t)n) == 0, "the bytes differ from the host coder's", H, W, name);
  for (int64_t i = acx_jpeg::kHeaderBytes; i + 1 < n - 2; ++i)
    if (exact[i] == 0xFF && exact[i + 1] == 0) *stuffed = true;
  free(exact);
  uint8_t* small = (uint8_t*)malloc((size_t)n - 1);                // one byte short
  need = -1;
  check(encode_emulated(coef, header, sizeof(header), g, small, n - 1, &need) == ACX_E_WORKSPACE, "no ACX_E_WORKSPACE", H, W, name);
  check(need == n, "the needed size of a slot too small", H, W, name);
  check(memcmp(small, want.data(), (size_t)n - 1) == 0, "the first cap bytes of a slot too small", H, W, name);
  free(small);
  uint8_t* tiny = (uint8_t*)malloc(1);                             // not even the header
  check(encode_emulated(coef, header, sizeof(header), g, tiny, 1, &need) == ACX_E_WORKSPACE && need == n, "slot of one byte", H, W, name);
  free(tiny);
}

static void refused(const std::vector<int16_t>& coef, const uint16_t* qt, int H, int W, const char* name) {
  J::Geo g;
  check(J::make_geo(H, W, &g), "geometry", H, W, name);
  uint8_t header[acx_jpeg::kHeaderBytes];
  acx_jpeg::encode_header(qt, H, W, header, sizeof(header));
  std::vector<uint8_t> buf((size_t)acx_jpeg::encode_bound(H, W));
  check(acx_jpeg::entropy_encode(coef.data(), coef.size(), qt, H, W, buf.data(), buf.size()) == ACX_E_BADARG, "the host coder accepts it", H, W, name);
  int64_t need = -1;
  uint8_t* slot = (uint8_t*)malloc(16);
  check(encode_emulated(coef, header, sizeof(header), g, slot, 16, &need) == ACX_E_BADARG && need == 0, "accepted", H, W, name);
  free(slot);
}

// block s of the scan is the s-th block entropy_encode's loop nest visits, its predecessor the block whose DC that loop predicts from
static void scan_order(int H, int W) {
  J::Geo g;
  check(J::make_geo(H, W, &g), "geometry", H, W, "scan order");
  acx_jpeg_info o;
  memset(&o, 0, sizeof(o));
  o.width = W;
  o.height = H;
  o.ncomp = 3;
  o.comp_h[0] = o.comp_v[0] = o.hmax = o.vmax = 2;
  o.comp_h[1] = o.comp_v[1] = o.comp_h[2] = o.comp_v[2] = 1;
  acx_jpeg::layout(&o);
  check((uint64_t)o.coef_elems == J::coef_elems(g), "coef_elems", H, W, "scan order");
  uint32_t s = 0;
  int64_t last[3] = {-1, -1, -1};
  bool ok = true;
  for (int my = 0; my < o.mcus_y; ++my)
    for (int mx = 0; mx < o.mcus_x; ++mx)
      for (int c = 0; c < 3; ++c)
        for (int v = 0; v < o.comp_v[c]; ++v)
          for (int h = 0; h < o.comp_h[c]; ++h, ++s) {
            const int64_t by = (int64_t)my * o.comp_v[c] + v, bx = (int64_t)mx * o.comp_h[c] + h;
            uint32_t comp = 9;
            ok = ok && (int64_t)J::block_offset(g, s, &comp) == o.coef_offset[c] + (by * o.blocks_wide[c] + bx) * 64;
            ok = ok && comp == (uint32_t)c && J::scan_index(g, comp, (uint32_t)by, (uint32_t)bx) == s && J::block_pred(s) == last[c];
            last[c] = s;
          }
  check(ok && s == g.nb, "the map differs from the host coder's loop nest", H, W, "scan order");
}

// a block of kMaxBlockBits bits where its DC difference has category 11: every AC +-1023, the DC `dc`
static void maximal(int16_t* blk, int dc) {
  blk[0] = (int16_t)dc;
  for (int k = 1; k < 64; ++k) blk[k] = (int16_t)((k & 1) ? -1023 : 1023);
}

int main() {
  uint16_t qt[128];
  for (int i = 0; i < 128; ++i) qt[i] = (uint16_t)(1 + (i * 7) % 255);
  // the tables are the ones the host coder derives
  {
    const uint8_t* hbits[4] = {acx_jpeg::kDcLumaBits, acx_jpeg::kAcLumaBits, acx_jpeg::kDcChromaBits, acx_jpeg::kAcChromaBits};
    const uint8_t* hvals[4] = {acx_jpeg::kDcVals, acx_jpeg::kAcLumaVals, acx_jpeg::kDcVals, acx_jpeg::kAcChromaVals};
    const uint32_t* mine[4] = {J::kTabs.dc[0], J::kTabs.ac[0], J::kTabs.dc[1], J::kTabs.ac[1]};
    for (int t = 0; t < 4; ++t) {
      acx_jpeg::EncTable e;
      acx_jpeg::enc_derive(hbits[t], hvals[t], &e);
      for (int sym = 0; sym < ((t & 1) ? 256 : 16); ++sym)
        check(mine[t][sym] == (((uint32_t)e.len[sym] << 16) | e.code[sym]), "a table entry differs", 0, 0, "tables");
    }
  }
  // sizes the entry must refuse, and the largest it takes
  {
    J::Geo g;
    check(!J::make_geo(0, 16, &g) && !J::make_geo(16, 65536, &g) && !J::make_geo(65535, 65535, &g), "a size accepted", 0, 0, "geometry");
    check(J::make_geo(65535, 832, &g) && (int64_t)g.nb * J::kMaxBlockBits <= J::kMaxFrameBits, "832 x 65535 refused", 0, 0, "geometry");
    check(!J::make_geo(65535, 833, &g), "833 x 65535 accepted", 0, 0, "geometry");
    J::Plan p;
    J::make_geo(800, 1200, &g);
    J::make_plan(g, 32, &p);
    const uint64_t maxU = ((uint64_t)g.nb * J::kMaxBlockBits + 7) / 8;
    check(p.bits_stride % 16 == 0 && p.bits_stride >= ((maxU + 15) & ~15ull) + 16 && p.cnt_stride >= J::chunks_of((uint32_t)maxU) &&
              p.lens_stride >= g.nb && p.lens % 16 == 0 && p.cnt % 16 == 0 && p.bits % 16 == 0 && p.lens >= 32 * 16 &&
              p.bytes == p.bits + 32 * p.bits_stride,
          "the workspace plan", 800, 1200, "geometry");
  }
  const int sizes[4][2] = {{16, 16}, {32, 48}, {33, 47}, {176, 208}};
  // the edge blocks of tools/jpeg_encode_check.cpp
  std::vector<std::vector<int16_t>> edges;
  {
    std::vector<int16_t> b(64, 0);
    b[J::kNat[63]] = 5;
    edges.push_back(b);
    for (int run = 16; run <= 62; ++run) {
      std::vector<int16_t> z(64, 0);
      z[J::kNat[run + 1]] = (int16_t)((run & 1) ? -3 : 7);
      edges.push_back(z);
    }
    for (int v = -1023; v <= 1023; v += 2046) {
      std::vector<int16_t> a(64, 0);
      a[J::kNat[1]] = (int16_t)v;
      a[J::kNat[40]] = (int16_t)-v;
      a[J::kNat[63]] = (int16_t)v;
      edges.push_back(a);
    }
  }
  bool stuffed = false;
  for (const auto& hw : sizes) {
    const int H = hw[0], W = hw[1];
    scan_order(H, W);
    const size_t nb = (size_t)((W + 15) / 16) * ((H + 15) / 16) * 6, n = nb * 64;
    compare(std::vector<int16_t>(n, 0), qt, H, W, "all zero", &stuffed);
    for (size_t k = 0; k < edges.size(); k += nb) {
      std::vector<int16_t> c(n, 0);
      for (size_t j = 0; j < nb && k + j < edges.size(); ++j) memcpy(&c[j * 64], edges[k + j].data(), 128);
      compare(c, qt, H, W, "edge blocks", &stuffed);
    }
    std::vector<int16_t> dc(n, 0);
    for (size_t j = 0; j < nb; ++j) dc[j * 64] = (int16_t)((j & 1) ? -1023 : 1023);
    compare(dc, qt, H, W, "DC differences of category 11", &stuffed);
    std::vector<int16_t> dense(n), sparse(n, 0);
    uint32_t seed = 99u + (uint32_t)H;
    for (size_t i = 0; i < n; ++i) {
      seed = seed * 1664525u + 1013904223u;
      dense[i] = (int16_t)((int)((seed >> 8) % 2047u) - 1023);
      if ((seed >> 24) < 26u) sparse[i] = (int16_t)((int)((seed >> 4) % 81u) - 40);
    }
    compare(dense, qt, H, W, "dense random", &stuffed);
    compare(sparse, qt, H, W, "sparse random", &stuffed);
    // blocks of kMaxBlockBits bits, alone and between blocks of 6 and 4 bits
    std::vector<int16_t> big(n), mixed(n, 0);
    {
      J::Geo g;
      J::make_geo(H, W, &g);
      int sign[3] = {1, 1, 1};
      for (uint32_t b = 0; b < g.nb; ++b) {                          // in scan order: the DC alternates within each component
        uint32_t c;
        const uint32_t off = J::block_offset(g, b, &c);
        maximal(&big[off], 1023 * sign[c]);
        if (b & 1) maximal(&mixed[off], 1023 * sign[c]);
        sign[c] = -sign[c];
      }
    }
    compare(big, qt, H, W, "maximal blocks", &stuffed);
    compare(mixed, qt, H, W, "zero and maximal blocks", &stuffed);
    // values the tables cannot code are refused, not coded wrongly
    std::vector<int16_t> bad(sparse);
    bad[n - 64 + 5] = 1024;
    refused(bad, qt, H, W, "AC 1024");
    bad[n - 64 + 5] = -1024;
    refused(bad, qt, H, W, "AC -1024");
    bad = sparse;
    bad[0] = -2047;
    bad[64] = 2047;
    refused(bad, qt, H, W, "DC difference of category 12");
    bad = sparse;
    bad[0] = -32768;
    bad[64] = 32767;
    bad[70] = -32768;
    refused(bad, qt, H, W, "the ends of int16");
  }
  if (!stuffed) {
    fprintf(stderr, "no case produced an FF byte in its scan\n");
    ++failures;
  }
  printf("jpeg_encode_dev_check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
