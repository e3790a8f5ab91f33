// Stand-alone check of the host JPEG entropy ENCODER (anomalyclip_amd/csrc/acx_jpeg_enc_host.h) for a sanitizer build, on the CPU:
//
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_encode_check.cpp -o jpeg_encode_check
//   ./jpeg_encode_check
//
// It needs no file: for the sizes 16x16, 48x32 and 1200x800 it builds the coefficient frames the Huffman coder treats specially --
// all zero; a block with only coefficient 63 set (no EOB); every zero run 16 ... 62 (ZRL); AC +-1023; DC differences of category
// 11 in both signs; dense random values (FF bytes, stuffing) -- encodes each into a heap buffer of EXACTLY the bytes it needs, so a
// write one byte past it is the sanitizer's to report, and reads the file back with the project's own parser and decoder: the
// coefficients must return exactly.  A buffer one byte short must give ACX_E_WORKSPACE.  Exit status 0: every case held.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../anomalyclip_amd/csrc/acx_jpeg_enc_host.h"

static int failures = 0;

static void check(bool ok, const char* what, int H, int W, const char* name) {
  if (!ok) {
    fprintf(stderr, "%dx%d %s: %s\n", W, H, name, what);
    ++failures;
  }
}

static void round_trip(const std::vector<int16_t>& coef, const uint16_t* qt, int H, int W, const char* name, bool* stuffed) {
  const int64_t bound = acx_jpeg::encode_bound(H, W);
  std::vector<uint8_t> big((size_t)bound);
  const int64_t n = acx_jpeg::entropy_encode(coef.data(), coef.size(), qt, H, W, big.data(), big.size());
  check(n > 0 && n <= bound, "encode failed or passed the bound", H, W, name);
  if (n <= 0) return;
  uint8_t* exact = (uint8_t*)malloc((size_t)n);                    // exactly n bytes
  check(acx_jpeg::entropy_encode(coef.data(), coef.size(), qt, H, W, exact, (size_t)n) == n, "exact-size buffer refused", H, W, name);
  check(memcmp(exact, big.data(), (size_t)n) == 0, "the bytes depend on the buffer", H, W, name);
  uint8_t* small = (uint8_t*)malloc((size_t)n - 1);                // one byte short
  check(acx_jpeg::entropy_encode(coef.data(), coef.size(), qt, H, W, small, (size_t)n - 1) == ACX_E_WORKSPACE, "no ACX_E_WORKSPACE", H, W, name);
  free(small);
  check(acx_jpeg::entropy_encode(coef.data(), coef.size(), qt, H, W, nullptr, 0) == ACX_E_WORKSPACE, "empty buffer", H, W, name);
  acx_jpeg_info info;
  check(acx_jpeg::parse(exact, (size_t)n, &info) == ACX_OK, "parse", H, W, name);
  check(info.width == W && info.height == H && info.ncomp == 3 && info.comp_h[0] == 2 && info.comp_v[0] == 2, "geometry", H, W, name);
  check((size_t)info.coef_elems == coef.size(), "coef_elems", H, W, name);
  std::vector<int16_t> back(coef.size(), (int16_t)0);
  check(acx_jpeg::entropy_decode(exact, (size_t)n, &info, back.data(), back.size()) == ACX_OK, "decode", H, W, name);
  check(back == coef, "the coefficients did not come back", H, W, name);
  for (int64_t i = info.scan_offset; i + 1 < n - 2; ++i)
    if (exact[i] == 0xFF && exact[i + 1] == 0) *stuffed = true;
  free(exact);
}

int main() {
  static const uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  uint16_t qt[128];
  for (int i = 0; i < 128; ++i) qt[i] = (uint16_t)(1 + (i * 7) % 255);
  const int sizes[3][2] = {{16, 16}, {32, 48}, {800, 1200}};
  // the edge blocks
  std::vector<std::vector<int16_t>> edges;
  {
    std::vector<int16_t> b(64, 0);
    b[nat[63]] = 5;
    edges.push_back(b);
    for (int run = 16; run <= 62; ++run) {
      std::vector<int16_t> z(64, 0);
      z[nat[run + 1]] = (int16_t)((run & 1) ? -3 : 7);
      edges.push_back(z);
    }
    for (int v = -1023; v <= 1023; v += 2046) {
      std::vector<int16_t> a(64, 0);
      a[nat[1]] = (int16_t)v;
      a[nat[40]] = (int16_t)-v;
      a[nat[63]] = (int16_t)v;
      edges.push_back(a);
    }
  }
  bool stuffed = false;
  for (const auto& hw : sizes) {
    const int H = hw[0], W = hw[1];
    const size_t nb = (size_t)((W + 15) / 16) * ((H + 15) / 16) * 6, n = nb * 64;
    round_trip(std::vector<int16_t>(n, 0), qt, H, W, "all zero", &stuffed);
    for (size_t k = 0; k < edges.size(); k += nb) {
      std::vector<int16_t> c(n, 0);
      for (size_t j = 0; j < nb && k + j < edges.size(); ++j) memcpy(&c[j * 64], edges[k + j].data(), 128);
      round_trip(c, qt, H, W, "edge blocks", &stuffed);
    }
    std::vector<int16_t> dc(n, 0);
    for (size_t j = 0; j < nb; ++j) dc[j * 64] = (int16_t)((j & 1) ? -1023 : 1023);
    round_trip(dc, qt, H, W, "DC differences of category 11", &stuffed);
    std::vector<int16_t> dense(n);
    uint32_t seed = 99u + (uint32_t)H;
    for (size_t i = 0; i < n; ++i) {
      seed = seed * 1664525u + 1013904223u;
      dense[i] = (int16_t)((int)((seed >> 8) % 2047u) - 1023);
    }
    round_trip(dense, qt, H, W, "dense random", &stuffed);
    // values the tables cannot code are refused, not coded wrongly
    std::vector<int16_t> bad(n, 0);
    bad[5] = 1024;
    std::vector<uint8_t> buf((size_t)acx_jpeg::encode_bound(H, W));
    check(acx_jpeg::entropy_encode(bad.data(), n, qt, H, W, buf.data(), buf.size()) == ACX_E_BADARG, "AC 1024 accepted", H, W, "refusals");
    bad[5] = 0;
    bad[0] = 2000;
    bad[64] = -2000;
    check(acx_jpeg::entropy_encode(bad.data(), n, qt, H, W, buf.data(), buf.size()) == ACX_E_BADARG, "DC category 12 accepted", H, W, "refusals");
    check(acx_jpeg::entropy_encode(bad.data(), n - 64, qt, H, W, buf.data(), buf.size()) == ACX_E_BADARG, "short coef accepted", H, W, "refusals");
  }
  if (!stuffed) {
    fprintf(stderr, "no case produced an FF byte in its scan\n");
    ++failures;
  }
  printf("jpeg_encode_check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
