// Stand-alone check of the host JPEG decoder (anomalyclip_amd/csrc/acx_jpeg_host.h) for a sanitizer build:
//
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp -o jpeg_host_check
//   ./jpeg_host_check a.jpg b.jpg ...
//
// Every file named on the command line is parsed and entropy-decoded whole, cut at 40 evenly spaced lengths, and with seeded byte
// flips inside its scan.  Each variant is decoded from a heap copy of exactly its length into a heap buffer of exactly the frame's
// coefficients, so a read or a write one byte outside either is the sanitizer's to report.  Any error code is a fine answer for a
// damaged file; exit status 0 means that no call misbehaved and that every whole file gave what its name promises (a name that
// holds "unsupported" must be ACX_E_UNSUPPORTED, every other file ACX_OK).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../anomalyclip_amd/csrc/acx_jpeg_host.h"

static int run(const uint8_t* src, size_t n, int* parse_rc) {
  uint8_t* data = (uint8_t*)malloc(n ? n : 1);           // exactly n bytes: an over-read is out of bounds
  if (n) memcpy(data, src, n);
  acx_jpeg_info info;
  int rc = acx_jpeg::parse(data, n, &info);
  if (parse_rc) *parse_rc = rc;
  if (rc == ACX_OK) {
    std::vector<int16_t> coef((size_t)info.coef_elems, (int16_t)0);
    rc = acx_jpeg::entropy_decode(data, n, &info, coef.data(), coef.size());
    if (rc == ACX_OK && info.coef_elems > 64) {          // a buffer one block short must be refused, not overrun
      std::vector<int16_t> small((size_t)info.coef_elems - 64, (int16_t)0);
      if (acx_jpeg::entropy_decode(data, n, &info, small.data(), small.size()) != ACX_E_BADARG) rc = 1;
    }
  }
  free(data);
  return rc;
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* fh = fopen(argv[a], "rb");
    if (!fh) {
      fprintf(stderr, "%s: cannot open\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> file;
    uint8_t chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), fh)) > 0) file.insert(file.end(), chunk, chunk + got);
    fclose(fh);
    int prc = 0;
    const int rc = run(file.data(), file.size(), &prc);
    const bool unsupported = strstr(argv[a], "unsupported") != nullptr;
    const int want = unsupported ? ACX_E_UNSUPPORTED : ACX_OK;
    printf("%s: %zu bytes -> %d\n", argv[a], file.size(), rc);
    if (rc != want) {
      fprintf(stderr, "%s: expected %d, got %d\n", argv[a], want, rc);
      ++bad;
    }
    for (int k = 0; k < 40; ++k) {                       // truncations
      const int t = run(file.data(), file.size() * (size_t)k / 40, nullptr);
      if (t > 0) ++bad;
    }
    if (prc == ACX_OK) {                                 // byte flips inside the scan
      acx_jpeg_info info;
      acx_jpeg::parse(file.data(), file.size(), &info);
      uint32_t seed = 12345u + (uint32_t)a;
      for (int k = 0; k < 40; ++k) {
        std::vector<uint8_t> f2(file);
        for (int j = 0; j < 1 + k % 4; ++j) {
          seed = seed * 1664525u + 1013904223u;
          const size_t span = file.size() - (size_t)info.scan_offset;
          if (span == 0) break;
          const size_t at = (size_t)info.scan_offset + (seed >> 8) % span;
          seed = seed * 1664525u + 1013904223u;
          f2[at] ^= (uint8_t)(1u << ((seed >> 16) & 7));
        }
        if (run(f2.data(), f2.size(), nullptr) > 0) ++bad;
      }
    }
  }
  return bad ? 1 : 0;
}
