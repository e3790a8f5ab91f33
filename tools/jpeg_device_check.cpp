// Stand-alone check of the device entropy decoder's text on the CPU, for a sanitizer build:
//
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_device_check.cpp -o jpeg_device_check
//   ./jpeg_device_check a.jpg b.jpg ...                 (--list: also prints one line per variant: file, kind, index, status)
//
// It includes acx_jpeg_scan_pack's body (acx_jpeg_host.h) and the header the kernel is made of (acx_jpeg_sync.h) and runs the
// kernel's phases -- tables, speculation, synchronisation rounds, prefix sums, write pass, status -- with the workgroup's threads
// emulated one after the other.  Every file named on the command line is taken whole, cut at 40 evenly spaced lengths, and with
// seeded bit flips inside its scan (the variants of tools/jpeg_host_check.cpp); each variant lives in a heap copy of exactly its
// length, its packed scan in a heap buffer of exactly its padded length, its coefficients in one of exactly the frame's.  For every
// variant the parser and the packer accept, at sub_bits 32 (where 1024 subsequences cover the scan), 64 and automatic, the status
// must equal acx_jpeg_entropy_decode's, and the coefficients too wherever that status is 0 (a failed frame's coefficients are
// whatever the host decoder had written when it gave up: nothing reads them).  Exit status 0: all of that held, and every whole file
// decoded with status 0.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../anomalyclip_amd/csrc/acx_jpeg_host.h"
#include "../anomalyclip_amd/csrc/acx_jpeg_sync.h"

using namespace acx_jsync;

// the kernel's body for one frame; `rounds` receives the synchronisation rounds it took
static int device_decode(const uint8_t* scan, size_t scan_bytes_padded, int64_t bits64, const acx_jpeg_huff* huff, const Geo& g,
                         uint32_t sub_arg, int16_t* coef, uint32_t* rounds) {
  const uint8_t* hf = (const uint8_t*)huff;
  const uint32_t sub = sub_arg ? sub_arg : min_sub_bits(bits64 < 0 ? 0 : (uint64_t)bits64);
  bool ok = bits64 >= 0 && (uint64_t)sub * kThreads >= (uint64_t)bits64 && (bits64 + 31) / 32 * 4 <= (int64_t)scan_bytes_padded;
  uint32_t used = 0, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
  for (uint32_t c = 0; c < 3; ++c)
    if (c < g.ncomp) {
      td[c] = hf[kHuffTd + c];
      ta[c] = hf[kHuffTa + c];
      ok = ok && td[c] < 4 && ta[c] < 4;
      td[c] &= 3;
      ta[c] &= 3;
      ok = ok && hf[kHuffPresent + td[c]] && hf[kHuffPresent + 4 + ta[c]];
      used |= (1u << td[c]) | (16u << ta[c]);
    }
  if (!ok) return kBad;
  const uint32_t bits = (uint32_t)bits64;
  const uint32_t nsub = bits == 0 ? 1u : (bits + sub - 1) / sub;
  if (nsub > (uint32_t)kThreads) abort();

  Shared* Sp = (Shared*)calloc(1, sizeof(Shared));       // (zeroed: the look tables and the records, as the kernel's threads do)
  Shared& S = *Sp;
  for (uint32_t i = 0; i < 8 * 256; ++i) S.tab[i >> 8].vals[i & 255] = hf[kHuffVals + i];
  for (uint32_t c = 0; c < 3; ++c) {
    S.sel[0][c] = td[c];
    S.sel[1][c] = 4 + ta[c];
  }
  int bad = 0;
  for (uint32_t t = 0; t < 8; ++t)
    if ((used >> t) & 1)
      if (derive_codes(hf + kHuffBits + t * 17, &S.tab[t]) != 0) bad = 1;
  if (bad) {
    free(Sp);
    return kBad;
  }
  std::vector<Scan> sc(nsub);
  std::vector<State> st(nsub);
  std::vector<char> active(nsub, 1);
  for (uint32_t t = 0; t < nsub; ++t) {
    scan_init(&sc[t], (const uint32_t*)scan, bits);
    phase_speculate(S, g, sc[t], t, sub, st[t]);
  }
  uint32_t r = 1;
  for (; r < nsub; ++r) {
    bool any = false;
    for (uint32_t t = 0; t < nsub; ++t) {
      bool a = active[t] != 0;
      any |= phase_sync_round(S, g, sc[t], t, r, sub, nsub, st[t], a);
      active[t] = a;
    }
    if (!any) break;
  }
  *rounds = r;
  for (uint32_t t = 1; t < (uint32_t)kThreads; ++t) {
    S.nblk[t] += S.nblk[t - 1];
    for (int c = 0; c < 3; ++c) S.dc[c][t] += S.dc[c][t - 1];
  }
  for (uint32_t t = 0; t < nsub; ++t) phase_write(S, g, sc[t], t, sub, coef);
  const int rc = (S.err || !S.done) ? kBad : 0;
  free(Sp);
  return rc;
}

static int g_list = 0;

// 0: the variant agrees (or is not the device decoder's to take); 1: a disagreement.  *status: the host decoder's answer
static int run(const char* name, const char* kind, int index, const uint8_t* src, size_t n, int* status) {
  uint8_t* data = (uint8_t*)malloc(n ? n : 1);           // exactly n bytes: an over-read is out of bounds
  if (n) memcpy(data, src, n);
  acx_jpeg_info info;
  int bad = 0;
  int rc = acx_jpeg::parse(data, n, &info);
  *status = rc;
  Geo g;
  if (rc == ACX_OK && make_geo(info.height, info.width, info.ncomp, info.comp_h[0], info.comp_v[0], &g)) {
    if ((int64_t)g.coef_elems != info.coef_elems) abort();
    std::vector<int16_t> want((size_t)info.coef_elems, (int16_t)0);
    const int host = acx_jpeg::entropy_decode(data, n, &info, want.data(), want.size());
    *status = host;
    // the packer: a destination one byte short is refused, the exact one is filled to its last byte and no further
    const size_t room = (n - (size_t)info.scan_offset + ACX_JPEG_SCAN_ALIGN - 1) / ACX_JPEG_SCAN_ALIGN * ACX_JPEG_SCAN_ALIGN;
    uint8_t* tmp = (uint8_t*)malloc(room ? room : 1);
    int64_t payload = -1;
    acx_jpeg_huff huff;
    const int prc = acx_jpeg::scan_pack(data, n, &info, tmp, room, &payload, &huff);
    if (prc == ACX_E_UNSUPPORTED) {
      if (info.restart_interval == 0) bad = 1;
    } else if (prc != ACX_OK) {
      fprintf(stderr, "%s %s %d: scan_pack -> %d\n", name, kind, index, prc);
      bad = 1;
    } else {
      const size_t padded = ((size_t)payload + ACX_JPEG_SCAN_ALIGN - 1) / ACX_JPEG_SCAN_ALIGN * ACX_JPEG_SCAN_ALIGN;
      uint8_t* scan = (uint8_t*)malloc(padded ? padded : 1);
      int64_t p2 = -1;
      if (acx_jpeg::scan_pack(data, n, &info, scan, padded, &p2, nullptr) != ACX_OK || p2 != payload) bad = 1;
      if (padded > 0 && acx_jpeg::scan_pack(data, n, &info, scan, padded - 1, &p2, nullptr) != ACX_E_BADARG) bad = 1;
      if (acx_jpeg::scan_pack(data, n, &info, scan, padded, &p2, nullptr) != ACX_OK) bad = 1;
      const uint32_t autosub = min_sub_bits((uint64_t)payload * 8);
      const uint32_t subs[3] = {32, 64, 0};
      for (int k = 0; k < 3; ++k) {
        if (subs[k] && subs[k] < autosub) continue;      // (an explicit size too small for the scan is refused before any launch)
        int16_t* got = (int16_t*)calloc((size_t)g.coef_elems, sizeof(int16_t));
        uint32_t rounds = 0;
        const int dev = device_decode(scan, padded, payload * 8, &huff, g, subs[k], got, &rounds);
        if (dev != host) {
          fprintf(stderr, "%s %s %d sub_bits %u: status %d, the host decoder's %d\n", name, kind, index, subs[k], dev, host);
          bad = 1;
        } else if (host == ACX_OK && memcmp(got, want.data(), (size_t)g.coef_elems * sizeof(int16_t)) != 0) {
          fprintf(stderr, "%s %s %d sub_bits %u: coefficients differ\n", name, kind, index, subs[k]);
          bad = 1;
        }
        if (g_list && k == 0)
          printf("%s\t%s\t%d\t%d\t%lld\t%u\n", name, kind, index, host, (long long)payload, rounds);
        free(got);
      }
      free(scan);
    }
    free(tmp);
  }
  free(data);
  return bad;
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--list")) {
      g_list = 1;
      continue;
    }
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
    int status = 0;
    bad += run(argv[a], "whole", 0, file.data(), file.size(), &status);
    if (status != ACX_OK) {
      fprintf(stderr, "%s: the host decoder gives %d on the whole file\n", argv[a], status);
      ++bad;
    }
    for (int k = 0; k < 40; ++k) bad += run(argv[a], "cut", k, file.data(), file.size() * (size_t)k / 40, &status);
    acx_jpeg_info info;
    if (acx_jpeg::parse(file.data(), file.size(), &info) == ACX_OK) {
      uint32_t seed = 12345u + (uint32_t)file.size();
      for (int k = 0; k < 40; ++k) {                     // bit flips inside the scan
        std::vector<uint8_t> f2(file);
        for (int j = 0; j < 1 + k % 4; ++j) {
          seed = seed * 1664525u + 1013904223u;
          const size_t span = file.size() - (size_t)info.scan_offset;
          if (span == 0) break;
          const size_t at = (size_t)info.scan_offset + (seed >> 8) % span;
          seed = seed * 1664525u + 1013904223u;
          f2[at] ^= (uint8_t)(1u << ((seed >> 16) & 7));
        }
        bad += run(argv[a], "flip", k, f2.data(), f2.size(), &status);
      }
    }
  }
  if (bad) fprintf(stderr, "%d variants disagree\n", bad);
  return bad ? 1 : 0;
}
