// inflate_core_check.cpp — the Deflate core (land_trendr_amd/csrc/lt_inflate_core.h) in a program
// of its own, built with AddressSanitizer and UBSan by tests/test_inflate_core_sanitized.py and run
// on the corpus file that test writes: records of
//   int64 n_in, int64 cap, int64 want (the count, or a negative error), n_in stream bytes,
//   max(want, 0) expected bytes.
// Each stream is copied into a heap buffer of exactly n_in bytes and decoded into one of exactly
// cap bytes, so a read or a write one byte outside either is a report. Prints "ok <cases>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../land_trendr_amd/csrc/lt_inflate_core.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> file;
  uint8_t chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + n);
  fclose(f);
  size_t pos = 0;
  long cases = 0;
  while (pos < file.size()) {
    int64_t hdr[3];
    if (file.size() - pos < sizeof hdr) return 3;
    memcpy(hdr, file.data() + pos, sizeof hdr);
    pos += sizeof hdr;
    const int64_t n_in = hdr[0], cap = hdr[1], want = hdr[2];
    const int64_t n_want = want > 0 ? want : 0;
    if (n_in < 0 || cap < 0 || (int64_t)(file.size() - pos) < n_in + n_want) return 3;
    uint8_t* in = (uint8_t*)malloc((size_t)n_in ? (size_t)n_in : 1);
    uint8_t* out = (uint8_t*)malloc((size_t)cap ? (size_t)cap : 1);
    if (n_in) memcpy(in, file.data() + pos, (size_t)n_in);
    memset(out, 0xEE, (size_t)cap);
    uint16_t table[lt_inflate::kEntries];
    const int64_t n = lt_inflate::decode(in, n_in, out, cap, lt_inflate::FlatTable{table});
    bool ok = n == want;
    if (ok && n_want) ok = memcmp(out, file.data() + pos + n_in, (size_t)n_want) == 0;
    // a success writes nothing past its count (a failing call may leave what it had decoded)
    for (int64_t i = n_want; ok && n >= 0 && i < cap; i++) ok = out[i] == 0xEE;
    free(in);
    free(out);
    if (!ok) {
      printf("case %ld: got %lld, want %lld\n", cases, (long long)n, (long long)want);
      return 1;
    }
    pos += (size_t)(n_in + n_want);
    cases++;
  }
  printf("ok %ld\n", cases);
  return 0;
}
