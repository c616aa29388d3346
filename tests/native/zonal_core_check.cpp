// The zonal table's per-pixel code (land_trendr_amd/csrc/lt_zonal.h) in a program of its own, for
// a sanitized build (tests/test_zonal_core_sanitized.py: g++ -fsanitize=address,undefined): reads
// a corpus of cases with their expected tables, runs the per-pixel code on buffers of exactly the
// sizes the ABI names, each on the heap, and compares every word.
//
// Corpus: per case eight little-endian int64 (P, key_lo, n_bins, n_zones, has_duration,
// has_value, 0, 0), then matched [P] u8, zone [P] i32, key [P] i32, duration [P] i32 if
// has_duration, value [P] f64 if has_value, the table the call starts from and the table it must
// leave, each [n_zones + 1][n_bins + 1][4] u64. Prints "ok <cases>" and exits 0, or says what
// differs and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../land_trendr_amd/csrc/lt_zonal.h"

template <class T>
static T* take(FILE* f, int64_t n) {
  T* p = (T*)malloc(n > 0 ? n * sizeof(T) : 1);
  if (n > 0 && fread(p, sizeof(T), n, f) != (size_t)n) {
    fprintf(stderr, "short corpus\n");
    exit(2);
  }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s corpus\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int64_t h[8];
  long c = 0;
  while (fread(h, sizeof(int64_t), 8, f) == 8) {
    const int64_t P = h[0];
    const int32_t key_lo = (int32_t)h[1], n_bins = (int32_t)h[2], n_zones = (int32_t)h[3];
    const int64_t words = lt::zonal_cells(n_zones, n_bins) * lt::kZonalWords;
    uint8_t* matched = take<uint8_t>(f, P);
    int32_t* zone = take<int32_t>(f, P);
    int32_t* key = take<int32_t>(f, P);
    int32_t* duration = h[4] ? take<int32_t>(f, P) : nullptr;
    double* value = h[5] ? take<double>(f, P) : nullptr;
    uint64_t* table = take<uint64_t>(f, words);
    uint64_t* want = take<uint64_t>(f, words);
    const char* why;
    const int rc = lt::zonal_check(matched, zone, key, P, n_bins, n_zones, 0, table, &why);
    if (rc != LT_OK) return fprintf(stderr, "case %ld: rc %d (%s)\n", c, rc, why), 1;
    const lt::ZonalArgs A = {matched, zone, key, duration, value, P, key_lo, n_bins, n_zones,
                             (unsigned long long*)table};
    for (int64_t p = 0; p < P; p++) {
      const lt::ZonalPix x = lt::zonal_pixel(A, p);
      if (x.cell < 0) continue;
      uint64_t* w = table + (int64_t)x.cell * lt::kZonalWords;
      w[0] += 1;
      w[1] += (uint64_t)x.dur;
      w[2] += (uint64_t)x.q;
      w[3] += (uint64_t)x.has_value;
    }
    for (int64_t i = 0; i < words; i++) {
      if (table[i] == want[i]) continue;
      fprintf(stderr, "case %ld: word %lld is %lld, expected %lld\n", c, (long long)i,
              (long long)table[i], (long long)want[i]);
      return 1;
    }
    free(matched); free(zone); free(key); free(duration); free(value); free(table); free(want);
    c++;
  }
  fclose(f);
  printf("ok %ld\n", c);
  return 0;
}
