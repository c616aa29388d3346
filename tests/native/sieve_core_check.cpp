// The MMU sieve's phase steps (land_trendr_amd/csrc/lt_sieve.h) in a program of its own, for a
// sanitized build (tests/test_sieve_core_sanitized.py: g++ -fsanitize=address,undefined): reads a
// corpus of cases with their expected outputs, runs the serial twin of the four launches on
// buffers of exactly the sizes the ABI names, each on the heap, and compares every element.
//
// Corpus: per case six little-endian int64 (rows, cols, connectivity, min_pixels, has_key,
// reverse), then matched [P] uint8, key [P] int32 if has_key, and the expected root [P] int32,
// size [P] int32 and applied matched [P] uint8. Prints "ok <cases>" and exits 0, or says what
// differs and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../land_trendr_amd/csrc/lt_sieve.h"

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
  int64_t h[6];
  long n_cases = 0;
  while (fread(h, sizeof(int64_t), 6, f) == 6) {
    const int64_t P = h[0] * h[1];
    uint8_t* matched = take<uint8_t>(f, P);
    int32_t* key = h[4] ? take<int32_t>(f, P) : nullptr;
    int32_t* key0 = nullptr;
    if (key) {
      key0 = (int32_t*)malloc(P > 0 ? P * 4 : 1);
      memcpy(key0, key, P * 4);
    }
    int32_t* want_root = take<int32_t>(f, P);
    int32_t* want_size = take<int32_t>(f, P);
    uint8_t* want_matched = take<uint8_t>(f, P);
    const int64_t wb = lt::sieve_workspace_bytes(h[0], h[1]);
    if (wb < 8) return fprintf(stderr, "case %ld: workspace bytes %lld\n", n_cases, (long long)wb), 1;
    int32_t* root = (int32_t*)malloc(P > 0 ? P * 4 : 1);
    int32_t* size = (int32_t*)malloc(P > 0 ? P * 4 : 1);
    void* ws = malloc(wb);
    lt_sieve_in in;
    memset(&in, 0, sizeof in);
    in.rows = h[0];
    in.cols = h[1];
    in.matched = matched;
    in.key = key;
    in.connectivity = (int32_t)h[2];
    in.min_pixels = (int32_t)h[3];
    in.apply = 1;
    lt_sieve_out out = {root, size, ws, wb};
    const char* why;
    const int rc = lt::sieve_check(&in, &out, &why);
    if (rc != LT_OK) return fprintf(stderr, "case %ld: rc %d (%s)\n", n_cases, rc, why), 1;
    if (P > 0) {
      lt::SieveArgs A;
      lt::sieve_args(&in, &out, A);
      lt::sieve_host(A, h[5] != 0);
    }
    for (int64_t q = 0; q < P; q++) {
      if (root[q] != want_root[q] || size[q] != want_size[q] || matched[q] != want_matched[q] ||
          (key && key[q] != key0[q])) {
        fprintf(stderr, "case %ld (%lld x %lld): pixel %lld root %d/%d size %d/%d matched %d/%d\n",
                n_cases, (long long)h[0], (long long)h[1], (long long)q, root[q], want_root[q],
                size[q], want_size[q], matched[q], want_matched[q]);
        return 1;
      }
    }
    free(matched); free(key); free(key0); free(want_root); free(want_size); free(want_matched);
    free(root); free(size); free(ws);
    n_cases++;
  }
  fclose(f);
  printf("ok %ld\n", n_cases);
  return 0;
}
