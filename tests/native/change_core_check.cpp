// The change maps' per-pixel code (land_trendr_amd/csrc/lt_change.h) in a program of its own, for
// a sanitized build (tests/test_change_core_sanitized.py: g++ -fsanitize=address,undefined): reads
// a corpus of cases with their expected outputs, runs the per-pixel code on buffers of exactly the
// sizes the ABI names, each on the heap, and compares every element bit for bit (any NaN equal to
// any NaN).
//
// Corpus: per case six little-endian int64 (P, Y, M, presence: 0 none / 1 present / 2 winner,
// has_fit, 0), then year [Y] int32, M lt_change_rule structs, val_fit [Y][P] f64, vertex [Y][P]
// u8, the presence plane (u8 or i16) if any, val_raw [Y][P] f64 and spike [Y][P] u8 if has_fit;
// then the expected matched [M][P] u8, onset_year and duration [M][P] i32, magnitude, preval, rate
// [M][P] f64 and, if has_fit, dsnr [M][P] f64, rmse [P] f64, n_fit [P] i32. Prints "ok <cases>"
// and exits 0, or says what differs and exits 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../land_trendr_amd/csrc/lt_change.h"

template <class T>
static T* take(FILE* f, int64_t n) {
  T* p = (T*)malloc(n > 0 ? n * sizeof(T) : 1);
  if (n > 0 && fread(p, sizeof(T), n, f) != (size_t)n) {
    fprintf(stderr, "short corpus\n");
    exit(2);
  }
  return p;
}

template <class T>
static T* fresh(int64_t n) {
  return (T*)malloc(n > 0 ? n * sizeof(T) : 1);
}

template <class T>
static bool differ(const char* what, long c, const T* got, const T* want, int64_t n) {
  for (int64_t i = 0; i < n; i++) {
    if (memcmp(&got[i], &want[i], sizeof(T)) == 0) continue;
    if (sizeof(T) == 8 && std::isnan((double)got[i]) && std::isnan((double)want[i])) continue;
    fprintf(stderr, "case %ld: %s[%lld] is %.17g, expected %.17g\n", c, what, (long long)i,
            (double)got[i], (double)want[i]);
    return true;
  }
  return false;
}

template <int M>
static void run(const lt_change_in* in, int n_maps, const lt_change_rule* rules,
                const lt_change_out* out) {
  lt::ChangeArgs<M> A;
  lt::change_args<M>(in, n_maps, rules, out, A);
  for (int64_t p = 0; p < in->n_pix; p++) lt::change_pixel<M>(A, p);
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: %s corpus\n", argv[0]), 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  int64_t h[6];
  long c = 0;
  while (fread(h, sizeof(int64_t), 6, f) == 6) {
    const int64_t P = h[0], Y = h[1], M = h[2], YP = Y * P, MP = M * P;
    const bool fit = h[4] != 0;
    int32_t* year = take<int32_t>(f, Y);
    lt_change_rule* rules = take<lt_change_rule>(f, M);
    double* val_fit = take<double>(f, YP);
    uint8_t* vertex = take<uint8_t>(f, YP);
    uint8_t* present = h[3] == 1 ? take<uint8_t>(f, YP) : nullptr;
    int16_t* winner = h[3] == 2 ? take<int16_t>(f, YP) : nullptr;
    double* val_raw = fit ? take<double>(f, YP) : nullptr;
    uint8_t* spike = fit ? take<uint8_t>(f, YP) : nullptr;
    uint8_t* w_matched = take<uint8_t>(f, MP);
    int32_t* w_onset = take<int32_t>(f, MP);
    int32_t* w_dur = take<int32_t>(f, MP);
    double* w_mag = take<double>(f, MP);
    double* w_pre = take<double>(f, MP);
    double* w_rate = take<double>(f, MP);
    double* w_dsnr = fit ? take<double>(f, MP) : nullptr;
    double* w_rmse = fit ? take<double>(f, P) : nullptr;
    int32_t* w_nfit = fit ? take<int32_t>(f, P) : nullptr;
    lt_change_in in;
    memset(&in, 0, sizeof in);
    in.n_pix = P;
    in.stride = P;
    in.n_years = (int32_t)Y;
    in.year = year;
    in.val_fit = val_fit;
    in.vertex = vertex;
    in.val_raw = val_raw;
    in.present = present;
    in.winner = winner;
    in.spike = spike;
    lt_change_out out;
    memset(&out, 0, sizeof out);
    out.stride = P;
    out.matched = fresh<uint8_t>(MP);
    out.onset_year = fresh<int32_t>(MP);
    out.duration = fresh<int32_t>(MP);
    out.magnitude = fresh<double>(MP);
    out.preval = fresh<double>(MP);
    out.rate = fresh<double>(MP);
    if (fit) {
      out.dsnr = fresh<double>(MP);
      out.rmse = fresh<double>(P);
      out.n_fit = fresh<int32_t>(P);
    }
    const char* why;
    const int rc = lt::change_check(&in, (int)M, rules, &out, &why);
    if (rc != LT_OK) return fprintf(stderr, "case %ld: rc %d (%s)\n", c, rc, why), 1;
    if (P > 0) {
      switch (lt::change_instance((int)M)) {
        case 1: run<1>(&in, (int)M, rules, &out); break;
        case 2: run<2>(&in, (int)M, rules, &out); break;
        case 4: run<4>(&in, (int)M, rules, &out); break;
        default: run<8>(&in, (int)M, rules, &out); break;
      }
    }
    if (differ("matched", c, out.matched, w_matched, MP) ||
        differ("onset_year", c, out.onset_year, w_onset, MP) ||
        differ("duration", c, out.duration, w_dur, MP) ||
        differ("magnitude", c, out.magnitude, w_mag, MP) ||
        differ("preval", c, out.preval, w_pre, MP) || differ("rate", c, out.rate, w_rate, MP))
      return 1;
    if (fit && (differ("dsnr", c, out.dsnr, w_dsnr, MP) || differ("rmse", c, out.rmse, w_rmse, P) ||
                differ("n_fit", c, out.n_fit, w_nfit, P)))
      return 1;
    free(year); free(rules); free(val_fit); free(vertex); free(present); free(winner);
    free(val_raw); free(spike); free(w_matched); free(w_onset); free(w_dur); free(w_mag);
    free(w_pre); free(w_rate); free(w_dsnr); free(w_rmse); free(w_nfit);
    free(out.matched); free(out.onset_year); free(out.duration); free(out.magnitude);
    free(out.preval); free(out.rate); free(out.dsnr); free(out.rmse); free(out.n_fit);
    c++;
  }
  fclose(f);
  printf("ok %ld\n", c);
  return 0;
}
