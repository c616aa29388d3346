// grid_sample_check.cpp — the grid sampling core (land_trendr_amd/csrc/lt_sample.h) and its
// threaded host build (lt_io.cpp lt_grid_sample) in a program of their own, to be compiled with
// -fsanitize=address,undefined together with lt_io.cpp (tests/test_sample_host.py): the shapes of
// the Python corpus (tests/samplefixture.py) — a grid of 37 x 53, a source of 29 x 61 shifted by
// (-5, +3), one smaller than the grid in both axes, sample sizes 1, 2, 4 and 8 bytes, three band
// selections of 6 bands, four pixel ranges, out_stride > n inside canaries, the mask mode over a
// validity row that is partly 0 — against a per-pixel restatement, and every rejected argument.
// Every buffer is a heap allocation of its exact size, so a read or write outside one is reported.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/lt_io.h"

namespace {

constexpr int64_t kH = 37, kW = 53, kP = kH * kW;
constexpr uint8_t kCanary = 0xA5;
constexpr int kPad = 24;
int failures = 0;

void fail(const char* what, int a = 0, int b = 0, int c = 0) {
  if (failures++ < 10) printf("FAIL %s (%d, %d, %d)\n", what, a, b, c);
}

// grid index i + shift as pt2val addresses a raster of n: valid in [-n, n), negatives wrapped
std::vector<int32_t> axis(int64_t len, int64_t shift, int64_t n) {
  std::vector<int32_t> o((size_t)len);
  for (int64_t i = 0; i < len; i++) {
    const int64_t v = i + shift;
    o[(size_t)i] = (v < -n || v >= n) ? -1 : (int32_t)(v < 0 ? v + n : v);
  }
  return o;
}

uint64_t rnd(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return s >> 17;
}

struct Source {
  int64_t h, w, dy, dx;
};

void run_case(const Source& S, int bps, const std::vector<int32_t>& sel, int64_t p0, int64_t p1,
              int threads, uint64_t seed) {
  const int bands = 6;
  const int64_t n = p1 - p0, stride = n + 5;
  std::vector<uint8_t> src((size_t)(bands * S.h * S.w * bps));
  for (auto& b : src) b = (uint8_t)rnd(seed);
  const std::vector<int32_t> xo = axis(kW, S.dx, S.w), yo = axis(kH, S.dy, S.h);
  std::vector<uint8_t> out((size_t)(sel.size() * stride * bps + 2 * kPad), kCanary);
  std::vector<uint8_t> valid((size_t)(n + 2 * kPad), kCanary);
  const int64_t rc = lt_grid_sample(src.data(), bps, bands, S.h, S.w, xo.data(), yo.data(), kW, kH,
                                    p0, n, (int)sel.size(), sel.data(), out.data() + kPad, stride,
                                    valid.data() + kPad, 0, threads);
  if (rc != 0) return fail("bands rc", (int)rc);
  std::vector<uint8_t> want_out(out.size(), kCanary), want_valid(valid.size(), kCanary);
  for (int64_t i = 0; i < n; i++) {
    const int64_t r = (p0 + i) / kW, c = (p0 + i) % kW;
    const bool on = xo[(size_t)c] >= 0 && yo[(size_t)r] >= 0;
    want_valid[(size_t)(kPad + i)] = on ? 1 : 0;
    for (size_t b = 0; b < sel.size(); b++) {
      uint8_t* d = want_out.data() + kPad + ((int64_t)b * stride + i) * bps;
      if (on)
        memcpy(d, src.data() + ((sel[b] * S.h + yo[(size_t)r]) * S.w + xo[(size_t)c]) * bps,
               (size_t)bps);
      else
        memset(d, 0, (size_t)bps);
    }
  }
  if (out != want_out) fail("bands out", bps, (int)p0, (int)p1);
  if (valid != want_valid) fail("bands valid", bps, (int)p0, (int)p1);

  // the mask: its own extent, many zero samples, over the validity row just made
  const Source M{40, 50, 2, -4};
  std::vector<uint8_t> mask((size_t)(2 * M.h * M.w * bps));
  for (int64_t k = 0; k < 2 * M.h * M.w; k++) {
    const bool zero = rnd(seed) % 5 < 2;
    for (int b = 0; b < bps; b++) mask[(size_t)(k * bps + b)] = zero ? 0 : (uint8_t)(rnd(seed) | 1);
  }
  const std::vector<int32_t> mx = axis(kW, M.dx, M.w), my = axis(kH, M.dy, M.h);
  const int32_t sel0 = 0;
  const int64_t rm = lt_grid_sample(mask.data(), bps, 2, M.h, M.w, mx.data(), my.data(), kW, kH, p0,
                                    n, 1, &sel0, nullptr, 0, valid.data() + kPad, 1, threads);
  if (rm != 0) return fail("mask rc", (int)rm);
  for (int64_t i = 0; i < n; i++) {
    const int64_t r = (p0 + i) / kW, c = (p0 + i) % kW;
    if (mx[(size_t)c] < 0 || my[(size_t)r] < 0) continue;
    const uint8_t* m = mask.data() + (my[(size_t)r] * M.w + mx[(size_t)c]) * bps;
    bool zero = true;
    for (int b = 0; b < bps; b++) zero = zero && m[b] == 0;
    if (zero) want_valid[(size_t)(kPad + i)] = 0;
  }
  if (valid != want_valid) fail("mask valid", bps, (int)p0, (int)p1);
}

void expect_arg_error(const char* what, int64_t rc, const std::vector<uint8_t>& out,
                      const std::vector<uint8_t>& valid) {
  if (rc != LT_IO_ERR_ARG) fail(what, (int)rc);
  for (uint8_t b : out)
    if (b != kCanary) return fail(what, -100);
  for (uint8_t b : valid)
    if (b != kCanary) return fail(what, -101);
}

void run_rejects() {
  const int64_t h = 29, w = 61, n = 64;
  std::vector<uint8_t> src((size_t)(6 * h * w * 2 + 2), 1);
  const std::vector<int32_t> xo = axis(kW, 3, w), yo = axis(kH, -5, h);
  std::vector<uint8_t> out((size_t)(2 * n * 2 + 2), kCanary), valid((size_t)n, kCanary);
  const int32_t sel[2] = {1, 0}, bad_hi[2] = {6, 0}, bad_lo[2] = {0, -1};
  const int64_t big = (int64_t)1 << 31;
#define CALL(SRC, BPS, NB, SH, SW, XO, YO, GW, GH, P0, N, NS, SEL, OUT, OS, VAL, MODE)              \
  lt_grid_sample(SRC, BPS, NB, SH, SW, XO, YO, GW, GH, P0, N, NS, SEL, OUT, OS, VAL, MODE, 2)
  const uint8_t* s = src.data();
  uint8_t* o = out.data();
  uint8_t* v = valid.data();
  const int32_t* x = xo.data();
  const int32_t* y = yo.data();
  expect_arg_error("bps 3", CALL(s, 3, 6, h, w, x, y, kW, kH, 10, n, 2, sel, o, n, v, 0), out, valid);
  expect_arg_error("mode", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, n, 2, sel, o, n, v, 2), out, valid);
  expect_arg_error("n_sel 0", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, n, 0, sel, o, n, v, 0), out, valid);
  expect_arg_error("n_sel 17", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, n, 17, sel, o, n, v, 0), out, valid);
  expect_arg_error("sel high", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, n, 2, bad_hi, o, n, v, 0), out, valid);
  expect_arg_error("sel low", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, n, 2, bad_lo, o, n, v, 0), out, valid);
  expect_arg_error("sel null", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, n, 2, nullptr, o, n, v, 0), out, valid);
  expect_arg_error("src_h < 0", CALL(s, 2, 6, -1, w, x, y, kW, kH, 10, n, 2, sel, o, n, v, 0), out, valid);
  expect_arg_error("src_w big", CALL(s, 2, 6, h, big, x, y, kW, kH, 10, n, 2, sel, o, n, v, 0), out, valid);
  expect_arg_error("grid_w < 0", CALL(s, 2, 6, h, w, x, y, -1, kH, 10, n, 2, sel, o, n, v, 0), out, valid);
  expect_arg_error("p0 < 0", CALL(s, 2, 6, h, w, x, y, kW, kH, -1, n, 2, sel, o, n, v, 0), out, valid);
  expect_arg_error("n < 0", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, -1, 2, sel, o, n, v, 0), out, valid);
  expect_arg_error("past the grid", CALL(s, 2, 6, h, w, x, y, kW, kH, kP - 63, n, 2, sel, o, n, v, 0), out, valid);
  expect_arg_error("out_stride", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, n, 2, sel, o, n - 1, v, 0), out, valid);
  expect_arg_error("src null", CALL(nullptr, 2, 6, h, w, x, y, kW, kH, 10, n, 2, sel, o, n, v, 0), out, valid);
  expect_arg_error("out null", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, n, 2, sel, nullptr, n, v, 0), out, valid);
  expect_arg_error("valid null", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, n, 2, sel, o, n, nullptr, 0), out, valid);
  expect_arg_error("src misaligned", CALL(s + 1, 2, 6, h, w, x, y, kW, kH, 10, n, 2, sel, o, n, v, 0), out, valid);
  expect_arg_error("out misaligned", CALL(s, 2, 6, h, w, x, y, kW, kH, 10, n, 2, sel, o + 1, n, v, 0), out, valid);
#undef CALL
}

}  // namespace

int main() {
  const Source sources[2] = {{29, 61, -5, 3}, {11, 17, -13, -20}};
  const std::vector<std::vector<int32_t>> sels = {{0}, {1, 0}, {2, 4}};
  const int64_t ranges[4][2] = {{0, kP}, {17, 18}, {60, 191}, {100, 100}};
  int cases = 0;
  for (const Source& S : sources)
    for (int bps : {1, 2, 4, 8})
      for (const auto& sel : sels)
        for (const auto& r : ranges)
          for (int threads : {1, 3}) {
            run_case(S, bps, sel, r[0], r[1], threads, 1000 + (uint64_t)cases);
            cases++;
          }
  run_rejects();
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok %d cases\n", cases);
  return 0;
}
