// lt_change.h — the change maps' per-pixel code (lt_abi.h lt_change_maps) and the key count's
// (lt_label_counts), host and device: one source for the kernels (lt_change.hip) and for their
// host twin (tests/native/change_host_check.hip).
//
// A pixel's segments are walked the way label_pixel (lt_pixel.h) and vertex_pixel (lt_vertex.h)
// walk its vertices: the slots that hold a point in year order, the first of them the first left
// vertex whatever its flag says, every later flagged one closing a segment and opening the next.
// Every map is evaluated on a segment as it closes, so the planes are read once however many maps
// there are; the per-map state (the winner's year, duration, magnitude, preval and rate, and one
// bit of a found mask) is held in arrays that are only ever indexed by the unrolled map loop's
// counter, so it stays in registers (M is a template parameter: 1, 2, 4 or 8).
#pragma once
#include <stdint.h>

#include "../../include/lt_abi.h"

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace lt {

// what the kernel is launched with: the ABI structs, the years and the rules by value (uniform:
// the years and the rules are read with scalar loads)
template <int M>
struct ChangeArgs {
  lt_change_in in;    // (in.year is a host pointer: never read on the device)
  lt_change_out out;
  int32_t n_maps;     // <= M
  int32_t want_fit;   // rmse, n_fit or dsnr is written: val_raw and spike are read
  int32_t year[LT_MAX_YEARS];
  lt_change_rule rule[M];
};

// the smallest instance that holds n_maps
inline int change_instance(int n_maps) { return n_maps <= 1 ? 1 : n_maps <= 2 ? 2 : n_maps <= 4 ? 4 : 8; }

inline bool change_op_ok(int32_t op) {
  return op == LT_Q_UNSET || op == LT_Q_GT || op == LT_Q_LT || op == LT_Q_GE || op == LT_Q_LE;
}

// the argument checks of lt_change_maps, shared with the host twin: LT_OK or the LT_ERR_* code and
// what to say (n_pix == 0 is LT_OK too: the caller returns before it launches anything)
inline int change_check(const lt_change_in* in, int n_maps, const lt_change_rule* rules,
                        const lt_change_out* out, const char** why) {
  *why = "";
  if (!in || !rules || !out) return *why = "null argument", LT_ERR_ARG;
  if (in->n_pix < 0 || in->n_years < 0) return *why = "negative n_pix or n_years", LT_ERR_ARG;
  if (in->n_pix == 0) return LT_OK;
  if (n_maps < 1 || n_maps > LT_MAX_CHANGE_MAPS)
    return *why = "n_maps outside [1, LT_MAX_CHANGE_MAPS]", LT_ERR_ARG;
  if (in->n_years > LT_MAX_YEARS) return *why = "n_years above LT_MAX_YEARS", LT_ERR_LIMIT;
  if (in->n_pix > LT_MAX_TILE_PIX) return *why = "n_pix above LT_MAX_TILE_PIX", LT_ERR_LIMIT;
  if (in->n_years > 0 && (!in->val_fit || !in->vertex || !in->year))
    return *why = "val_fit / vertex planes and year required", LT_ERR_ARG;
  if (in->stride < in->n_pix || out->stride < in->n_pix)
    return *why = "stride or out->stride below n_pix", LT_ERR_ARG;
  if (in->present && in->winner) return *why = "at most one of present / winner", LT_ERR_ARG;
  if ((out->rmse || out->n_fit || out->dsnr) && !(in->val_raw && in->spike))
    return *why = "rmse / n_fit / dsnr need val_raw and spike", LT_ERR_ARG;
  for (int m = 0; m < n_maps; m++) {
    const lt_change_rule& r = rules[m];
    if (r.delta != LT_CM_LOSS && r.delta != LT_CM_GAIN) return *why = "delta", LT_ERR_ARG;
    if (r.sort < LT_CS_GREATEST || r.sort > LT_CS_GENTLEST) return *why = "sort", LT_ERR_ARG;
    if (r.index_sign != 1 && r.index_sign != -1) return *why = "index_sign", LT_ERR_ARG;
    if (!change_op_ok(r.mag_op) || !change_op_ok(r.dur_op) || !change_op_ok(r.pre_op))
      return *why = "filter op", LT_ERR_ARG;
    if (r.year_set && r.year_lo > r.year_hi) return *why = "year_lo above year_hi", LT_ERR_ARG;
  }
  return LT_OK;
}

template <int M>
inline void change_args(const lt_change_in* in, int n_maps, const lt_change_rule* rules,
                        const lt_change_out* out, ChangeArgs<M>& A) {
  A.in = *in;
  A.out = *out;
  A.n_maps = n_maps;
  A.want_fit = (out->rmse || out->n_fit || out->dsnr) ? 1 : 0;
  for (int y = 0; y < LT_MAX_YEARS; y++) A.year[y] = y < in->n_years ? in->year[y] : 0;
  for (int m = 0; m < M; m++) A.rule[m] = rules[m < n_maps ? m : 0];
}

// a filter: true iff the comparison that is set holds (a NaN operand makes it false)
__host__ __device__ inline bool change_cmp(int32_t op, double a, double v) {
  return op == LT_Q_UNSET ? true
       : op == LT_Q_GT    ? a > v
       : op == LT_Q_LT    ? a < v
       : op == LT_Q_GE    ? a >= v
                          : a <= v;
}

// One pixel. The year loop runs Y times for every lane; the flag, presence and spike rows are read
// by every lane (1-2 B each, a coalesced row), val_raw only with want_fit (a uniform branch),
// val_fit then at every fitted point and otherwise only where the lane has a vertex.
template <int M>
__host__ __device__ inline void change_pixel(const ChangeArgs<M>& A, int64_t p) {
  const int64_t is = A.in.stride, os = A.out.stride;
  const int Y = A.in.n_years;
  const bool want_fit = A.want_fit != 0;
  int32_t byear[M], bdur[M];
  double bmag[M], bpre[M], brate[M];
  uint32_t found = 0;
#pragma unroll
  for (int m = 0; m < M; m++) {
    byear[m] = bdur[m] = 0;
    bmag[m] = bpre[m] = brate[m] = 0.0;
  }
  bool open = false;   // a left vertex is held
  int32_t yl = 0;
  double fl = 0.0;
  double acc = 0.0;
  int32_t n_fit = 0;
  for (int y = 0; y < Y; y++) {
    const int64_t q = (int64_t)y * is + p;
    const bool pres = A.in.present ? A.in.present[q] != 0
                                   : (A.in.winner ? A.in.winner[q] >= 0 : true);
    if (!pres) continue;
    const bool vert = A.in.vertex[q] != 0 || !open;
    double f = 0.0;
    bool have_f = false;
    if (want_fit && A.in.spike[q] == 0) {
      f = A.in.val_fit[q];
      have_f = true;
      const double r = A.in.val_raw[q] - f;
      const double rr = r * r;
      acc = acc + rr;
      n_fit++;
    }
    if (!vert) continue;
    if (!have_f) f = A.in.val_fit[q];
    const int32_t yr = A.year[y];
    if (open) {  // the segment (yl, fl) -> (yr, f) closes
      const int32_t dur = yr - yl;
      const double d = fl - f;
      const double mag = __builtin_fabs(d);
      const double rate = mag / (double)dur;
      // the rules are read from the kernel argument as each segment closes (scalar loads of a
      // few cached lines): held across the year loop, eight rules' 128 words would not fit the
      // scalar registers beside the plane pointers
      int at = 0;
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" : "+s"(at));
#endif
#pragma unroll
      for (int m = 0; m < M; m++) {
        if (m >= A.n_maps) continue;
        const lt_change_rule& R = A.rule[m + at];
        const double sd = R.index_sign > 0 ? d : -d;
        bool keep = R.delta == LT_CM_LOSS ? sd > 0.0 : sd < 0.0;
        keep = keep && (!R.year_set || (R.year_lo <= yl && yl <= R.year_hi));
        keep = keep && change_cmp(R.mag_op, mag, R.mag_val);
        keep = keep && change_cmp(R.dur_op, (double)dur, R.dur_val);
        keep = keep && change_cmp(R.pre_op, fl, R.pre_val);
        bool better;
        switch (R.sort) {
          case LT_CS_GREATEST: better = mag > bmag[m]; break;
          case LT_CS_LEAST: better = mag < bmag[m]; break;
          case LT_CS_NEWEST: better = yl > byear[m]; break;
          case LT_CS_OLDEST: better = yl < byear[m]; break;
          case LT_CS_LONGEST: better = dur > bdur[m]; break;
          case LT_CS_SHORTEST: better = dur < bdur[m]; break;
          case LT_CS_STEEPEST: better = rate > brate[m]; break;
          default: better = rate < brate[m]; break;
        }
        if (keep && (!(found & (1u << m)) || better)) {
          found |= 1u << m;
          byear[m] = yl;
          bdur[m] = dur;
          bmag[m] = mag;
          bpre[m] = fl;
          brate[m] = rate;
        }
      }
    }
    open = true;
    yl = yr;
    fl = f;
  }
  double rmse = (double)LT_NODATA;
  if (want_fit) {
    if (n_fit > 0) rmse = __builtin_sqrt(acc / (double)n_fit);
    if (A.out.rmse) A.out.rmse[p] = rmse;
    if (A.out.n_fit) A.out.n_fit[p] = n_fit;
  }
#pragma unroll
  for (int m = 0; m < M; m++) {
    if (m >= A.n_maps) continue;
    const int64_t o = (int64_t)m * os + p;
    const bool hit = (found & (1u << m)) != 0;
    const double nd = (double)LT_NODATA;
    if (A.out.matched) A.out.matched[o] = hit ? 1 : 0;
    if (A.out.onset_year) A.out.onset_year[o] = hit ? byear[m] : LT_NODATA;
    if (A.out.duration) A.out.duration[o] = hit ? bdur[m] : LT_NODATA;
    if (A.out.magnitude) A.out.magnitude[o] = hit ? bmag[m] : nd;
    if (A.out.preval) A.out.preval[o] = hit ? bpre[m] : nd;
    if (A.out.rate) A.out.rate[o] = hit ? brate[m] : nd;
    if (A.out.dsnr) A.out.dsnr[o] = (hit && n_fit > 0) ? bmag[m] / rmse : nd;
  }
}

// ---- lt_label_counts ----

constexpr int kCountMaxBins = 256;

inline int counts_check(const uint8_t* matched, const int32_t* key, int64_t n_pix, int32_t n_bins,
                        const uint64_t* counts, const char** why) {
  *why = "";
  if (n_pix < 0) return *why = "negative n_pix", LT_ERR_ARG;
  if (n_pix == 0) return LT_OK;
  if (!matched || !key || !counts) return *why = "null argument", LT_ERR_ARG;
  if (n_bins < 1 || n_bins > kCountMaxBins) return *why = "n_bins outside [1, 256]", LT_ERR_ARG;
  if (n_pix > LT_MAX_TILE_PIX) return *why = "n_pix above LT_MAX_TILE_PIX", LT_ERR_LIMIT;
  return LT_OK;
}

// the bin of one pixel: -1 unmatched, k for key == key_lo + k, n_bins for a key outside the range
__host__ __device__ inline int count_bin(uint8_t matched, int32_t key, int32_t key_lo,
                                         int32_t n_bins) {
  if (matched == 0) return -1;
  const int64_t k = (int64_t)key - (int64_t)key_lo;
  return (k >= 0 && k < n_bins) ? (int)k : n_bins;
}

}  // namespace lt
