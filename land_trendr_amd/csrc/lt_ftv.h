// lt_ftv.h — fit to vertex (FTV): the segments of an analysis applied to another series.
//
// The analysis finds a pixel's spikes and vertices on one index. FTV takes those planes as given
// (winner / spike / vertex per year slot, as lt_analyze_* wrote them) and the values of a second
// index, and runs the last two steps of the reference's analyze on them:
//   vertices2eqns :646-669        one emulated-dgelsd least squares per pair of consecutive vertices
//   eqns2fitted_points :682-722   the fitted value of every point, as oracle/lt_oracle.c restates it
// (the reference's utils.py). Both take any series and any vertex list, so the result is defined
// bit for bit: val_raw, val_fit, fit_m, fit_b, right_m, right_b of lt_tile_out.
//
// One source for the kernel (lt_ftv.hip: a lane is a pixel, a workgroup is one wave) and for the
// host twin (tests/native/ftv_host_check.hip: a "wave" of one lane). What differs between the two
// is the Wave policy: any (cross-lane on the device, the identity on the host), fit
// (lsq_fit_lockstep on the device; the same lsq_factor + lsq_apply[_small] per lane on the host)
// and store (nontemporal on the device). All arithmetic is the lsq_* functions of lt_lapack.h.
//
// Layout, as lt_fast.h: the fitting series (the non-spike present points) lives in [k][lane]
// planes (LDS on the device), presence / spike / vertex flags in 64-bit masks per lane, every loop
// runs over a wave-uniform counter, and no per-lane array is indexed at run time.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif

#include "../../include/lt_abi.h"
#include "lt_lapack.h"

namespace lt {

// year slots whose plane loads are issued together (then their value gathers, together)
#ifndef LT_FTV_WB
#define LT_FTV_WB 8
#endif

// One launch's arguments (passed by value to the kernel; year[] is read at wave-uniform indices).
struct FtvArgs {
  lt_ftv_in in;
  int64_t os;        // out->stride
  double* val_raw;   // the planes of lt_tile_out that FTV writes, each may be null
  double* val_fit;
  double* fit_m;
  double* fit_b;
  double* right_m;
  double* right_b;
  int32_t* status;
  int32_t n_obs;     // K
  int32_t n_years;   // Y
  int32_t year[LT_MAX_YEARS];
};

// The fitting series of LANES pixels: value and year offset of non-spike point k of each lane.
template <int MAXY, class VT, int LANES>
struct FtvSeries {
  VT ys[MAXY][LANES];
  uint8_t xn[MAXY][LANES];
};

// the second index's value of observation o at pixel p, in the series' storage type
template <class VT>
__host__ __device__ inline VT ftv_value(const lt_ftv_in& in, int64_t o, int64_t p) {
  const int64_t i = o * in.obs_stride + p;
  if constexpr (sizeof(VT) == 2) {
    return ((const int16_t*)in.obs_index)[i];  // an int16 index raster: exact
  } else {
    if (in.obs_index == nullptr) return in.obs_val[i];
    switch (in.index_type) {  // launch-uniform: float(val), utils.py:357
      case LT_T_I16: return (double)((const int16_t*)in.obs_index)[i];
      case LT_T_U16: return (double)((const uint16_t*)in.obs_index)[i];
      case LT_T_I32: return (double)((const int32_t*)in.obs_index)[i];
      case LT_T_F32: return (double)((const float*)in.obs_index)[i];
      case LT_T_U8: return (double)((const uint8_t*)in.obs_index)[i];
      case LT_T_U32: return (double)((const uint32_t*)in.obs_index)[i];
      case LT_T_I8: return (double)((const int8_t*)in.obs_index)[i];
      case LT_T_I64: return (double)((const int64_t*)in.obs_index)[i];
      default: return ((const double*)in.obs_index)[i];
    }
  }
}

// The host twin's Wave: one lane, so the cross-lane steps are the identity, and the fit is what
// lsq_fit_lockstep does for one lane (the x half computed, not looked up: the table holds
// lsq_factor's results).
struct FtvHostWave {
  __host__ __device__ bool any(bool b) const { return b; }
  template <class GX, class GY>
  __host__ __device__ int fit(bool act, int m, GX X, GY Y, double& slope, double& icpt) const {
    slope = 0.0;
    icpt = 0.0;
    if (!act) return 0;
    lsq_xf f;
    lsq_factor(m, X, f);
    double ssr;
    return m > 4 ? lsq_apply(f, X, Y, true, false, slope, icpt, ssr)
                 : lsq_apply_small(f, X, Y, slope, icpt);
  }
  template <class T>
  __host__ __device__ void store(T* at, T v) const { *at = v; }
};

// One pixel per lane: p the pixel, live = p < n_pix (dead lanes load and store nothing but take
// part in every lockstep step). Y <= MAXY, the year span <= 255 and n_obs <= LT_MAX_OBS are the
// caller's to have checked (lt_ftv_tile).
template <int MAXY, class VT, int LANES, class Wave>
__host__ __device__ inline void ftv_pixel(const FtvArgs& A, int64_t p, bool live, int lane,
                                          FtvSeries<MAXY, VT, LANES>& L, const Wave& W) {
  const int Y = A.n_years, K = A.n_obs;
  const int64_t is = A.in.stride, os = A.os;
  const double nan = __builtin_nan("");
  int status = LT_ST_OK;

  // ---- the planes of the analysis and the second index's values of its winners ----
  int T = 0, n = 0;      // present points, non-spike present points
  int32_t y0 = 0;        // the first present year (timeseries2int_series, utils.py:552-554)
  uint64_t pres = 0;     // present year slots
  uint64_t spk = 0;      // spikes, by year slot
  uint64_t vmask = 0;    // vertices, by non-spike index
  constexpr int WB = LT_FTV_WB;
  for (int yb = 0; yb < Y; yb += WB) {  // wave-uniform
    int w[WB];
    uint8_t sf[WB], vf[WB];
#pragma unroll
    for (int j = 0; j < WB; j++) {
      const int y = yb + j;
      w[j] = -1;
      sf[j] = 0;
      vf[j] = 0;
      if (y < Y && live) {
        const int64_t o = (int64_t)y * is + p;
        w[j] = A.in.winner[o];
        sf[j] = A.in.spike[o];
        vf[j] = A.in.vertex[o];
      }
    }
    VT val[WB];
#pragma unroll
    for (int j = 0; j < WB; j++) {
      val[j] = (VT)0;
      if (w[j] < -1 || w[j] >= K) {  // malformed: not an observation; the year counts as absent
        status |= LT_ST_NUMERIC;
        w[j] = -1;
      }
      if (w[j] >= 0) val[j] = ftv_value<VT>(A.in, w[j], p);
    }
#pragma unroll
    for (int j = 0; j < WB; j++) {
      const int y = yb + j;
      if (y >= Y) break;
      const bool pr = w[j] >= 0;
      if (pr) {
        if (T == 0) y0 = A.year[y];
        T++;
        pres |= 1ull << y;
        if (sf[j]) {
          spk |= 1ull << y;
        } else {  // n <= y < MAXY
          L.ys[n][lane] = val[j];
          L.xn[n][lane] = (uint8_t)(A.year[y] - y0);
          if (vf[j]) vmask |= 1ull << n;
          n++;
        }
      }
      // val_raw: the winner's value, spikes included (TrendlinePoint.val_raw); NaN if absent
      if (live && A.val_raw) W.store(A.val_raw + ((int64_t)y * os + p), pr ? (double)val[j] : nan);
    }
  }
  if (live && T == 0) status |= LT_ST_EMPTY;        // the reference raises for these pixels:
  if (live && T == 1) status |= LT_ST_SINGLE_YEAR;  // every fit field NaN, as lt_analyze_* leaves
  const bool good = live && T >= 2;
  // malformed: an analysis leaves at least the first and the last non-spike point as vertices
  if (good && __builtin_popcountll(vmask) < 2) status |= LT_ST_NUMERIC;

  // ---- vertices2eqns + eqns2fitted_points, year-major (lt_fast.h's per-year loop): each year
  // slot is one wave-uniform step and each plane gets one coalesced row. A lane reaching a vertex
  // that has a next vertex needs that segment's fit; the fits run in lockstep and each lane keeps
  // one fit ahead, so a fit step is issued only in a year where some lane reaches such a vertex
  // with its lookahead empty, and in it every lane whose lookahead is free fits its next segment:
  // about one fit step per vertex of the wave's longest lane, not one per year ----
  uint64_t vrem = good ? vmask : 0;  // vertices not reached yet
  uint64_t frem = vrem;              // vertices whose segment is not fitted yet (the lowest next)
  double pm = 0.0, pb = 0.0;         // eqn of the previous vertex
  double cm = 0.0, cb = 0.0;         // eqn of the current vertex: the right eqn of the points
  double nm = 0.0, nb = 0.0;         // lookahead: eqn of the segment from the next vertex
  bool have_n = false;
  int k = 0, q = 0;                  // non-spike index, vertex number
  for (int y = 0; y < Y; y++) {      // wave-uniform
    const bool pr = good && ((pres >> y) & 1);
    const bool sp = pr && ((spk >> y) & 1);
    const bool isv = pr && !sp && ((vrem >> k) & 1);
    const uint64_t after = vrem & (vrem - 1);  // vertices after this one
    const bool nextfit = isv && after != 0;
    double sm = 0.0, sbv = 0.0;
    bool fitnow = false;
    if (W.any(nextfit && !have_n)) {
      const uint64_t fnext = frem & (frem - 1);
      fitnow = fnext != 0 && (!have_n || nextfit);
      const int kbase = fitnow ? __builtin_ctzll(frem) : 0;
      const int kb = fitnow ? __builtin_ctzll(fnext) : 1;
      // segment q: the non-spike points from vertex q to vertex q+1 inclusive
      const int rc = W.fit(
          fitnow, kb - kbase + 1, [&](int i) { return (int)L.xn[kbase + i][lane]; },
          [&](int i) { return (double)L.ys[kbase + i][lane]; }, sm, sbv);
      if (fitnow) {
        if (rc < 0) status |= LT_ST_NUMERIC;
        frem = fnext;
      }
    }
    if (nextfit) {
      pm = cm;
      pb = cb;
      cm = have_n ? nm : sm;
      cb = have_n ? nb : sbv;
      have_n = have_n && fitnow;  // the slot was used: refilled by this year's step
    } else {
      have_n = have_n || fitnow;
    }
    if (have_n && fitnow) {
      nm = sm;
      nb = sbv;
    }
    if (isv && !nextfit) {  // the last vertex takes the previous eqn (utils.py:662)
      pm = cm;
      pb = cb;
    }
    // eqns2fitted_points: the right eqn, or at a vertex where the eqn changes the closer of the
    // left and the right one to the raw value (the left on a tie); (m * x) + b, no FMA
    const double x = (double)(A.year[y] - y0);
    double fv = (cm * x) + cb, fmv = cm, fbv = cb;
    if (isv && q > 0 && !(pm == cm && pb == cb)) {
      const double raw_v = (double)L.ys[k][lane];
      const double fl = (pm * x) + pb;
      if (__builtin_fabs(fl - raw_v) <= __builtin_fabs(fv - raw_v)) {
        fv = fl;
        fmv = pm;
        fbv = pb;
      }
    }
    if (isv) {
      vrem = after;
      q++;
    }
    if (live) {  // absent years and pixels the reference raises for: NaN
      const int64_t o = (int64_t)y * os + p;
      if (A.val_fit) W.store(A.val_fit + o, pr ? fv : nan);
      if (A.fit_m) W.store(A.fit_m + o, pr ? fmv : nan);
      if (A.fit_b) W.store(A.fit_b + o, pr ? fbv : nan);
      if (A.right_m) W.store(A.right_m + o, pr ? cm : nan);
      if (A.right_b) W.store(A.right_b + o, pr ? cb : nan);
    }
    if (pr && !sp) k++;
  }
  if (live && A.status) A.status[p] = status;
}

}  // namespace lt
