// lt_zonal.h — the zonal table's per-pixel code (lt_abi.h lt_zonal_stats), host and device: one
// source for the kernels (lt_zonal.hip), for their host twin (tests/native/zonal_host_check.hip)
// and for the sanitized program (tests/native/zonal_core_check.cpp).
//
// The table is [n_zones + 1][n_bins + 1][4] 64-bit words. A matched pixel's row is its zone index
// (the last row for an index outside [0, n_zones)), its column count_bin's (key - key_lo, the last
// column for a key outside the range), and it adds 1, its duration, its magnitude in 1/16ths and 1
// to the cell's four words. Every word is a two's-complement sum made with unsigned 64-bit adds,
// so a table is a function of the input alone, whatever order the adds arrive in.
//
// Bounds of one call (n_pix <= LT_MAX_TILE_PIX = 2^28): word 0 and word 3 <= 2^28, |word 1| <=
// 2^28 * 2^31 = 2^59, |word 2| <= 2^28 * 2^34 = 2^62: no word can wrap within one call on a zeroed
// table. A caller that accumulates several calls into one table owns that bound.
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

constexpr int kZonalMaxBins = 256;
constexpr int kZonalWords = 4;  // per cell: pixels, duration sum, magnitude sum * 16, magnitudes
// lt_zonal_stats' path argument
constexpr int kZonalAuto = 0, kZonalLds = 1, kZonalWave = 2;
// The block-private table of the LDS path holds at most this many cells: 1024 cells of four
// 64-bit words are 32 KB, so five blocks of 256 lanes (20 waves) share a CU's 160 KB. The kernel
// streams 21 bytes a pixel and does little with them, so what it needs is loads in flight: five
// waves a SIMD, each with its five plane loads outstanding, and a table this size (33 zones over
// 30 years) covers the class rasters (ownership, land cover) the path is for. The LDS is sized by
// the call's own cell count, so a smaller table leaves room for more blocks. (Reasoned, not
// measured: no time of the kernel has been taken yet, DESIGN.md § Zonal tables.)
constexpr int kZonalLdsCells = 1024;

// what the kernels are launched with (uniform: read with scalar loads)
struct ZonalArgs {
  const uint8_t* matched;
  const int32_t* zone;
  const int32_t* key;
  const int32_t* duration;  // or null
  const double* value;      // or null
  int64_t n_pix;
  int32_t key_lo, n_bins, n_zones;
  unsigned long long* table;
};

inline int64_t zonal_cells(int32_t n_zones, int32_t n_bins) {
  return ((int64_t)n_zones + 1) * ((int64_t)n_bins + 1);
}

// the argument checks of lt_zonal_stats, shared with the host twin: LT_OK or the LT_ERR_* code and
// what to say (n_pix == 0 is LT_OK: the caller returns before it launches anything)
inline int zonal_check(const uint8_t* matched, const int32_t* zone, const int32_t* key,
                       int64_t n_pix, int32_t n_bins, int32_t n_zones, int32_t path,
                       const uint64_t* table, const char** why) {
  *why = "";
  if (n_pix < 0) return *why = "negative n_pix", LT_ERR_ARG;
  if (n_pix == 0) return LT_OK;
  if (!matched || !zone || !key || !table) return *why = "null argument", LT_ERR_ARG;
  if (n_bins < 1 || n_bins > kZonalMaxBins) return *why = "n_bins outside [1, 256]", LT_ERR_ARG;
  if (n_zones < 1 || n_zones > LT_MAX_ZONES)
    return *why = "n_zones outside [1, LT_MAX_ZONES]", LT_ERR_ARG;
  if (path < kZonalAuto || path > kZonalWave) return *why = "path outside [0, 2]", LT_ERR_ARG;
  if (path == kZonalLds && zonal_cells(n_zones, n_bins) > kZonalLdsCells)
    return *why = "path 1 needs (n_zones + 1) * (n_bins + 1) <= 1024", LT_ERR_ARG;
  if (n_pix > LT_MAX_TILE_PIX) return *why = "n_pix above LT_MAX_TILE_PIX", LT_ERR_LIMIT;
  return LT_OK;
}

// the path a call takes
inline int zonal_path(int32_t path, int32_t n_zones, int32_t n_bins) {
  if (path != kZonalAuto) return path;
  return zonal_cells(n_zones, n_bins) <= kZonalLdsCells ? kZonalLds : kZonalWave;
}

// one pixel's cell and addends
struct ZonalPix {
  int32_t cell;       // row * (n_bins + 1) + column (< 65537 * 257 < 2^25), -1 unmatched
  int32_t has_value;  // words 2 and 3 are added to
  int64_t dur;        // word 1's addend (0 without a duration plane)
  int64_t q;          // word 2's addend
};

// the magnitude in 1/16ths: clamped to +-2^30 (so +-inf clamp), times 16 (exact: a power of two,
// no overflow), rounded half to even; |q| <= 2^34. NaN is the caller's to skip.
__host__ __device__ inline int64_t zonal_fixed(double v) {
  const double lim = 1073741824.0;
  const double c = v < -lim ? -lim : (v > lim ? lim : v);
  return (int64_t)__builtin_rint(c * 16.0);
}

__host__ __device__ inline ZonalPix zonal_pixel(const ZonalArgs& A, int64_t p) {
  ZonalPix x;
  x.cell = -1;
  x.has_value = 0;
  x.dur = x.q = 0;
  if (A.matched[p] == 0) return x;
  const int32_t z = A.zone[p];
  const int32_t row = (z >= 0 && z < A.n_zones) ? z : A.n_zones;
  const int64_t k = (int64_t)A.key[p] - (int64_t)A.key_lo;
  const int32_t col = (k >= 0 && k < A.n_bins) ? (int32_t)k : A.n_bins;
  x.cell = row * (A.n_bins + 1) + col;
  if (A.duration) x.dur = (int64_t)A.duration[p];
  if (A.value) {
    const double v = A.value[p];
    if (v == v) {
      x.has_value = 1;
      x.q = zonal_fixed(v);
    }
  }
  return x;
}

}  // namespace lt
