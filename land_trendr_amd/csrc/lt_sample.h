// lt_sample.h — a raster sampled at the grid points of a job in raster order, compiled for the
// host (g++: lt_io.cpp's lt_grid_sample) and for the device (hipcc: lt_sample.hip,
// lt_grid_sample_dev).
//
// The reference samples every raster and every cloud mask at the template's grid points
// (apply_grid / pt2val, utils.py:285-297, 328-359): raster_array[y_off, x_off] per point, numpy's
// negative-index wrap, the point skipped where that raises. In raster order grid point (r, c) has
// the coordinates (xv[c], yv[r]), so x_off depends on c alone and y_off on r alone: the host makes
// the two offset axes (ingest.axis_offsets: wrapped, -1 where pt2val raises) and what is left is an
// integer gather, one plane per selected band, with the validity byte written beside it:
//   BANDS  out[b][i] = on ? src[sel[b]][yoff[r] * src_w + xoff[c]] : 0;  valid[i] = on
//   MASK   valid[i] &= !(on && the sample of band sel[0] is all zero bytes)
// for grid pixel p = p0 + i, r = p / grid_w, c = p % grid_w, on = both offsets inside the source.
// An offset outside [0, src_w) / [0, src_h) counts as off the raster, whatever the caller uploaded:
// nothing outside `src` is ever read.
//
// Work unit: kGroup consecutive pixels. A grid row's xoff is a run of consecutive columns almost
// everywhere, so a group that lies in one row with such a run moves as one block per plane (the
// source is misaligned by the raster's shift: the loads are sample-aligned only); any other group
// goes pixel by pixel.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LT_SAMPLE_HD __host__ __device__
#else
#define LT_SAMPLE_HD
#endif

#ifndef LT_SAMPLE_WIDE  // 0: every group pixel by pixel (A/B builds of the block path)
#define LT_SAMPLE_WIDE 1
#endif

namespace lt_sample {

constexpr int kGroup = 8;       // pixels per work unit (one 8-byte store of validity bytes)
constexpr int kMaxSel = 16;
constexpr int kBands = 0, kMask = 1;  // LT_SAMPLE_BANDS / LT_SAMPLE_MASK (include/lt_abi.h)

// lt_sample_job (include/lt_abi.h), field for field
struct Args {
  const void* src;
  int32_t bps, src_bands;
  int64_t src_h, src_w;
  const int32_t* xoff;
  const int32_t* yoff;
  int64_t grid_w, grid_h;
  int64_t p0, n;
  int32_t n_sel, sel[kMaxSel];
  void* out;
  int64_t out_stride;
  uint8_t* valid;
  int32_t mode;
};

// What both builds reject before anything runs (LT_ERR_ARG / LT_IO_ERR_ARG): null when the job is
// good, else what is wrong with it.
inline const char* check(const Args& a) {
  constexpr int64_t kMaxDim = (int64_t)1 << 31;
  if (!(a.bps == 1 || a.bps == 2 || a.bps == 4 || a.bps == 8)) return "bps must be 1, 2, 4 or 8";
  if (a.mode != kBands && a.mode != kMask) return "bad mode";
  if (a.n_sel < 1 || a.n_sel > kMaxSel) return "n_sel must be 1..16";
  if (a.src_bands < 1) return "src_bands must be positive";
  for (int b = 0; b < a.n_sel; b++)
    if (a.sel[b] < 0 || a.sel[b] >= a.src_bands) return "sel outside the source's bands";
  if (a.src_h < 0 || a.src_w < 0 || a.grid_w < 0 || a.grid_h < 0 || a.p0 < 0 || a.n < 0)
    return "negative size";
  if (a.src_h >= kMaxDim || a.src_w >= kMaxDim || a.grid_w >= kMaxDim || a.grid_h >= kMaxDim)
    return "rasters of 2^31 or more rows or columns are not taken";
  if (a.p0 > a.grid_w * a.grid_h || a.n > a.grid_w * a.grid_h - a.p0)
    return "p0 + n outside the grid";
  if (a.mode == kBands && a.out_stride < a.n) return "out_stride below n";
  if (a.n > 0 && (!a.src || !a.xoff || !a.yoff || !a.valid || (a.mode == kBands && !a.out)))
    return "null argument";
  if ((uintptr_t)a.src % (uintptr_t)a.bps != 0 ||
      (a.mode == kBands && (uintptr_t)a.out % (uintptr_t)a.bps != 0))
    return "misaligned src or out";
  return nullptr;
}

template <class T>
struct Block {
  T v[kGroup];
};

// kGroup samples from / to a sample-aligned address
template <class T>
LT_SAMPLE_HD inline Block<T> load_block(const T* p) {
  Block<T> b;
  __builtin_memcpy(b.v, p, sizeof(b.v));
  return b;
}
template <class T>
LT_SAMPLE_HD inline void store_block(T* p, const Block<T>& b) {
  __builtin_memcpy(p, b.v, sizeof(b.v));
}

LT_SAMPLE_HD inline void row_col(const Args& a, int64_t p, int64_t& r, int64_t& c) {
  if ((((uint64_t)p | (uint64_t)a.grid_w) >> 32) == 0) {  // (a 64-bit division is a long one)
    r = (int64_t)((uint32_t)p / (uint32_t)a.grid_w);
    c = (int64_t)((uint32_t)p % (uint32_t)a.grid_w);
  } else {
    r = p / a.grid_w;
    c = p - r * a.grid_w;
  }
}

// pixels [i0, i1) of the job, 0 < i1 - i0 <= kGroup; T: the unsigned type of bps bytes
template <class T>
LT_SAMPLE_HD inline void sample_group(const Args& a, int64_t i0, int64_t i1) {
  const T* const src = (const T*)a.src;
  T* const out = (T*)a.out;
  const int64_t plane = a.src_h * a.src_w;
  int64_t r, c;
  row_col(a, a.p0 + i0, r, c);
#if LT_SAMPLE_WIDE
  if (i1 - i0 == kGroup && c + kGroup <= a.grid_w) {
    const int64_t y = a.yoff[r];
    const int64_t x0 = a.xoff[c];
    bool run = y >= 0 && y < a.src_h && x0 >= 0 && x0 + kGroup <= a.src_w;
    for (int k = 1; k < kGroup; k++) run = run && a.xoff[c + k] == x0 + k;
    if (run) {
      const int64_t at = y * a.src_w + x0;
      if (a.mode == kBands) {
        for (int b = 0; b < a.n_sel; b++)
          store_block(out + b * a.out_stride + i0, load_block(src + a.sel[b] * plane + at));
        Block<uint8_t> one;
        for (int k = 0; k < kGroup; k++) one.v[k] = 1;
        store_block(a.valid + i0, one);
      } else {
        const Block<T> m = load_block(src + a.sel[0] * plane + at);
        Block<uint8_t> v = load_block(a.valid + i0);
        for (int k = 0; k < kGroup; k++) v.v[k] &= (uint8_t)(m.v[k] != 0);
        store_block(a.valid + i0, v);
      }
      return;
    }
  }
#endif
  for (int64_t i = i0; i < i1; i++) {
    const int64_t y = a.yoff[r], x = a.xoff[c];
    const bool on = y >= 0 && y < a.src_h && x >= 0 && x < a.src_w;
    const int64_t at = on ? y * a.src_w + x : 0;
    if (a.mode == kBands) {
      for (int b = 0; b < a.n_sel; b++)
        out[b * a.out_stride + i] = on ? src[a.sel[b] * plane + at] : (T)0;
      a.valid[i] = on ? 1 : 0;
    } else if (on && src[a.sel[0] * plane + at] == 0) {
      a.valid[i] = 0;
    } else {
      a.valid[i] &= 1;
    }
    if (++c == a.grid_w) {
      c = 0;
      r++;
    }
  }
}

// group g of the job: pixels [g * kGroup, min(n, (g + 1) * kGroup))
LT_SAMPLE_HD inline void sample_group_of(const Args& a, int64_t g) {
  const int64_t i0 = g * kGroup;
  const int64_t i1 = i0 + kGroup < a.n ? i0 + kGroup : a.n;
  switch (a.bps) {
    case 1: sample_group<uint8_t>(a, i0, i1); break;
    case 2: sample_group<uint16_t>(a, i0, i1); break;
    case 4: sample_group<uint32_t>(a, i0, i1); break;
    default: sample_group<uint64_t>(a, i0, i1); break;
  }
}

LT_SAMPLE_HD inline int64_t groups(const Args& a) { return (a.n + kGroup - 1) / kGroup; }

}  // namespace lt_sample
