// Host-side harness for the x-set factor table's maps (land_trendr_amd/csrc/lt_lapack.h).
// TEST INFRASTRUCTURE: xset_key (the slot lsq_lockstep loads for a segment's x values),
// xset_of_key (the x-set build_xtable_kernel fills a slot from, lt_abi.hip) and lsq_factor (what
// the slot stores), one x-set at a time, compiled for the CPU: tests/test_span_host.py enumerates
// the x-sets. Built by __graft_entry__.build() into tests/native/build/liblt_xsetcheck.so. Not
// part of the product.
#include <string.h>

#include "../../land_trendr_amd/csrc/lt_lapack.h"

// the slot of xs[0..m-1], or -1
extern "C" int ltx_xset_key(int m, const int* xs) {
  return lt::xset_key(m, [&](int k) { return xs[k]; });
}

// the x-set of slot idx into *m and xs[0..63]; 0 for a slot no x-set maps to
extern "C" int ltx_xset_of_key(int idx, int* m, int* xs) {
  *m = 0;
  return lt::xset_of_key(idx, *m, xs) ? 1 : 0;
}

extern "C" int ltx_xset_table_size() { return lt::kXtSize; }

extern "C" int ltx_lsq_xf_size() { return (int)sizeof(lt::lsq_xf); }

// lsq_factor of xs[0..m-1] into out (ltx_lsq_xf_size() bytes, cleared first); returns its rc
extern "C" int ltx_lsq_factor(int m, const int* xs, void* out) {
  lt::lsq_xf f;
  memset(&f, 0, sizeof f);
  lt::lsq_factor(m, [&](int k) { return xs[k]; }, f);
  memcpy(out, &f, sizeof f);
  return f.rc;
}
