// Host-side harness for the lazy DP's two entry orders (land_trendr_amd/csrc/lt_pixel.h dp_lazy,
// LT_DP_SEED). TEST INFRASTRUCTURE: compiles the __host__ __device__ code for the CPU, so
// tests/test_dp_seed.py can run both orders side by side against the exact-OPT DP without a GPU.
// Built by __graft_entry__.build() into tests/native/build/liblt_dpseedcheck.so. Not part of the
// product (which has no CPU path).
#include <string.h>

#include "../../land_trendr_amd/csrc/lt_pixel.h"

// The lazy DP on one compacted series, the group entered at the end of the column (seed = 0) or
// seeded into the trackers after the 1- and 2-point starts (seed = 1): returns the
// ambiguous-column mask, fills the argmins and whether the series goes to the exact-OPT DP.
extern "C" uint64_t ltx_dp_lazy_order(int n, const uint8_t* xs, const double* ys, double c,
                                      uint8_t* arg, int* deferred, int seed) {
  uint64_t amb = 0;
  *deferred = seed ? !lt::dp_lazy<64, true>(n, xs, ys, c, arg, &amb)
                   : !lt::dp_lazy<64, false>(n, xs, ys, c, arg, &amb);
  return amb;
}

// The order the library's default build takes (LT_DP_SEED)
extern "C" int ltx_dp_seed_default() { return LT_DP_SEED != 0; }

// The exact-OPT DP (dp_screened) on one compacted series: the argmin of every column.
extern "C" int ltx_dp_exact(int n, const uint8_t* xs, const double* ys, double c, uint8_t* arg) {
  double OPT[65];
  OPT[0] = 0.0;
  int status = 0;
  lt::dp_screened<64>(n, xs, ys, c, OPT, arg, status);
  return status;
}
