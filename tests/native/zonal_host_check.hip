// Host twin of the zonal-table kernels (land_trendr_amd/csrc/lt_zonal.h, lt_zonal.hip).
// TEST INFRASTRUCTURE: compiles the exact __host__ __device__ per-pixel code the kernels run and
// the entry point's argument checks for the CPU, so tests/test_zonal_host.py can check every case
// of lt_zonal_stats against the independent reference of tests/zonalfixture.py without a GPU, and
// the job's CPU tests have a zonal_stats to call. Built by __graft_entry__.build() into
// tests/native/build/liblt_zonalcheck.so. Not part of the product (which has no CPU path).
#include "../../land_trendr_amd/csrc/lt_zonal.h"

// lt_zonal_stats over host arrays: every pointer a HOST pointer. Returns LT_OK, or the LT_ERR_*
// lt_zonal_stats gives for these arguments. The pixels are added one at a time in index order;
// the sums are unsigned 64-bit, as the kernels'.
extern "C" int ltx_zonal_stats(const uint8_t* matched, const int32_t* zone, const int32_t* key,
                               const int32_t* duration, const double* value, int64_t n_pix,
                               int32_t key_lo, int32_t n_bins, int32_t n_zones, int32_t path,
                               uint64_t* table) {
  const char* why;
  const int rc = lt::zonal_check(matched, zone, key, n_pix, n_bins, n_zones, path, table, &why);
  if (rc != LT_OK || n_pix == 0) return rc;
  const lt::ZonalArgs A = {matched, zone, key, duration, value, n_pix, key_lo, n_bins, n_zones,
                           (unsigned long long*)table};
  for (int64_t p = 0; p < n_pix; p++) {
    const lt::ZonalPix x = lt::zonal_pixel(A, p);
    if (x.cell < 0) continue;
    uint64_t* w = table + (int64_t)x.cell * lt::kZonalWords;
    w[0] += 1;
    w[1] += (uint64_t)x.dur;
    w[2] += (uint64_t)x.q;
    w[3] += (uint64_t)x.has_value;
  }
  return LT_OK;
}

// the path a call with path == 0 takes (1 or 2)
extern "C" int ltx_zonal_path(int32_t path, int32_t n_zones, int32_t n_bins) {
  return lt::zonal_path(path, n_zones, n_bins);
}
