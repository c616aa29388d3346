// Host twin of the change-map kernels (land_trendr_amd/csrc/lt_change.h, lt_change.hip).
// TEST INFRASTRUCTURE: compiles the exact __host__ __device__ per-pixel code the kernels run, the
// entry points' argument checks and the instance choice for the CPU, so tests/test_change_host.py
// can check every semantic case of lt_change_maps and lt_label_counts against the independent
// reference of tests/changefixture.py without a GPU, and the job's CPU tests have a change_maps to
// call. Built by __graft_entry__.build() into tests/native/build/liblt_changecheck.so. Not part of
// the product (which has no CPU path).
#include "../../land_trendr_amd/csrc/lt_change.h"

template <int M>
static void run(const lt_change_in* in, int n_maps, const lt_change_rule* rules,
                const lt_change_out* out) {
  lt::ChangeArgs<M> A;
  lt::change_args<M>(in, n_maps, rules, out, A);
  for (int64_t p = 0; p < in->n_pix; p++) lt::change_pixel<M>(A, p);
}

// lt_change_maps over host planes: the same structs, every pointer a HOST pointer. Returns LT_OK,
// or the LT_ERR_* lt_change_maps gives for these arguments.
extern "C" int ltx_change_maps(const lt_change_in* in, int n_maps, const lt_change_rule* rules,
                               const lt_change_out* out) {
  const char* why;
  const int rc = lt::change_check(in, n_maps, rules, out, &why);
  if (rc != LT_OK || in->n_pix == 0) return rc;
  switch (lt::change_instance(n_maps)) {
    case 1: run<1>(in, n_maps, rules, out); break;
    case 2: run<2>(in, n_maps, rules, out); break;
    case 4: run<4>(in, n_maps, rules, out); break;
    default: run<8>(in, n_maps, rules, out); break;
  }
  return LT_OK;
}

// lt_label_counts over host arrays.
extern "C" int ltx_label_counts(const uint8_t* matched, const int32_t* key, int64_t n_pix,
                                int32_t key_lo, int32_t n_bins, uint64_t* counts) {
  const char* why;
  const int rc = lt::counts_check(matched, key, n_pix, n_bins, counts, &why);
  if (rc != LT_OK || n_pix == 0) return rc;
  for (int64_t p = 0; p < n_pix; p++) {
    const int b = lt::count_bin(matched[p], key[p], key_lo, n_bins);
    if (b >= 0) counts[b]++;
  }
  return LT_OK;
}
