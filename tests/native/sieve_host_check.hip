// Host twin of the MMU sieve kernels (land_trendr_amd/csrc/lt_sieve.h, lt_sieve.hip).
// TEST INFRASTRUCTURE: compiles the exact __host__ __device__ phase steps the kernels run, and the
// entry point's argument checks, for the CPU: each step over a block's lanes in turn, block after
// block, forwards or backwards, so tests/test_sieve_host.py can check every case of
// lt_sieve_labels against the pixel-pair reference of tests/sievefixture.py without a GPU, and the
// GPU tests have a fast expectation for their large scenes. Built by __graft_entry__.build() into
// tests/native/build/liblt_sievecheck.so. Not part of the product (which has no CPU path).
#include "../../land_trendr_amd/csrc/lt_sieve.h"

// lt_sieve_labels over host planes: the same structs, every pointer a HOST pointer. reverse != 0
// runs the blocks of every launch from the last to the first. Returns LT_OK, or the LT_ERR_*
// lt_sieve_labels gives for these arguments.
extern "C" int ltx_sieve_labels(const lt_sieve_in* in, const lt_sieve_out* out, int reverse) {
  const char* why;
  const int rc = lt::sieve_check(in, out, &why);
  if (rc != LT_OK || in->rows == 0 || in->cols == 0) return rc;
  lt::SieveArgs A;
  lt::sieve_args(in, out, A);
  lt::sieve_host(A, reverse != 0);
  return LT_OK;
}

extern "C" int64_t ltx_sieve_workspace_bytes(int64_t rows, int64_t cols) {
  return lt::sieve_workspace_bytes(rows, cols);
}
