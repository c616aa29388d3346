// lt_change.hip — the change maps on the device (lt_abi.h lt_change_maps) and the per-key count of
// a label plane (lt_label_counts).
//
// The per-pixel logic is lt_change.h, the source tests/native/change_host_check.hip compiles for
// the host. A lane is a pixel, 256 lanes a block: the flag, presence and spike rows of a year are
// read by neighbouring lanes (coalesced, 1-2 B per lane), the binary64 values where the lane needs
// them, and all n_maps maps are evaluated in the one pass, their state in registers: the kernel is
// instantiated for 1, 2, 4 and 8 maps with the map loop unrolled, and the smallest instance that
// holds n_maps is launched. The years and the rules travel in the kernel argument. No LDS, no
// scratch. Nothing here waits for the device.
//
// lt_label_counts: a block-local LDS histogram of n_bins + 1 words, then one 64-bit atomic add per
// non-empty bin per block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lt_abi.h"
#include "lt_change.h"
#include "lt_launch.h"

namespace {

constexpr int kBlock = 256;

template <int M>
__global__ __launch_bounds__(kBlock) void change_kernel(const lt::ChangeArgs<M> A) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= A.in.n_pix) return;
  lt::change_pixel<M>(A, p);
}

template <int M>
hipError_t launch_change(const lt_change_in* in, int n_maps, const lt_change_rule* rules,
                         const lt_change_out* out, hipStream_t stream) {
  lt::ChangeArgs<M> A;
  lt::change_args<M>(in, n_maps, rules, out, A);
  const unsigned blocks = (unsigned)((in->n_pix + kBlock - 1) / kBlock);  // <= 2^20
  hipLaunchKernelGGL(change_kernel<M>, dim3(blocks), dim3(kBlock), 0, stream, A);
  return hipGetLastError();
}

// each block counts a run of kCountPerBlock pixels (a multiple of the block, below 2^32, so the
// LDS words cannot wrap) and adds its non-empty bins to the 64-bit totals
constexpr int64_t kCountPerBlock = 256 * 64;

__global__ __launch_bounds__(kBlock) void counts_kernel(const uint8_t* matched, const int32_t* key,
                                                        int64_t n_pix, int32_t key_lo,
                                                        int32_t n_bins,
                                                        unsigned long long* counts) {
  __shared__ unsigned int hist[lt::kCountMaxBins + 1];
  for (int b = threadIdx.x; b <= n_bins; b += kBlock) hist[b] = 0;
  __syncthreads();
  const int64_t p0 = (int64_t)blockIdx.x * kCountPerBlock;
  const int64_t p1 = p0 + kCountPerBlock < n_pix ? p0 + kCountPerBlock : n_pix;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += kBlock) {
    const int b = lt::count_bin(matched[p], key[p], key_lo, n_bins);
    if (b >= 0) atomicAdd(&hist[b], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b <= n_bins; b += kBlock) {
    const unsigned int n = hist[b];
    if (n != 0) atomicAdd(&counts[b], (unsigned long long)n);
  }
}

}  // namespace

extern "C" int lt_change_maps(lt_ctx* c, const lt_change_in* in, int n_maps,
                              const lt_change_rule* rules, const lt_change_out* out,
                              void* stream_) {
  if (!c) return LT_ERR_ARG;
  const char* why;
  const int rc = lt::change_check(in, n_maps, rules, out, &why);
  if (rc != LT_OK) return lt::ctx_fail(c, rc, "lt_change_maps: %s", why);
  if (in->n_pix == 0) return LT_OK;  // nothing is read or written
  hipError_t e = hipSetDevice(lt::ctx_device(c));
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  hipStream_t stream = (hipStream_t)stream_;
  switch (lt::change_instance(n_maps)) {
    case 1: e = launch_change<1>(in, n_maps, rules, out, stream); break;
    case 2: e = launch_change<2>(in, n_maps, rules, out, stream); break;
    case 4: e = launch_change<4>(in, n_maps, rules, out, stream); break;
    default: e = launch_change<8>(in, n_maps, rules, out, stream); break;
  }
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "change_kernel: %s", hipGetErrorString(e));
  return LT_OK;
}

extern "C" int lt_label_counts(lt_ctx* c, const uint8_t* matched, const int32_t* key,
                               int64_t n_pix, int32_t key_lo, int32_t n_bins, uint64_t* counts,
                               void* stream_) {
  if (!c) return LT_ERR_ARG;
  const char* why;
  const int rc = lt::counts_check(matched, key, n_pix, n_bins, counts, &why);
  if (rc != LT_OK) return lt::ctx_fail(c, rc, "lt_label_counts: %s", why);
  if (n_pix == 0) return LT_OK;
  hipError_t e = hipSetDevice(lt::ctx_device(c));
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  const unsigned blocks = (unsigned)((n_pix + kCountPerBlock - 1) / kCountPerBlock);
  hipLaunchKernelGGL(counts_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream_, matched,
                     key, n_pix, key_lo, n_bins, (unsigned long long*)counts);
  e = hipGetLastError();
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "counts_kernel: %s", hipGetErrorString(e));
  return LT_OK;
}
