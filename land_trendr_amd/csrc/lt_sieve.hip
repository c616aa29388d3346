// lt_sieve.hip — the MMU sieve on the device (lt_abi.h lt_sieve_labels): connected-component
// labelling of one rule's label plane by union-find, and the clear of the patches below the
// minimum mapping unit.
//
// The phase bodies are lt_sieve.h, the source tests/native/sieve_host_check.hip compiles for the
// host. Four launches on the caller's stream and nothing between them: a local phase (one block
// per 64 x 16 tile, unions in 8 KiB of LDS), the border merge (one lane per tile-border pixel,
// atomicMin links on the global parent array, every access to it there an agent-scope atomic), the
// resolve of every local root (one counter add per local component) and the expand. No workgroup
// waits for another, and every loop is bounded by the decreasing-parent argument in lt_sieve.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lt_abi.h"
#include "lt_launch.h"
#include "lt_sieve.h"

namespace {

using lt::kSvBlock;

__global__ __launch_bounds__(kSvBlock) void sieve_local_kernel(const lt::SieveArgs A) {
  __shared__ lt::SieveShared S;
  const int64_t b = blockIdx.x;
  const int l = threadIdx.x;
  lt::sieve_local_load(A, b, l, S);
  __syncthreads();
  lt::sieve_local_unite(A, l, S);
  __syncthreads();
  lt::sieve_local_flatten(l, S);
  __syncthreads();
  lt::sieve_local_count(l, S);
  __syncthreads();
  lt::sieve_local_store(A, b, l, S);
}

__global__ __launch_bounds__(kSvBlock) void sieve_merge_kernel(const lt::SieveArgs A) {
  lt::sieve_merge(A, (int64_t)blockIdx.x * kSvBlock + threadIdx.x);
}

__global__ __launch_bounds__(kSvBlock) void sieve_resolve_kernel(const lt::SieveArgs A) {
  lt::sieve_resolve(A, (int64_t)blockIdx.x * kSvBlock + threadIdx.x);
}

__global__ __launch_bounds__(kSvBlock) void sieve_expand_kernel(const lt::SieveArgs A) {
  lt::sieve_expand(A, (int64_t)blockIdx.x * kSvBlock + threadIdx.x);
}

}  // namespace

extern "C" int64_t lt_sieve_workspace_bytes(int64_t rows, int64_t cols) {
  return lt::sieve_workspace_bytes(rows, cols);
}

extern "C" int lt_sieve_labels(lt_ctx* c, const lt_sieve_in* in, const lt_sieve_out* out,
                               void* stream_) {
  if (!c) return LT_ERR_ARG;
  const char* why;
  const int rc = lt::sieve_check(in, out, &why);
  if (rc != LT_OK) return lt::ctx_fail(c, rc, "lt_sieve_labels: %s", why);
  if (in->rows == 0 || in->cols == 0) return LT_OK;  // nothing is read or written
  lt::SieveArgs A;
  lt::sieve_args(in, out, A);
  hipError_t e = hipSetDevice(lt::ctx_device(c));
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  hipStream_t st = (hipStream_t)stream_;
  // tiles <= 2^28 (a 1-column raster: a tile per 16 rows), border lanes <= 94 * 2^28 / 256 blocks
  const int64_t T = lt::sieve_tiles(A), P = lt::sieve_pixels(A);
  const unsigned mb = (unsigned)((T * lt::kSvBorder + kSvBlock - 1) / kSvBlock);
  const unsigned pb = (unsigned)((P + kSvBlock - 1) / kSvBlock);
  const int ph = in->phases ? in->phases : 15;  // (a timing tool runs them one by one)
  if (ph & 1) hipLaunchKernelGGL(sieve_local_kernel, dim3((unsigned)T), dim3(kSvBlock), 0, st, A);
  if (ph & 2) hipLaunchKernelGGL(sieve_merge_kernel, dim3(mb), dim3(kSvBlock), 0, st, A);
  if (ph & 4) hipLaunchKernelGGL(sieve_resolve_kernel, dim3(pb), dim3(kSvBlock), 0, st, A);
  if (ph & 8) hipLaunchKernelGGL(sieve_expand_kernel, dim3(pb), dim3(kSvBlock), 0, st, A);
  e = hipGetLastError();
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "sieve kernels: %s", hipGetErrorString(e));
  return LT_OK;
}
