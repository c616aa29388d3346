// lt_vertex.hip — the vertex table on the device (lt_abi.h lt_vertex_table): each pixel's vertices
// compacted from its per-year planes into [V][stride] planes of year / val_fit / val_raw and a
// count.
//
// The per-pixel logic is lt_vertex.h, the source tests/native/vertex_host_check.hip compiles for
// the host. A lane is a pixel: the flag and presence rows of a year are read by neighbouring lanes
// (coalesced, 1-2 B per lane), the binary64 values only by the lanes that have a vertex there, and
// each vertex goes to the lane's own row, out[n_lane * stride + p]: lanes whose counters agree
// store neighbouring words, and every word of a wave's 64 pixels in every row is written within
// the launch (by a vertex or by the trailing fill), so the lines are completed in the L2. Nothing
// here waits for the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lt_abi.h"
#include "lt_launch.h"
#include "lt_vertex.h"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void vertex_kernel(const lt::VertexArgs A) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= A.in.n_pix) return;
  lt::vertex_pixel(A, p);
}

}  // namespace

extern "C" int lt_vertex_table(lt_ctx* c, const lt_vertex_in* in, const lt_vertex_out* out,
                               void* stream_) {
  if (!c) return LT_ERR_ARG;
  const char* why;
  const int rc = lt::vertex_check(in, out, &why);
  if (rc != LT_OK) return lt::ctx_fail(c, rc, "lt_vertex_table: %s", why);
  if (in->n_pix == 0) return LT_OK;  // nothing is read or written
  lt::VertexArgs A;
  lt::vertex_args(in, out, A);
  hipError_t e = hipSetDevice(lt::ctx_device(c));
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  const unsigned blocks = (unsigned)((in->n_pix + kBlock - 1) / kBlock);  // <= 2^20
  hipLaunchKernelGGL(vertex_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream_, A);
  e = hipGetLastError();
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "vertex_kernel: %s", hipGetErrorString(e));
  return LT_OK;
}
