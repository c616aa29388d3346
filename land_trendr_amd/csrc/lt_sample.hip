// lt_sample.hip — a decoded raster in device memory sampled at a job's grid points (lt_abi.h
// lt_grid_sample_dev): the gather apply_grid / pt2val do per point (utils.py:285-297, 328-359),
// into plane k of the device stack, with the validity byte written beside it; then the cloud mask
// the same way into that byte.
//
// The per-pixel logic is lt_sample.h, the source liblt_io.so's lt_grid_sample is compiled from. A
// thread takes groups of lt_sample::kGroup consecutive pixels (grid-stride): a group inside one
// grid row whose columns are a run of the source's moves as one sample-aligned block per plane,
// any other group pixel by pixel. Neighbouring lanes take neighbouring groups, so a wave reads and
// writes one contiguous span per plane. No LDS, no atomics: a pixel is written by one thread, and
// the mask job's read-modify-write of `valid` follows the bands job of the same raster in stream
// order. Nothing here waits for the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lt_abi.h"
#include "lt_launch.h"
#include "lt_sample.h"

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void grid_sample_kernel(const lt_sample::Args a) {
  const int64_t n_groups = lt_sample::groups(a);
  const int64_t step = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < n_groups; g += step)
    lt_sample::sample_group_of(a, g);
}

lt_sample::Args args_of(const lt_sample_job& J) {
  lt_sample::Args a;
  a.src = J.src;
  a.bps = J.bps;
  a.src_bands = J.src_bands;
  a.src_h = J.src_h;
  a.src_w = J.src_w;
  a.xoff = J.xoff;
  a.yoff = J.yoff;
  a.grid_w = J.grid_w;
  a.grid_h = J.grid_h;
  a.p0 = J.p0;
  a.n = J.n;
  a.n_sel = J.n_sel;
  for (int b = 0; b < lt_sample::kMaxSel; b++) a.sel[b] = J.sel[b];
  a.out = J.out;
  a.out_stride = J.out_stride;
  a.valid = J.valid;
  a.mode = J.mode;
  return a;
}

}  // namespace

extern "C" int lt_grid_sample_dev(lt_ctx* c, const lt_sample_job* jobs, int n_jobs, void* stream_) {
  if (!c) return LT_ERR_ARG;
  if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return lt::ctx_fail(c, LT_ERR_ARG, "null argument%s", "");
  for (int k = 0; k < n_jobs; k++) {  // every job checked before the first launch
    const char* bad = lt_sample::check(args_of(jobs[k]));
    if (bad) return lt::ctx_fail(c, LT_ERR_ARG, "sample job: %s", bad);
  }
  if (n_jobs == 0) return LT_OK;
  hipError_t e = hipSetDevice(lt::ctx_device(c));
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  hipStream_t st = (hipStream_t)stream_;
  for (int k = 0; k < n_jobs; k++) {
    const lt_sample::Args a = args_of(jobs[k]);
    const int64_t n_groups = lt_sample::groups(a);
    if (n_groups == 0) continue;
    int64_t blocks = (n_groups + kThreads - 1) / kThreads;
    if (blocks > 65536) blocks = 65536;  // the rest by the grid-stride loop
    hipLaunchKernelGGL(grid_sample_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "grid_sample_kernel: %s", hipGetErrorString(e));
  }
  return LT_OK;
}
