// lt_ftv.hip — fit to vertex on the device (lt_abi.h lt_ftv_tile): the segments an analysis found
// on one index, fitted to a second index's values (vertices2eqns + eqns2fitted_points,
// utils.py:646-722, on given winner / spike / vertex planes).
//
// The per-pixel logic is lt_ftv.h, the source tests/native/ftv_host_check.hip compiles for the
// host. A lane is a pixel and a workgroup is one wave (as the analyze kernels): every plane access
// is row y, element p, so rows coalesce; the fitting series is in LDS as [k][lane] planes (int16
// for an int16 index raster, binary64 otherwise), sized by the year bucket of the instance (32,
// 48 or 64 year slots) so that short scenes do not pay for 64; the segment fits run in lockstep
// (lt_fast.h lsq_fit_lockstep: the x half from the context's x-set table, lsq_factor for the lanes
// that miss, the general lsq_apply only if some lane's segment has more than four points); each
// binary64 plane is written one coalesced row at a time with nontemporal stores. Nothing here
// waits for the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/lt_abi.h"
#include "lt_launch.h"
#include "lt_fast.h"
#include "lt_ftv.h"

namespace {

constexpr int kWave = 64;

// the device's Wave policy of lt::ftv_pixel
struct DevWave {
  const lt::lsq_xf* __restrict__ xtab;
  __device__ bool any(bool b) const { return __ballot(b) != 0; }
  template <class GX, class GY>
  __device__ int fit(bool act, int m, GX X, GY Y, double& slope, double& icpt) const {
    return lt::lsq_fit_lockstep(act, m, X, Y, xtab, slope, icpt);
  }
  template <class T>
  __device__ void store(T* at, T v) const { __builtin_nontemporal_store(v, at); }
};

template <int MAXY, class VT>
__global__ __launch_bounds__(kWave) void ftv_kernel(const lt::FtvArgs A,
                                                    const lt::lsq_xf* __restrict__ xtab) {
  __shared__ lt::FtvSeries<MAXY, VT, kWave> L;
  const int lane = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * kWave + lane;
  lt::ftv_pixel<MAXY, VT, kWave>(A, p, p < A.in.n_pix, lane, L, DevWave{xtab});
}

template <class VT>
void launch(int Y, unsigned blocks, hipStream_t st, const lt::FtvArgs& A, const lt::lsq_xf* xtab) {
  if (Y <= 32)
    hipLaunchKernelGGL((ftv_kernel<32, VT>), dim3(blocks), dim3(kWave), 0, st, A, xtab);
  else if (Y <= 48)
    hipLaunchKernelGGL((ftv_kernel<48, VT>), dim3(blocks), dim3(kWave), 0, st, A, xtab);
  else
    hipLaunchKernelGGL((ftv_kernel<64, VT>), dim3(blocks), dim3(kWave), 0, st, A, xtab);
}

}  // namespace

extern "C" int lt_ftv_tile(lt_ctx* c, const lt_scene* sc, const lt_ftv_in* in,
                           const lt_tile_out* out, void* stream_) {
  if (!c) return LT_ERR_ARG;
  auto fail = [&](int code, const char* msg) { return lt::ctx_fail(c, code, "lt_ftv_tile: %s", msg); };
  if (!sc || !in || !out) return fail(LT_ERR_ARG, "null argument");
  if (in->n_pix < 0) return fail(LT_ERR_ARG, "negative n_pix");
  if (in->n_pix == 0) return LT_OK;  // nothing is read or written
  if (in->stride < in->n_pix || in->obs_stride < in->n_pix || out->stride < in->n_pix)
    return fail(LT_ERR_ARG, "stride, obs_stride or out->stride below n_pix");
  if ((in->obs_val != nullptr) == (in->obs_index != nullptr))
    return fail(LT_ERR_ARG, "exactly one of obs_val / obs_index required");
  if (in->obs_index && (in->index_type < LT_T_F64 || in->index_type > LT_T_I64))
    return fail(LT_ERR_ARG, "bad index_type");
  // the scene, as lt_analyze_tile admits it (of its arrays only the years are read here)
  const int K = sc->n_obs, Y = sc->n_years;
  if (K < 0 || K > LT_MAX_OBS || Y < 0 || Y > LT_MAX_YEARS)
    return fail(LT_ERR_LIMIT, "scene exceeds LT_MAX_OBS/LT_MAX_YEARS");
  if (Y > 0 && !sc->year) return fail(LT_ERR_ARG, "scene years missing");
  for (int y = 1; y < Y; y++)
    if (sc->year[y] <= sc->year[y - 1]) return fail(LT_ERR_ARG, "years must be strictly ascending");
  if (Y > 0 && sc->year[Y - 1] - sc->year[0] > 255) return fail(LT_ERR_LIMIT, "year span above 255");
  if (in->n_pix > LT_MAX_TILE_PIX) return fail(LT_ERR_LIMIT, "tile above LT_MAX_TILE_PIX");
  if (Y > 0 && (!in->winner || !in->spike || !in->vertex))
    return fail(LT_ERR_ARG, "winner / spike / vertex planes required");

  lt::FtvArgs A;
  memset(&A, 0, sizeof A);
  A.in = *in;
  A.os = out->stride;
  A.val_raw = out->val_raw;
  A.val_fit = out->val_fit;
  A.fit_m = out->fit_m;
  A.fit_b = out->fit_b;
  A.right_m = out->right_m;
  A.right_b = out->right_b;
  A.status = out->status;
  A.n_obs = K;
  A.n_years = Y;
  for (int y = 0; y < Y; y++) A.year[y] = sc->year[y];

  hipError_t e = hipSetDevice(lt::ctx_device(c));
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  const unsigned blocks = (unsigned)((in->n_pix + kWave - 1) / kWave);  // <= 2^22
  hipStream_t st = (hipStream_t)stream_;
  // the series' storage: int16 for an int16 index raster (exact), binary64 for everything else
  if (in->obs_index && in->index_type == LT_T_I16)
    launch<int16_t>(Y, blocks, st, A, lt::ctx_xtab(c));
  else
    launch<double>(Y, blocks, st, A, lt::ctx_xtab(c));
  e = hipGetLastError();
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "ftv_kernel: %s", hipGetErrorString(e));
  return LT_OK;
}
