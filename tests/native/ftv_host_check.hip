// Host twin of the fit-to-vertex kernel (land_trendr_amd/csrc/lt_ftv.h, lt_ftv.hip).
// TEST INFRASTRUCTURE: compiles the exact __host__ __device__ per-pixel code the kernel runs, for
// the CPU, with a "wave" of one lane, so tests/test_ftv_host.py can check every semantic case of
// lt_ftv_tile against the goldens, the reference fixture and a numpy restatement without a GPU.
// Built by __graft_entry__.build() into tests/native/build/liblt_ftvcheck.so. Not part of the
// product (which has no CPU path).
#include <string.h>

#include "../../land_trendr_amd/csrc/lt_ftv.h"

// lt_ftv_tile over a host tile: the same structs, every pointer a HOST pointer. Returns LT_OK, or
// the LT_ERR_* lt_ftv_tile gives for these arguments.
extern "C" int ltx_ftv_tile(const lt_scene* sc, const lt_ftv_in* in, const lt_tile_out* out) {
  if (!sc || !in || !out || in->n_pix < 0) return LT_ERR_ARG;
  if (in->n_pix == 0) return LT_OK;
  if (in->stride < in->n_pix || in->obs_stride < in->n_pix || out->stride < in->n_pix)
    return LT_ERR_ARG;
  if ((in->obs_val != nullptr) == (in->obs_index != nullptr)) return LT_ERR_ARG;
  if (in->obs_index && (in->index_type < LT_T_F64 || in->index_type > LT_T_I64)) return LT_ERR_ARG;
  const int K = sc->n_obs, Y = sc->n_years;
  if (K < 0 || K > LT_MAX_OBS || Y < 0 || Y > LT_MAX_YEARS) return LT_ERR_LIMIT;
  if (Y > 0 && !sc->year) return LT_ERR_ARG;
  for (int y = 1; y < Y; y++)
    if (sc->year[y] <= sc->year[y - 1]) return LT_ERR_ARG;
  if (Y > 0 && sc->year[Y - 1] - sc->year[0] > 255) return LT_ERR_LIMIT;
  if (Y > 0 && (!in->winner || !in->spike || !in->vertex)) return LT_ERR_ARG;
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
  const lt::FtvHostWave W;
  // the kernel's series types: int16 for an int16 index raster, binary64 otherwise
  if (in->obs_index && in->index_type == LT_T_I16) {
    static lt::FtvSeries<LT_MAX_YEARS, int16_t, 1> L;
    for (int64_t p = 0; p < in->n_pix; p++)
      lt::ftv_pixel<LT_MAX_YEARS, int16_t, 1>(A, p, true, 0, L, W);
  } else {
    static lt::FtvSeries<LT_MAX_YEARS, double, 1> L;
    for (int64_t p = 0; p < in->n_pix; p++)
      lt::ftv_pixel<LT_MAX_YEARS, double, 1>(A, p, true, 0, L, W);
  }
  return LT_OK;
}
