// lt_vertex.h — the vertex table's per-pixel code (lt_abi.h lt_vertex_table), host and device: one
// source for the kernel (lt_vertex.hip) and for its host twin (tests/native/vertex_host_check.hip).
//
// A pixel's vertices are compacted from its per-year planes the way label_pixel (lt_pixel.h) walks
// them, which restates Trendline.parse_disturbances (classes.py:156-176): the slots that hold a
// point in year order, the first of them vertex 0 whatever its flag says, every later flagged one
// the next vertex. Values travel as 64-bit words, so NaN payloads and -0.0 arrive as they were.
#pragma once
#include <stdint.h>

#include "../../include/lt_abi.h"

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace lt {

// what the kernel is launched with: the two ABI structs and the years by value
struct VertexArgs {
  lt_vertex_in in;    // (in.year is a host pointer: never read on the device)
  lt_vertex_out out;
  int32_t year[LT_MAX_YEARS];
};

// the argument checks of lt_vertex_table, shared with the host twin: LT_OK or the LT_ERR_* code and
// what to say (n_pix == 0 is LT_OK too: the caller returns before it launches anything)
inline int vertex_check(const lt_vertex_in* in, const lt_vertex_out* out, const char** why) {
  *why = "";
  if (!in || !out) return *why = "null argument", LT_ERR_ARG;
  if (in->n_pix < 0 || in->n_years < 0) return *why = "negative n_pix or n_years", LT_ERR_ARG;
  if (in->n_pix == 0) return LT_OK;
  if (in->n_years > LT_MAX_YEARS) return *why = "n_years above LT_MAX_YEARS", LT_ERR_LIMIT;
  if (in->n_pix > LT_MAX_TILE_PIX) return *why = "n_pix above LT_MAX_TILE_PIX", LT_ERR_LIMIT;
  if (in->n_years > 0 && (!in->val_fit || !in->vertex || !in->year))
    return *why = "val_fit / vertex planes and year required", LT_ERR_ARG;
  if (in->stride < in->n_pix || out->stride < in->n_pix)
    return *why = "stride or out->stride below n_pix", LT_ERR_ARG;
  if (in->present && in->winner) return *why = "at most one of present / winner", LT_ERR_ARG;
  if (out->vertex_raw && !in->val_raw) return *why = "vertex_raw needs val_raw", LT_ERR_ARG;
  if (out->max_vertices < 1 || out->max_vertices > LT_MAX_YEARS)
    return *why = "max_vertices outside [1, LT_MAX_YEARS]", LT_ERR_ARG;
  return LT_OK;
}

inline void vertex_args(const lt_vertex_in* in, const lt_vertex_out* out, VertexArgs& A) {
  A.in = *in;
  A.out = *out;
  for (int y = 0; y < LT_MAX_YEARS; y++) A.year[y] = y < in->n_years ? in->year[y] : 0;
}

// One pixel. The year loop runs Y times for every lane; the flag and presence rows are read by
// every lane (1-2 B each, a coalesced row), val_fit / val_raw only where the lane has a vertex.
// The lane's slot counter n addresses its row of the outputs; nothing is indexed at run time but
// global memory. The trailing LT_NODATA fill walks j for all lanes together, so a row's fill
// stores are neighbours.
__host__ __device__ inline void vertex_pixel(const VertexArgs& A, int64_t p) {
  const int64_t is = A.in.stride, os = A.out.stride;
  const int Y = A.in.n_years, V = A.out.max_vertices;
  const uint64_t* fit = (const uint64_t*)A.in.val_fit;
  const uint64_t* raw = (const uint64_t*)A.in.val_raw;
  uint64_t* ofit = (uint64_t*)A.out.vertex_fit;
  uint64_t* oraw = (uint64_t*)A.out.vertex_raw;
  int n = 0;
  for (int y = 0; y < Y; y++) {
    const int64_t q = (int64_t)y * is + p;
    const bool flag = A.in.vertex[q] != 0;
    const bool pres = A.in.present ? A.in.present[q] != 0
                                   : (A.in.winner ? A.in.winner[q] >= 0 : true);
    if (!(pres && (flag || n == 0))) continue;
    if (n < V) {
      const int64_t o = (int64_t)n * os + p;
      if (A.out.vertex_year) A.out.vertex_year[o] = A.year[y];
      if (ofit) ofit[o] = fit[q];
      if (oraw) oraw[o] = raw[q];
    }
    n++;
  }
  for (int j = 0; j < V; j++) {
    if (j < n) continue;
    const int64_t o = (int64_t)j * os + p;
    if (A.out.vertex_year) A.out.vertex_year[o] = LT_NODATA;
    if (A.out.vertex_fit) A.out.vertex_fit[o] = (double)LT_NODATA;
    if (A.out.vertex_raw) A.out.vertex_raw[o] = (double)LT_NODATA;
  }
  if (A.out.n_vertices) A.out.n_vertices[p] = n;
}

}  // namespace lt
