// Host twin of the vertex-table kernel (land_trendr_amd/csrc/lt_vertex.h, lt_vertex.hip).
// TEST INFRASTRUCTURE: compiles the exact __host__ __device__ per-pixel code the kernel runs, and
// the entry point's argument checks, for the CPU, so tests/test_vertex_host.py can check every
// semantic case of lt_vertex_table against the goldens, the reference fixture and a numpy
// restatement without a GPU, and the job's CPU tests have a vertex_table to call. Built by
// __graft_entry__.build() into tests/native/build/liblt_vertexcheck.so. Not part of the product
// (which has no CPU path).
#include "../../land_trendr_amd/csrc/lt_vertex.h"

// lt_vertex_table over host planes: the same structs, every pointer a HOST pointer. Returns LT_OK,
// or the LT_ERR_* lt_vertex_table gives for these arguments.
extern "C" int ltx_vertex_table(const lt_vertex_in* in, const lt_vertex_out* out) {
  const char* why;
  const int rc = lt::vertex_check(in, out, &why);
  if (rc != LT_OK || in->n_pix == 0) return rc;
  lt::VertexArgs A;
  lt::vertex_args(in, out, A);
  for (int64_t p = 0; p < in->n_pix; p++) lt::vertex_pixel(A, p);
  return LT_OK;
}
