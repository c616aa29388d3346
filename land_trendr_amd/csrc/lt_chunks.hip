// lt_chunks.hip — TIFF strips and tiles, uncompressed, LZW or Deflate, decoded where the samples
// are going (lt_abi.h lt_tiff_decode_chunks_dev): lt_io.cpp's lt_tiff_decode_chunks with the
// compressed chunks and the planes in device memory. Beside lt_decode.hip, which keeps the
// strip-only LZW path as it is.
//
// One lane per chunk, as in lt_decode.hip: a lane decodes its chunk with the cores the host library
// also compiles (lt_chunk.h over lt_lzw_core.h and lt_inflate_core.h), reading back its own earlier
// output for the string and match copies: one thread's program order is all the ordering there is.
// The chunks of every image of a launch are one index space walked grid-stride by a bounded number
// of lanes. A lane's Huffman tables (350 16-bit entries) are in LDS, entry-major inside the wave
// (entry * 64 + lane): 44,800 bytes a workgroup of one wave, under the 64 KB a workgroup gets
// without attributes, three waves to a CU's 160 KB. The LZW string tables (LZW images only) are in
// global memory as in lt_decode.hip. A tile, or a chunky chunk, is decoded into the lane's chunk
// buffer and copied into the planes from there, clipped at the raster's edges.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lt_abi.h"
#include "lt_chunk.h"
#include "lt_launch.h"

namespace {

constexpr int kWave = 64;
constexpr int kTableWords = 4096;   // LZW, per lane: 16 KB
constexpr int kMaxJobs = 16;        // images per launch (the kernel's argument block)
constexpr int64_t kMaxWaves = 512;  // lanes in flight per launch: 32768
constexpr int64_t kChunkScratch = (int64_t)1 << 30;  // chunk buffers in flight, bytes

struct Batch {
  lt_chunk::Image img[kMaxJobs];
  int32_t* err[kMaxJobs];
  int64_t first[kMaxJobs + 1];  // image j's chunks are [first[j], first[j + 1]) of the index space
  int32_t n;
};

lt_chunk::Image image_of(const lt_chunks_job& J) {
  return lt_chunk::make_image(J.file, J.file_size, J.offsets, J.counts, J.compression, J.predictor,
                              J.bps, J.big_endian, J.width, J.height, J.bands, J.planar, J.chunk_w,
                              J.chunk_h, J.tiled, J.out);
}

__global__ __launch_bounds__(kWave) void decode_chunks_kernel(const Batch B, uint32_t* tables,
                                                              uint8_t* chunks,
                                                              int64_t chunk_stride) {
  __shared__ uint16_t huff[lt_inflate::kEntries * kWave];
  const int64_t lane = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int64_t lanes = (int64_t)gridDim.x * kWave;
  // (tables is null when no image of the call is LZW: never dereferenced then)
  const lt_lzw::StridedTable lzw{
      tables ? tables + (int64_t)blockIdx.x * kTableWords * kWave + threadIdx.x : nullptr, kWave};
  const lt_inflate::StridedTable inf{huff + threadIdx.x, kWave};
  uint8_t* const tmp = chunks ? chunks + lane * chunk_stride : nullptr;
  const int64_t total = B.first[B.n];
  for (int64_t s = lane; s < total; s += lanes) {
    int j = 0;
    while (j + 1 < B.n && s >= B.first[j + 1]) j++;
    const int rc = lt_chunk::decode_chunk(B.img[j], s - B.first[j], lzw, inf, tmp);
    if (rc != 0) atomicCAS(B.err[j], 0, rc);
  }
}

}  // namespace

namespace lt {

void chunks_release(ChunkScratch& s) {
  for (int k = 0; k < s.n_sets; k++) {
    if (s.set[k].d_tables) (void)hipFree(s.set[k].d_tables);
    if (s.set[k].d_chunks) (void)hipFree(s.set[k].d_chunks);
    s.set[k] = ChunkScratch::Set();
  }
  s.n_sets = 0;
}

}  // namespace lt

#define HIP_OR_FAIL(ctx, expr)                                               \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess)                                                    \
      return lt::ctx_fail(ctx, LT_ERR_HIP, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

extern "C" int lt_tiff_decode_chunks_dev(lt_ctx* c, const lt_chunks_job* jobs, int n_jobs,
                                         void* stream_) {
  if (!c) return LT_ERR_ARG;
  if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return lt::ctx_fail(c, LT_ERR_ARG, "null argument%s", "");
  int64_t max_staged = 0;
  bool any_lzw = false;
  for (int k = 0; k < n_jobs; k++) {
    const lt_chunk::Image I = image_of(jobs[k]);
    if (!jobs[k].err || lt_chunk::bad_image(I, jobs[k].n_chunks))
      return lt::ctx_fail(c, LT_ERR_ARG,
                          "bad chunks job (null pointer, size, compression 1/5/8, predictor 1/2, "
                          "planar 1/2, chunk count, or chunks of 1 MiB or more: the host path)%s", "");
    if (I.compression == 5) any_lzw = true;
    if (lt_chunk::staged(I) && lt_chunk::chunk_bytes(I) > max_staged)
      max_staged = lt_chunk::chunk_bytes(I);
  }
  if (n_jobs == 0) return LT_OK;
  int64_t max_lanes = 0;  // lanes of the widest launch (kMaxJobs images each)
  for (int k0 = 0; k0 < n_jobs; k0 += kMaxJobs) {
    int64_t total = 0;
    for (int k = k0; k < n_jobs && k < k0 + kMaxJobs; k++)
      total += lt_chunk::image_chunks(image_of(jobs[k]));
    if (total > max_lanes) max_lanes = total;
  }
  int64_t waves = (max_lanes + kWave - 1) / kWave;
  if (waves > kMaxWaves) waves = kMaxWaves;
  const int64_t chunk_stride = (max_staged + 15) / 16 * 16;
  if (chunk_stride > 0) {  // chunk buffers in flight: a bounded buffer, at least one wave
    const int64_t w = kChunkScratch / (chunk_stride * kWave);
    if (waves > w) waves = w > 1 ? w : 1;
  }
  HIP_OR_FAIL(c, hipSetDevice(lt::ctx_device(c)));
  hipStream_t st = (hipStream_t)stream_;
  lt::ChunkScratch& D = lt::ctx_chunks(c);
  int si = -1;
  for (int k = 0; k < D.n_sets; k++)
    if (D.stream[k] == st) si = k;
  if (si < 0) {
    if (D.n_sets == lt::ChunkScratch::kMaxSets) {  // more streams than sets: start over
      HIP_OR_FAIL(c, hipDeviceSynchronize());
      lt::chunks_release(D);
    }
    si = D.n_sets++;
    D.stream[si] = st;
    D.set[si] = lt::ChunkScratch::Set();
  }
  lt::ChunkScratch::Set& S = D.set[si];
  if (any_lzw && S.table_lanes < waves * kWave) {  // (hipFree waits for the launches using it)
    if (S.d_tables) HIP_OR_FAIL(c, hipFree(S.d_tables));
    S.d_tables = nullptr;
    S.table_lanes = 0;
    HIP_OR_FAIL(c, hipMalloc((void**)&S.d_tables,
                             (size_t)(waves * kWave) * kTableWords * sizeof(uint32_t)));
    S.table_lanes = waves * kWave;
  }
  if (S.chunks_bytes < waves * kWave * chunk_stride) {
    if (S.d_chunks) HIP_OR_FAIL(c, hipFree(S.d_chunks));
    S.d_chunks = nullptr;
    S.chunks_bytes = 0;
    HIP_OR_FAIL(c, hipMalloc((void**)&S.d_chunks, (size_t)(waves * kWave * chunk_stride)));
    S.chunks_bytes = waves * kWave * chunk_stride;
  }
  for (int k = 0; k < n_jobs; k++)
    HIP_OR_FAIL(c, hipMemsetAsync(jobs[k].err, 0, sizeof(int32_t), st));
  for (int k0 = 0; k0 < n_jobs; k0 += kMaxJobs) {
    Batch B;
    B.n = 0;
    B.first[0] = 0;
    for (int k = k0; k < n_jobs && k < k0 + kMaxJobs; k++) {
      B.img[B.n] = image_of(jobs[k]);
      B.err[B.n] = jobs[k].err;
      B.first[B.n + 1] = B.first[B.n] + lt_chunk::image_chunks(B.img[B.n]);
      B.n++;
    }
    for (int k = B.n; k < kMaxJobs; k++) {
      B.img[k] = lt_chunk::Image();
      B.err[k] = nullptr;
      B.first[k + 1] = B.first[B.n];
    }
    int64_t w = (B.first[B.n] + kWave - 1) / kWave;
    if (w > waves) w = waves;
    hipLaunchKernelGGL(decode_chunks_kernel, dim3((unsigned)w), dim3(kWave), 0, st, B,
                       any_lzw ? S.d_tables : nullptr, chunk_stride > 0 ? S.d_chunks : nullptr,
                       chunk_stride);
    HIP_OR_FAIL(c, hipGetLastError());
  }
  return LT_OK;
}
