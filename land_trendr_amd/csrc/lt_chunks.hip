// lt_chunks.hip — TIFF strips and tiles, uncompressed, LZW or Deflate, decoded where the samples
// are going: lt_io.cpp's lt_tiff_decode_chunks with the compressed chunks and the planes in device
// memory. The one device decoder, behind both entries of lt_abi.h: lt_tiff_decode_chunks_dev, and
// lt_tiff_decode_strips_dev, which spells its strip images out as chunk jobs.
//
// One lane per chunk: a lane decodes its chunk with the cores the host library also compiles
// (lt_chunk.h over lt_lzw_core.h and lt_inflate_core.h), reading back its own earlier output for
// the string and match copies: one thread's program order is all the ordering there is, no fences,
// no hand-off between lanes. The chunks of every image of a launch are one index space walked
// grid-stride by a bounded number of lanes. A lane's LZW string table (4096 words, LZW images only)
// is in global memory, entry-major inside its wave (wave base + entry * 64 + lane): every lane adds
// entry free_ent in the same turn of the code loop, so the table writes of a wave coalesce and only
// the lookups scatter. A tile, or a chunky chunk, is decoded into the lane's chunk buffer and
// copied into the planes from there, clipped at the raster's edges.
// The kernel has two instances, chosen per launch. With Deflate: a lane's Huffman tables (350
// 16-bit entries) are in LDS, entry-major inside the wave (entry * 64 + lane): 44,800 bytes a
// workgroup of one wave, under the 64 KB a workgroup gets without attributes, three waves to a
// CU's 160 KB. Without (no image of the launch has compression 8): no LDS, no private scratch and
// less than half the registers, so uncompressed and LZW images do not pay for the Deflate core.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/lt_abi.h"
#include "lt_chunk.h"
#include "lt_launch.h"

namespace {

constexpr int kWave = 64;
constexpr int kTableWords = 4096;   // LZW, per lane: 16 KB
constexpr int kMaxJobs = 16;        // images per launch (the kernel's argument block)
constexpr int64_t kMaxWaves = 512;  // lanes in flight per launch: 32768 (512 MB of tables)
// chunk buffers in flight, bytes, by entry
constexpr int64_t kStripStaging = (int64_t)256 << 20, kChunkStaging = (int64_t)1 << 30;

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

template <bool kInflate>
__global__ __launch_bounds__(kWave) void decode_chunks_kernel(const Batch B, uint32_t* tables,
                                                              uint8_t* chunks,
                                                              int64_t chunk_stride) {
  __shared__ uint16_t huff[kInflate ? lt_inflate::kEntries * kWave : 1];
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
    const int rc = lt_chunk::decode_chunk<kInflate>(B.img[j], s - B.first[j], lzw, inf, tmp);
    if (rc != 0) atomicCAS(B.err[j], 0, rc);
  }
}

// Both entries: the checks, the caps, the stream's scratch, then a launch per kMaxJobs images.
// staging_cap: the bytes of chunk buffers in flight the entry allows itself.
int decode_jobs(lt_ctx* c, const lt_chunks_job* jobs, int n_jobs, hipStream_t st,
                int64_t staging_cap) {
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
  int64_t max_lanes = 0;  // lanes of the widest launch
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
    const int64_t w = staging_cap / (chunk_stride * kWave);
    if (waves > w) waves = w > 1 ? w : 1;
  }
  HIP_OR_FAIL(c, hipSetDevice(lt::ctx_device(c)));
  lt::DecodeSet* S;
  HIP_OR_FAIL(c, lt::ctx_decode(c).find(st, &S));
  if (any_lzw)
    HIP_OR_FAIL(c, lt::grow(S->d_tables, S->tables_bytes,
                            waves * kWave * kTableWords * (int64_t)sizeof(uint32_t)));
  HIP_OR_FAIL(c, lt::grow(S->d_chunks, S->chunks_bytes, waves * kWave * chunk_stride));
  for (int k = 0; k < n_jobs; k++)
    HIP_OR_FAIL(c, hipMemsetAsync(jobs[k].err, 0, sizeof(int32_t), st));
  for (int k0 = 0; k0 < n_jobs; k0 += kMaxJobs) {
    Batch B;
    B.n = 0;
    B.first[0] = 0;
    bool inflate = false;  // the launch's kernel instance: with Deflate only when an image needs it
    for (int k = k0; k < n_jobs && k < k0 + kMaxJobs; k++) {
      B.img[B.n] = image_of(jobs[k]);
      B.err[B.n] = jobs[k].err;
      B.first[B.n + 1] = B.first[B.n] + lt_chunk::image_chunks(B.img[B.n]);
      if (B.img[B.n].compression == 8) inflate = true;
      B.n++;
    }
    for (int k = B.n; k < kMaxJobs; k++) {
      B.img[k] = lt_chunk::Image();
      B.err[k] = nullptr;
      B.first[k + 1] = B.first[B.n];
    }
    int64_t w = (B.first[B.n] + kWave - 1) / kWave;
    if (w > waves) w = waves;
    hipLaunchKernelGGL(inflate ? decode_chunks_kernel<true> : decode_chunks_kernel<false>,
                       dim3((unsigned)w), dim3(kWave), 0, st, B, any_lzw ? S->d_tables : nullptr,
                       chunk_stride > 0 ? S->d_chunks : nullptr, chunk_stride);
    HIP_OR_FAIL(c, hipGetLastError());
  }
  return LT_OK;
}

}  // namespace

extern "C" int lt_tiff_decode_chunks_dev(lt_ctx* c, const lt_chunks_job* jobs, int n_jobs,
                                         void* stream) {
  if (!c) return LT_ERR_ARG;
  if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return lt::ctx_fail(c, LT_ERR_ARG, "null argument%s", "");
  return decode_jobs(c, jobs, n_jobs, (hipStream_t)stream, kChunkStaging);
}

// The strip images as chunk jobs: strips as wide as the image, rows_per_strip rows each. What a
// strips job may not hold and a chunks job may (Deflate, no rows) is refused here.
extern "C" int lt_tiff_decode_strips_dev(lt_ctx* c, const lt_strips_job* jobs, int n_jobs,
                                         void* stream) {
  if (!c) return LT_ERR_ARG;
  if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return lt::ctx_fail(c, LT_ERR_ARG, "null argument%s", "");
  std::vector<lt_chunks_job> chunks((size_t)n_jobs);
  for (int k = 0; k < n_jobs; k++) {
    const lt_strips_job& J = jobs[k];
    if (J.rows_per_strip <= 0) return lt::ctx_fail(c, LT_ERR_ARG, "bad strips job%s", "");
    if (J.compression != 1 && J.compression != 5)
      return lt::ctx_fail(c, LT_ERR_ARG, "strips job: compression 1 or 5, predictor 1 or 2%s", "");
    // (lt_chunks_job's fields in order: chunk_w = width, chunk_h = rows_per_strip, tiled = 0)
    chunks[k] = lt_chunks_job{J.file, J.file_size, J.offsets, J.counts, J.n_strips,
                              J.compression, J.predictor, J.bps, J.big_endian,
                              J.width, J.height, J.bands, J.planar,
                              J.width, J.rows_per_strip, 0, J.out, J.err};
  }
  return decode_jobs(c, chunks.data(), n_jobs, (hipStream_t)stream, kStripStaging);
}
