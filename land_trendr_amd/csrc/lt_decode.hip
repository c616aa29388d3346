// lt_decode.hip — TIFF strips decoded where the samples are going (lt_abi.h
// lt_tiff_decode_strips_dev): lt_io.cpp's lt_tiff_decode_strips with the compressed strips and the
// planes in device memory.
//
// One lane per strip. A lane decodes its strip with the LZW core the host library also compiles
// (lt_lzw_core.h; liblt_io.so lt_lzw_decode_core), reading back its own earlier output for the
// string copies: one thread's program order is all the ordering there is, no fences, no hand-off
// between lanes. The strips of every image of a call are one index space walked grid-stride by a
// bounded number of lanes. A lane's string table (4096 words) is entry-major inside its wave
// (wave base + entry * 64 + lane): every lane adds entry free_ent in the same turn of the code loop,
// so the table writes of a wave coalesce and only the lookups scatter. Byte swap, predictor 2 and
// the chunky de-interleave follow in the same lane, in lt_tiff_decode_strips's order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lt_abi.h"
#include "lt_launch.h"
#include "lt_lzw_core.h"

namespace {

constexpr int kWave = 64;
constexpr int kTableWords = 4096;        // per lane: 16 KB
constexpr int kMaxJobs = 16;             // images per launch (the kernel's argument block)
constexpr int64_t kMaxWaves = 512;       // lanes in flight per launch: 32768 (512 MB of tables)
constexpr int64_t kStripScratch = (int64_t)256 << 20;  // chunky strips in flight, bytes

struct Batch {
  lt_strips_job job[kMaxJobs];
  int64_t first[kMaxJobs + 1];  // job j's strips are [first[j], first[j + 1]) of the index space
  int32_t n;
};

__device__ inline void strip_error(int32_t* err, int32_t code) { atomicCAS(err, 0, code); }

template <class T>
__device__ inline void undo_pred2(uint8_t* buf, int64_t rows, int64_t width, int spp) {
  T* a = (T*)buf;
  for (int64_t y = 0; y < rows; y++) {
    T* r = a + y * width * spp;
    for (int64_t x = spp; x < width * spp; x++) r[x] = (T)(r[x] + r[x - spp]);
  }
}

// Strip k of image J, as lt_tiff_decode_strips's worker does it. `tmp`: this lane's strip buffer
// (chunky images only).
__device__ void decode_strip(const lt_strips_job& J, int64_t k, const lt_lzw::StridedTable tab,
                             uint8_t* tmp) {
  const int bps = J.bps;
  const int spp = J.planar == 1 ? J.bands : 1;
  const int64_t per_band = (J.height + J.rows_per_strip - 1) / J.rows_per_strip;
  const int64_t b = J.planar == 1 ? 0 : k / per_band, r = J.planar == 1 ? k : k % per_band;
  if (b >= J.bands || r >= per_band) return;  // (the host counts only the image's strips)
  const int64_t y0 = r * J.rows_per_strip;
  const int64_t rows = J.rows_per_strip < J.height - y0 ? J.rows_per_strip : J.height - y0;
  const int64_t size = rows * J.width * spp * bps;
  const int64_t plane = J.width * J.height * bps;
  const uint64_t off = J.offsets[k], cnt = J.counts[k];
  if (off > (uint64_t)J.file_size || cnt > (uint64_t)J.file_size - off) {
    strip_error(J.err, lt_lzw::kErrData);
    return;
  }
  const uint8_t* src = J.file + off;
  uint8_t* const out = (uint8_t*)J.out;
  const bool direct = spp == 1;  // planar 2: straight into the band's rows
  uint8_t* dst = direct ? out + b * plane + y0 * J.width * bps : tmp;
  int64_t n;
  if (J.compression == 5) {
    n = lt_lzw::decode(src, (int64_t)cnt, dst, size, tab);
    if (n < 0) {
      strip_error(J.err, (int32_t)n);
      return;
    }
  } else {
    n = size < (int64_t)cnt ? size : (int64_t)cnt;
    for (int64_t i = 0; i < n; i++) dst[i] = src[i];
  }
  for (int64_t i = n; i < size; i++) dst[i] = 0;  // a short strip: zero-padded (libtiff)
  const int64_t samples = rows * J.width * spp;
  if (J.big_endian && bps > 1) {
    for (int64_t i = 0; i < samples; i++) {
      uint8_t* p = dst + i * bps;
      for (int a = 0; a < bps / 2; a++) {
        const uint8_t t = p[a];
        p[a] = p[bps - 1 - a];
        p[bps - 1 - a] = t;
      }
    }
  }
  if (J.predictor == 2) {
    switch (bps) {
      case 1: undo_pred2<uint8_t>(dst, rows, J.width, spp); break;
      case 2: undo_pred2<uint16_t>(dst, rows, J.width, spp); break;
      case 4: undo_pred2<uint32_t>(dst, rows, J.width, spp); break;
      default: undo_pred2<uint64_t>(dst, rows, J.width, spp); break;
    }
  }
  if (!direct) {  // chunky: de-interleave the samples into the band planes
    for (int bb = 0; bb < J.bands; bb++) {
      uint8_t* o = out + bb * plane + y0 * J.width * bps;
      const uint8_t* i = dst + bb * bps;
      for (int64_t px = 0; px < rows * J.width; px++)
        for (int a = 0; a < bps; a++) o[px * bps + a] = i[px * spp * bps + a];
    }
  }
}

__global__ __launch_bounds__(kWave) void decode_strips_kernel(const Batch B, uint32_t* tables,
                                                              uint8_t* strips,
                                                              int64_t strip_stride) {
  const int64_t lane = (int64_t)blockIdx.x * kWave + threadIdx.x;
  const int64_t lanes = (int64_t)gridDim.x * kWave;
  const lt_lzw::StridedTable tab{tables + (int64_t)blockIdx.x * kTableWords * kWave + threadIdx.x,
                                 kWave};
  uint8_t* const tmp = strips ? strips + lane * strip_stride : nullptr;
  const int64_t total = B.first[B.n];
  for (int64_t s = lane; s < total; s += lanes) {
    int j = 0;
    while (j + 1 < B.n && s >= B.first[j + 1]) j++;
    decode_strip(B.job[j], s - B.first[j], tab, tmp);
  }
}

// the strips of the image itself (what the host function requires of n_strips)
int64_t image_strips(const lt_strips_job& J) {
  const int64_t per_band = (J.height + J.rows_per_strip - 1) / J.rows_per_strip;
  return J.planar == 1 ? per_band : per_band * J.bands;
}

// decoded bytes of a full strip, or -1 when it is not below 1 MiB
int64_t strip_bytes(const lt_strips_job& J) {
  const int64_t rows = J.rows_per_strip < J.height ? J.rows_per_strip : J.height;
  const int spp = J.planar == 1 ? J.bands : 1;
  const double sz = (double)rows * (double)J.width * (double)spp * (double)J.bps;
  if (sz >= (double)lt_lzw::kCoreMaxOut) return -1;
  return rows * J.width * spp * J.bps;
}

}  // namespace

namespace lt {

void decode_release(DecodeScratch& s) {
  for (int k = 0; k < s.n_sets; k++) {
    if (s.set[k].d_tables) (void)hipFree(s.set[k].d_tables);
    if (s.set[k].d_strips) (void)hipFree(s.set[k].d_strips);
    s.set[k] = DecodeScratch::Set();
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

extern "C" int lt_tiff_decode_strips_dev(lt_ctx* c, const lt_strips_job* jobs, int n_jobs,
                                         void* stream_) {
  if (!c) return LT_ERR_ARG;
  if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return lt::ctx_fail(c, LT_ERR_ARG, "null argument%s", "");
  int64_t max_lanes = 0, max_chunky = 0;
  for (int k = 0; k < n_jobs; k++) {
    const lt_strips_job& J = jobs[k];
    if (!J.file || !J.offsets || !J.counts || !J.out || !J.err || J.file_size < 0 ||
        J.width <= 0 || J.height <= 0 || J.bands <= 0 || J.rows_per_strip <= 0 ||
        !(J.bps == 1 || J.bps == 2 || J.bps == 4 || J.bps == 8))
      return lt::ctx_fail(c, LT_ERR_ARG, "bad strips job%s", "");
    if ((J.compression != 1 && J.compression != 5) || (J.predictor != 1 && J.predictor != 2))
      return lt::ctx_fail(c, LT_ERR_ARG, "strips job: compression 1 or 5, predictor 1 or 2%s", "");
    if (J.planar != 1 && J.planar != 2)
      return lt::ctx_fail(c, LT_ERR_ARG, "strips job: planar 1 or 2%s", "");
    if (J.n_strips < image_strips(J))
      return lt::ctx_fail(c, LT_ERR_ARG, "strips job: fewer strips than the image has%s", "");
    const int64_t sz = strip_bytes(J);
    if (sz < 0)
      return lt::ctx_fail(c, LT_ERR_ARG, "strips of 1 MiB or more decoded: the host path%s", "");
    if (J.planar == 1 && J.bands > 1 && sz > max_chunky) max_chunky = sz;
  }
  if (n_jobs == 0) return LT_OK;
  // lanes of the widest launch (kMaxJobs images each)
  for (int k0 = 0; k0 < n_jobs; k0 += kMaxJobs) {
    int64_t total = 0;
    for (int k = k0; k < n_jobs && k < k0 + kMaxJobs; k++) total += image_strips(jobs[k]);
    if (total > max_lanes) max_lanes = total;
  }
  int64_t waves = (max_lanes + kWave - 1) / kWave;
  if (waves > kMaxWaves) waves = kMaxWaves;
  const int64_t strip_stride = (max_chunky + 15) / 16 * 16;
  if (strip_stride > 0) {  // chunky strips in flight: a bounded buffer, at least one wave
    const int64_t w = kStripScratch / (strip_stride * kWave);
    if (waves > w) waves = w > 1 ? w : 1;
  }
  HIP_OR_FAIL(c, hipSetDevice(lt::ctx_device(c)));
  hipStream_t st = (hipStream_t)stream_;
  lt::DecodeScratch& D = lt::ctx_decode(c);
  int si = -1;
  for (int k = 0; k < D.n_sets; k++)
    if (D.stream[k] == st) si = k;
  if (si < 0) {
    if (D.n_sets == lt::DecodeScratch::kMaxSets) {  // more streams than sets: start over
      HIP_OR_FAIL(c, hipDeviceSynchronize());
      lt::decode_release(D);
    }
    si = D.n_sets++;
    D.stream[si] = st;
    D.set[si] = lt::DecodeScratch::Set();
  }
  lt::DecodeScratch::Set& S = D.set[si];
  if (S.table_lanes < waves * kWave) {  // (hipFree waits for the launches still using it)
    if (S.d_tables) HIP_OR_FAIL(c, hipFree(S.d_tables));
    S.d_tables = nullptr;
    S.table_lanes = 0;
    HIP_OR_FAIL(c, hipMalloc((void**)&S.d_tables,
                             (size_t)(waves * kWave) * kTableWords * sizeof(uint32_t)));
    S.table_lanes = waves * kWave;
  }
  if (S.strips_bytes < waves * kWave * strip_stride) {
    if (S.d_strips) HIP_OR_FAIL(c, hipFree(S.d_strips));
    S.d_strips = nullptr;
    S.strips_bytes = 0;
    HIP_OR_FAIL(c, hipMalloc((void**)&S.d_strips, (size_t)(waves * kWave * strip_stride)));
    S.strips_bytes = waves * kWave * strip_stride;
  }
  for (int k = 0; k < n_jobs; k++)
    HIP_OR_FAIL(c, hipMemsetAsync(jobs[k].err, 0, sizeof(int32_t), st));
  for (int k0 = 0; k0 < n_jobs; k0 += kMaxJobs) {
    Batch B;
    B.n = 0;
    B.first[0] = 0;
    for (int k = k0; k < n_jobs && k < k0 + kMaxJobs; k++) {
      B.job[B.n] = jobs[k];
      B.first[B.n + 1] = B.first[B.n] + image_strips(jobs[k]);
      B.n++;
    }
    for (int k = B.n; k < kMaxJobs; k++) {
      B.job[k] = lt_strips_job();
      B.first[k + 1] = B.first[B.n];
    }
    int64_t w = (B.first[B.n] + kWave - 1) / kWave;
    if (w > waves) w = waves;
    hipLaunchKernelGGL(decode_strips_kernel, dim3((unsigned)w), dim3(kWave), 0, st, B, S.d_tables,
                       strip_stride > 0 ? S.d_strips : nullptr, strip_stride);
    HIP_OR_FAIL(c, hipGetLastError());
  }
  return LT_OK;
}
