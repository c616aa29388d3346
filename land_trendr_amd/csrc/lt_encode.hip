// lt_encode.hip — output rasters' TIFF strips encoded where the rasters are assembled (lt_abi.h
// lt_tiff_encode_strips_dev): lt_io.cpp's lt_tiff_encode_strips with the raster, the strips and
// their sizes in device memory.
//
// One lane per strip. A lane encodes its strip with the LZW core the host library also compiles
// (lt_lzw_core.h; liblt_io.so lt_lzw_encode_core) into a slot of its own in context-owned scratch
// (the worst case, raw * 3 / 2 + 16 bytes); predictor 2 is applied on the fly by the lane's byte
// source, never to the raster. A lane's dictionary (8192 words, open addressing) is entry-major
// inside its wave (wave base + slot * 64 + lane): the zeroing at a strip's start and at each Clear
// coalesces, the probes scatter. The strips of every job of a call are one index space, walked in
// rounds of a bounded number of lanes; per round three launches on the caller's stream: encode,
// an exclusive scan of the round's sizes (one block; a running total per job carries over to the
// next round), and a packing kernel (one block per strip, coalesced) that moves the slots to their
// final offsets in each job's `out`. Uncompressed rasters (compression 1) need none of this: one
// coalesced kernel writes their bytes straight to `out`. Nothing here waits for the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/lt_abi.h"
#include "lt_launch.h"
#include "lt_lzw_core.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxJobs = 16;                         // rasters per launch (the argument block)
constexpr int64_t kMaxLanes = lt::EncodeSet::kMaxLanes;  // in flight: 1 GiB of dictionaries
constexpr int64_t kSlotScratch = (int64_t)1 << 30;   // encoded strips in flight, bytes
constexpr int kScanThreads = 1024;
constexpr int kPackThreads = 256;

struct Batch {
  lt_encode_job job[kMaxJobs];
  int64_t first[kMaxJobs + 1];  // job j's strips are [first[j], first[j + 1]) of the index space
  int32_t n;
};

__device__ inline int job_of(const Batch& B, int64_t s) {
  int j = 0;
  while (j + 1 < B.n && s >= B.first[j + 1]) j++;
  return j;
}

// byte k of a strip whose rows are horizontally differenced (predictor 2, integer wrap, little
// endian): p is the strip's first sample, `cols` samples a row
template <class T>
struct Pred2Bytes {
  const T* p;
  int64_t cols;
  __device__ uint8_t byte(int64_t k) const {
    const int64_t s = k / (int64_t)sizeof(T);
    T v = p[s];
    if (s % cols != 0) v = (T)(v - p[s - 1]);
    return (uint8_t)(v >> (8 * (int)(k % (int64_t)sizeof(T))));
  }
};

// Compression 1: the strips back to back are the raster's own bytes (differenced for predictor 2)
// and every size is known, so no lane, slot or scan: thread per byte, coalesced, straight into
// `out`; a byte is written when its whole strip ends at or below cap (lt_tiff_encode_strips stops
// at the first strip that does not fit). Then the sizes and the total.
template <class Src>
__device__ inline void raw_strips(const lt_encode_job& J, const Src src) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t row_bytes = J.cols * J.bps, plane = J.rows * row_bytes, total = plane * J.bands;
  const int64_t per_band = (J.rows + J.rows_per_strip - 1) / J.rows_per_strip;
  for (int64_t i = tid; i < total; i += nthr) {
    const int64_t b = i / plane, r = (i - b * plane) / row_bytes / J.rows_per_strip;
    const int64_t y1 = (r + 1) * J.rows_per_strip < J.rows ? (r + 1) * J.rows_per_strip : J.rows;
    if (b * plane + y1 * row_bytes <= J.cap) J.out[i] = src.byte(i);
  }
  for (int64_t k = tid; k < per_band * J.bands; k += nthr) {
    const int64_t y0 = (k % per_band) * J.rows_per_strip;
    J.strip_sizes[k] =
        (J.rows_per_strip < J.rows - y0 ? J.rows_per_strip : J.rows - y0) * row_bytes;
  }
  if (tid == 0) *J.total = total > J.cap ? (int64_t)lt_lzw::kErrSpace : total;
}

__global__ __launch_bounds__(256) void raw_strips_kernel(const lt_encode_job J) {
  const uint8_t* in = (const uint8_t*)J.in;
  if (J.predictor == 2 && J.bps == 1) raw_strips(J, Pred2Bytes<uint8_t>{in, J.cols});
  else if (J.predictor == 2 && J.bps == 2)
    raw_strips(J, Pred2Bytes<uint16_t>{(const uint16_t*)in, J.cols});
  else if (J.predictor == 2 && J.bps == 4)
    raw_strips(J, Pred2Bytes<uint32_t>{(const uint32_t*)in, J.cols});
  else if (J.predictor == 2) raw_strips(J, Pred2Bytes<uint64_t>{(const uint64_t*)in, J.cols});
  else raw_strips(J, lt_lzw::PlainBytes{in});
}

// Compression 5: lane i of a round encodes strip s0 + i into slot i; slot_size[i]: its bytes, or
// LT_IO_ERR_*
__global__ __launch_bounds__(kWave) void encode_strips_kernel(const Batch B, int64_t s0, int64_t n,
                                                              uint32_t* tables, uint8_t* slots,
                                                              int64_t slot_stride,
                                                              int32_t* slot_size) {
  const int64_t lane = (int64_t)blockIdx.x * kWave + threadIdx.x;
  if (lane >= n) return;
  const lt_lzw::StridedTable tab{
      tables + (int64_t)blockIdx.x * lt_lzw::kEncSlots * kWave + threadIdx.x, kWave};
  const int64_t s = s0 + lane;
  const lt_encode_job& J = B.job[job_of(B, s)];
  const int64_t k = s - B.first[job_of(B, s)];
  const int64_t per_band = (J.rows + J.rows_per_strip - 1) / J.rows_per_strip;
  const int64_t b = k / per_band, y0 = (k % per_band) * J.rows_per_strip;
  const int64_t nr = J.rows_per_strip < J.rows - y0 ? J.rows_per_strip : J.rows - y0;
  const int64_t size = nr * J.cols * J.bps;
  const uint8_t* src = (const uint8_t*)J.in + (b * J.rows + y0) * J.cols * J.bps;
  uint8_t* dst = slots + lane * slot_stride;
  int64_t m;
  if (J.predictor == 2 && J.bps == 1)
    m = lt_lzw::encode_from(Pred2Bytes<uint8_t>{src, J.cols}, size, dst, slot_stride, tab);
  else if (J.predictor == 2 && J.bps == 2)
    m = lt_lzw::encode_from(Pred2Bytes<uint16_t>{(const uint16_t*)src, J.cols}, size, dst, slot_stride,
                   tab);
  else if (J.predictor == 2 && J.bps == 4)
    m = lt_lzw::encode_from(Pred2Bytes<uint32_t>{(const uint32_t*)src, J.cols}, size, dst, slot_stride,
                   tab);
  else if (J.predictor == 2)
    m = lt_lzw::encode_from(Pred2Bytes<uint64_t>{(const uint64_t*)src, J.cols}, size, dst, slot_stride,
                   tab);
  else
    m = lt_lzw::encode_from(lt_lzw::PlainBytes{src}, size, dst, slot_stride, tab);
  slot_size[lane] = (int32_t)m;
}

// One block. slot_off[i]: where strip s0 + i starts in its job's `out` (the job's running total of
// the earlier rounds + the sizes of the job's earlier strips of this round); the job's
// strip_sizes; carry[j] += the round's bytes of job j; in the last round `total`.
__global__ __launch_bounds__(kScanThreads) void scan_sizes_kernel(const Batch B, int64_t s0,
                                                                  int64_t n,
                                                                  const int32_t* slot_size,
                                                                  int64_t* slot_off, int64_t* carry,
                                                                  int32_t* err, int last) {
  __shared__ int64_t part[kScanThreads];
  __shared__ int64_t pbase[kMaxJobs], psum[kMaxJobs];
  const int t = threadIdx.x;
  const int64_t per = (n + kScanThreads - 1) / kScanThreads;
  const int64_t lo = (int64_t)t * per < n ? (int64_t)t * per : n;
  const int64_t hi = lo + per < n ? lo + per : n;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; i++) {
    const int32_t m = slot_size[i];
    sum += m > 0 ? m : 0;
  }
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {  // inclusive scan of the threads' sums
    const int64_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = part[t] - sum;
  for (int64_t i = lo; i < hi; i++) {  // the round's exclusive prefix
    const int32_t m = slot_size[i];
    slot_off[i] = run;
    run += m > 0 ? m : 0;
  }
  __syncthreads();
  if (t < kMaxJobs) {
    pbase[t] = 0;
    psum[t] = 0;
    if (t < B.n) {
      const int64_t a = (B.first[t] > s0 ? B.first[t] : s0) - s0;
      const int64_t e = (B.first[t + 1] < s0 + n ? B.first[t + 1] : s0 + n) - s0;
      if (e > a) {
        const int32_t m = slot_size[e - 1];
        pbase[t] = slot_off[a];
        psum[t] = slot_off[e - 1] + (m > 0 ? m : 0) - slot_off[a];
      }
    }
  }
  __syncthreads();
  for (int64_t i = lo; i < hi; i++) {
    const int j = job_of(B, s0 + i);
    const int32_t m = slot_size[i];
    slot_off[i] = carry[j] + slot_off[i] - pbase[j];
    B.job[j].strip_sizes[s0 + i - B.first[j]] = m > 0 ? m : 0;
    if (m < 0) atomicCAS(err + j, 0, m);
  }
  __syncthreads();
  if (t < B.n) {
    const int64_t c = carry[t] + psum[t];
    carry[t] = c;
    if (last) {
      const int32_t e = err[t];
      *B.job[t].total = e < 0 ? (int64_t)e : (c > B.job[t].cap ? (int64_t)lt_lzw::kErrSpace : c);
    }
  }
}

// block i moves slot i to its place; a strip that does not fit below `cap` whole is left out
__global__ __launch_bounds__(kPackThreads) void pack_strips_kernel(const Batch B, int64_t s0,
                                                                   int64_t n, const uint8_t* slots,
                                                                   int64_t slot_stride,
                                                                   const int32_t* slot_size,
                                                                   const int64_t* slot_off) {
  const int64_t i = blockIdx.x;
  if (i >= n) return;
  const int64_t m = slot_size[i];
  if (m <= 0) return;
  const lt_encode_job& J = B.job[job_of(B, s0 + i)];
  const int64_t off = slot_off[i];
  if (off < 0 || off > J.cap || m > J.cap - off) return;
  const uint8_t* src = slots + i * slot_stride;
  uint8_t* dst = J.out + off;
  for (int64_t x = threadIdx.x; x < m; x += kPackThreads) dst[x] = src[x];
}

int64_t job_strips(const lt_encode_job& J) {
  return (J.rows + J.rows_per_strip - 1) / J.rows_per_strip * J.bands;
}

}  // namespace

extern "C" int lt_tiff_encode_strips_dev(lt_ctx* c, const lt_encode_job* jobs, int n_jobs,
                                         void* stream_) {
  if (!c) return LT_ERR_ARG;
  if (n_jobs < 0 || (n_jobs > 0 && !jobs)) return lt::ctx_fail(c, LT_ERR_ARG, "null argument%s", "");
  int64_t max_raw = 0, max_strips = 0;
  std::vector<lt_encode_job> lzw;  // the compression 5 jobs: the lanes' work
  for (int k = 0; k < n_jobs; k++) {
    const lt_encode_job& J = jobs[k];
    if (!J.in || !J.out || !J.strip_sizes || !J.total || J.cap < 0 || J.bands <= 0 ||
        J.rows <= 0 || J.cols <= 0 || J.rows_per_strip <= 0 ||
        !(J.bps == 1 || J.bps == 2 || J.bps == 4 || J.bps == 8))
      return lt::ctx_fail(c, LT_ERR_ARG, "bad encode job%s", "");
    if ((J.compression != 1 && J.compression != 5) || (J.predictor != 1 && J.predictor != 2))
      return lt::ctx_fail(c, LT_ERR_ARG, "encode job: compression 1 or 5, predictor 1 or 2%s", "");
    if (J.predictor == 2 && (uintptr_t)J.in % (uintptr_t)J.bps != 0)
      return lt::ctx_fail(c, LT_ERR_ARG, "encode job: predictor 2 needs aligned samples%s", "");
    const int64_t nr = J.rows_per_strip < J.rows ? J.rows_per_strip : J.rows;
    if ((double)nr * (double)J.cols * (double)J.bps >= (double)lt_lzw::kCoreMaxOut)
      return lt::ctx_fail(c, LT_ERR_ARG, "strips of 1 MiB or more raw: the host path%s", "");
    if ((double)J.bands * (double)J.rows * (double)J.cols * (double)J.bps >= 4.0e18)
      return lt::ctx_fail(c, LT_ERR_ARG, "bad encode job%s", "");
    if (J.compression != 5) continue;
    lzw.push_back(J);
    if (nr * J.cols * J.bps > max_raw) max_raw = nr * J.cols * J.bps;
  }
  if (n_jobs == 0) return LT_OK;
  HIP_OR_FAIL(c, hipSetDevice(lt::ctx_device(c)));
  hipStream_t st = (hipStream_t)stream_;
  for (int k = 0; k < n_jobs; k++) {  // compression 1: one coalesced launch per raster
    const lt_encode_job& J = jobs[k];
    if (J.compression != 1) continue;
    const int64_t bytes = J.bands * J.rows * J.cols * J.bps;
    int64_t blocks = (bytes + 256 * 16 - 1) / (256 * 16);  // about 16 bytes a thread
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(raw_strips_kernel, dim3((unsigned)blocks), dim3(256), 0, st, J);
    HIP_OR_FAIL(c, hipGetLastError());
  }
  const int n_lzw = (int)lzw.size();
  if (n_lzw == 0) return LT_OK;
  for (int k0 = 0; k0 < n_lzw; k0 += kMaxJobs) {  // strips of the widest launch group
    int64_t total = 0;
    for (int k = k0; k < n_lzw && k < k0 + kMaxJobs; k++) total += job_strips(lzw[k]);
    if (total > max_strips) max_strips = total;
  }
  const int64_t slot_stride = (max_raw * 3 / 2 + 16 + 15) / 16 * 16;
  int64_t lanes = (max_strips + kWave - 1) / kWave * kWave;
  if (lanes > kMaxLanes) lanes = kMaxLanes;
  if (lanes * slot_stride > kSlotScratch) {  // a bounded buffer of slots, at least one wave
    lanes = kSlotScratch / (slot_stride * kWave) * kWave;
    if (lanes < kWave) lanes = kWave;
  }
  lt::EncodeSet* Sp;
  HIP_OR_FAIL(c, lt::ctx_encode(c).find(st, &Sp));
  lt::EncodeSet& S = *Sp;
  if (!S.d_meta)  // per lane a size and an offset, then per job a running total and an error word
    HIP_OR_FAIL(c, hipMalloc((void**)&S.d_meta, (size_t)(kMaxLanes * 12 + kMaxJobs * 12)));
  HIP_OR_FAIL(c, lt::grow(S.d_tables, S.tables_bytes,
                          lanes * lt_lzw::kEncSlots * (int64_t)sizeof(uint32_t)));
  HIP_OR_FAIL(c, lt::grow(S.d_slots, S.slots_bytes, lanes * slot_stride));
  int64_t* const slot_off = (int64_t*)S.d_meta;
  int64_t* const carry = slot_off + kMaxLanes;
  int32_t* const slot_size = (int32_t*)(carry + kMaxJobs);
  int32_t* const err = slot_size + kMaxLanes;
  for (int k0 = 0; k0 < n_lzw; k0 += kMaxJobs) {
    Batch B;
    B.n = 0;
    B.first[0] = 0;
    for (int k = k0; k < n_lzw && k < k0 + kMaxJobs; k++) {
      B.job[B.n] = lzw[k];
      B.first[B.n + 1] = B.first[B.n] + job_strips(lzw[k]);
      B.n++;
    }
    for (int k = B.n; k < kMaxJobs; k++) {
      B.job[k] = lt_encode_job();
      B.first[k + 1] = B.first[B.n];
    }
    HIP_OR_FAIL(c, hipMemsetAsync(carry, 0, kMaxJobs * sizeof(int64_t), st));
    HIP_OR_FAIL(c, hipMemsetAsync(err, 0, kMaxJobs * sizeof(int32_t), st));
    const int64_t total = B.first[B.n];
    for (int64_t s0 = 0; s0 < total; s0 += lanes) {
      const int64_t n = total - s0 < lanes ? total - s0 : lanes;
      const unsigned waves = (unsigned)((n + kWave - 1) / kWave);
      hipLaunchKernelGGL(encode_strips_kernel, dim3(waves), dim3(kWave), 0, st, B, s0, n,
                         S.d_tables, S.d_slots, slot_stride, slot_size);
      HIP_OR_FAIL(c, hipGetLastError());
      hipLaunchKernelGGL(scan_sizes_kernel, dim3(1), dim3(kScanThreads), 0, st, B, s0, n,
                         (const int32_t*)slot_size, slot_off, carry, err,
                         s0 + lanes >= total ? 1 : 0);
      HIP_OR_FAIL(c, hipGetLastError());
      hipLaunchKernelGGL(pack_strips_kernel, dim3((unsigned)n), dim3(kPackThreads), 0, st, B, s0,
                         n, (const uint8_t*)S.d_slots, slot_stride, (const int32_t*)slot_size,
                         (const int64_t*)slot_off);
      HIP_OR_FAIL(c, hipGetLastError());
    }
  }
  return LT_OK;
}
