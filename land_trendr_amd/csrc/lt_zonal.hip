// lt_zonal.hip — the per-zone, per-key table of a label plane on the device (lt_abi.h
// lt_zonal_stats).
//
// The per-pixel logic is lt_zonal.h, the source tests/native/zonal_host_check.hip compiles for the
// host. A lane is a pixel, 256 lanes a block, and a block walks a run of consecutive pixels, so
// the five planes are read coalesced (1 + 4 + 4 + 4 + 8 bytes a lane). Zones are spatially
// coherent: the lanes of a wave mostly share one (zone, key) cell, which is the shape that
// per-lane atomics on one address serialise on. Both paths therefore combine inside the wave
// before they touch the table:
//
//   wave_add  the lanes that share the first active lane's cell are found with a ballot, their
//             addends summed across the wave (the two counts are the ballots' population counts,
//             the duration and magnitude sums a 64-bit butterfly), and that one lane adds; a cell
//             that only one lane holds skips the butterfly.
//
//   path 1 (LDS)   (n_zones + 1) * (n_bins + 1) <= kZonalLdsCells: a block-private table in LDS.
//             A wave whose active lanes all share one cell (the common case) adds once through
//             wave_add; any other wave adds per lane with LDS atomics, which meet on few
//             addresses there. The block then adds its non-zero words to the global table, one
//             64-bit atomic each.
//   path 2 (wave)  any table: wave_add repeated until every active lane is retired, one set of
//             global 64-bit atomics per distinct cell per wave.
//
// All adds are unsigned 64-bit integer adds (agent scope), so every path gives the same table in
// every word, run after run. No scratch. Nothing here waits for the device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lt_abi.h"
#include "lt_launch.h"
#include "lt_zonal.h"

namespace {

constexpr int kBlock = 256;
// pixels a block walks: multiples of the block. The LDS path pays a table's clear and flush per
// block, so its runs are long (counts_kernel's figure); the wave path has nothing to amortise.
// Neither figure has been timed against another.
constexpr int64_t kLdsPerBlock = 256 * 64;
constexpr int64_t kWavePerBlock = 256 * 8;

typedef unsigned long long u64;

// the sum of v over the wave's lanes (all 64 execute this)
__device__ inline u64 wave_sum(u64 v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += (u64)__shfl_xor((long long)v, s, 64);
  return v;
}

// One round of the combine, executed by all 64 lanes: the lanes of `todo` that hold the cell of
// todo's first lane are summed and that lane adds the sums to tab[cell]; returns those lanes' mask.
// `todo` is non-zero and holds only lanes with x.cell >= 0.
template <class Add>
__device__ inline uint64_t wave_add(uint64_t todo, const lt::ZonalPix& x, Add add) {
  const int lane = (int)__lane_id();
  const int leader = __ffsll((long long)todo) - 1;
  const int32_t cell = __shfl(x.cell, leader, 64);
  const bool peer = ((todo >> lane) & 1) != 0 && x.cell == cell;
  const uint64_t peers = __ballot(peer);
  const uint64_t valued = __ballot(peer && x.has_value != 0);
  u64 dur = (u64)x.dur, q = (u64)x.q;
  if (peers != (1ull << leader)) {  // (uniform) more than one lane: sum theirs
    dur = wave_sum(peer ? dur : 0);
    q = wave_sum(peer ? q : 0);
  }
  if (lane == leader)
    add(cell, (u64)__popcll(peers), dur, q, (u64)__popcll(valued));
  return peers;
}

// (words that would add zero are skipped: a null duration or value plane costs no atomic)
__device__ inline void add_words(u64* cell_words, u64 n, u64 dur, u64 q, u64 nv) {
  atomicAdd(&cell_words[0], n);
  if (dur != 0) atomicAdd(&cell_words[1], dur);
  if (q != 0) atomicAdd(&cell_words[2], q);
  if (nv != 0) atomicAdd(&cell_words[3], nv);
}

__global__ __launch_bounds__(kBlock) void zonal_lds_kernel(const lt::ZonalArgs A) {
  extern __shared__ u64 tab[];  // [cells][4]
  const int words = (A.n_zones + 1) * (A.n_bins + 1) * lt::kZonalWords;  // <= 4096
  for (int w = threadIdx.x; w < words; w += kBlock) tab[w] = 0;
  __syncthreads();
  const int64_t p0 = (int64_t)blockIdx.x * kLdsPerBlock;
  const int64_t p1 = p0 + kLdsPerBlock < A.n_pix ? p0 + kLdsPerBlock : A.n_pix;
  // (the bound is the block's: every lane of a wave runs every iteration, as the ballots need)
  for (int64_t base = p0; base < p1; base += kBlock) {
    const int64_t p = base + threadIdx.x;
    lt::ZonalPix x = {-1, 0, 0, 0};
    if (p < p1) x = lt::zonal_pixel(A, p);
    const uint64_t active = __ballot(x.cell >= 0);
    if (active == 0) continue;
    const int32_t first = __shfl(x.cell, __ffsll((long long)active) - 1, 64);
    if (__ballot(x.cell >= 0 && x.cell != first) == 0) {  // one cell in the wave
      wave_add(active, x, [&](int32_t cell, u64 n, u64 dur, u64 q, u64 nv) {
        add_words(&tab[cell * lt::kZonalWords], n, dur, q, nv);
      });
    } else if (x.cell >= 0) {
      add_words(&tab[x.cell * lt::kZonalWords], 1, (u64)x.dur, (u64)x.q, (u64)x.has_value);
    }
  }
  __syncthreads();
  for (int w = threadIdx.x; w < words; w += kBlock) {
    const u64 v = tab[w];
    if (v != 0) atomicAdd(&A.table[w], v);
  }
}

__global__ __launch_bounds__(kBlock) void zonal_wave_kernel(const lt::ZonalArgs A) {
  const int64_t p0 = (int64_t)blockIdx.x * kWavePerBlock;
  const int64_t p1 = p0 + kWavePerBlock < A.n_pix ? p0 + kWavePerBlock : A.n_pix;
  for (int64_t base = p0; base < p1; base += kBlock) {
    const int64_t p = base + threadIdx.x;
    lt::ZonalPix x = {-1, 0, 0, 0};
    if (p < p1) x = lt::zonal_pixel(A, p);
    uint64_t todo = __ballot(x.cell >= 0);
    // every round retires at least the first lane of `todo`, so a wave is done in at most 64
    // rounds (64 distinct cells); `todo` is the same in every lane, so the loop is uniform
    while (todo != 0) {
      todo &= ~wave_add(todo, x, [&](int32_t cell, u64 n, u64 dur, u64 q, u64 nv) {
        add_words(&A.table[(int64_t)cell * lt::kZonalWords], n, dur, q, nv);
      });
    }
  }
}

}  // namespace

extern "C" int lt_zonal_stats(lt_ctx* c, const uint8_t* matched, const int32_t* zone,
                              const int32_t* key, const int32_t* duration, const double* value,
                              int64_t n_pix, int32_t key_lo, int32_t n_bins, int32_t n_zones,
                              int32_t path, uint64_t* table, void* stream_) {
  if (!c) return LT_ERR_ARG;
  const char* why;
  const int rc = lt::zonal_check(matched, zone, key, n_pix, n_bins, n_zones, path, table, &why);
  if (rc != LT_OK) return lt::ctx_fail(c, rc, "lt_zonal_stats: %s", why);
  if (n_pix == 0) return LT_OK;
  hipError_t e = hipSetDevice(lt::ctx_device(c));
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  const lt::ZonalArgs A = {matched, zone, key, duration, value, n_pix, key_lo, n_bins, n_zones,
                           (unsigned long long*)table};
  hipStream_t stream = (hipStream_t)stream_;
  if (lt::zonal_path(path, n_zones, n_bins) == lt::kZonalLds) {
    const unsigned blocks = (unsigned)((n_pix + kLdsPerBlock - 1) / kLdsPerBlock);
    const size_t lds = (size_t)lt::zonal_cells(n_zones, n_bins) * lt::kZonalWords * sizeof(u64);
    hipLaunchKernelGGL(zonal_lds_kernel, dim3(blocks), dim3(kBlock), lds, stream, A);
  } else {
    const unsigned blocks = (unsigned)((n_pix + kWavePerBlock - 1) / kWavePerBlock);
    hipLaunchKernelGGL(zonal_wave_kernel, dim3(blocks), dim3(kBlock), 0, stream, A);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return lt::ctx_fail(c, LT_ERR_HIP, "zonal kernel: %s", hipGetErrorString(e));
  return LT_OK;
}
