// lt_launch.h — what lt_abi.hip hands the analyze-stage dispatch for one tile, and what it shares
// with the TIFF decoder (lt_chunks.hip) and the strip encoder (lt_encode.hip).
//
// The kernels of the analyze and resolve stages (lt_kernels.h) are instantiated in a dispatch
// translation unit of their own: lt_dispatch.hip in the product library, a profiling unit in the
// profiling builds (profiles/). lt_abi.hip (contexts, argument checks, scene upload, streams,
// events) only sees this record and the two entry points below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lt_abi.h"
#include "lt_pixel.h"

namespace lt {

struct TileLaunch {
  const DevScene* scene;         // device copy of the tile's scene
  const lt_params* params;       // host struct (passed by value to the kernels)
  const lt_tile_in* in;
  const lt_tile_out* out;
  const lsq_xf* xtab;            // the context's x-set factor table
  int64_t* defer;                // [2][n_pix]: the binary32 and the binary64 deferred lists
  unsigned long long* counters;  // [4]: list counts [0]/[2], resolve work counters [1]/[3]
  uint64_t* yflags;              // [2][n_pix] spike / vertex year flags, or null
  int n_years;                   // Y
  int device;
  hipStream_t stream;
  uint64_t* tl_bits = nullptr;   // the compact trendline ([4][n_pix] words), or null
  double* tl_eqn = nullptr;      // its segment eqns ([Y-1][n_pix] (m, b) pairs)
};

// Scratch a context keeps for the TIFF decoder and encoder: grown on demand, freed with the context
// (release, called by lt_ctx_destroy). One set per stream an entry was called on: launches on one
// stream run one after the other and share a set, while several rasters are decoded or encoded
// side by side on streams of their own.
template <class Set>
struct StreamSets {
  static constexpr int kMaxSets = 16;
  hipStream_t stream[kMaxSets] = {};
  Set set[kMaxSets];
  int n_sets = 0;
  void release() {
    for (int k = 0; k < n_sets; k++) {
      set[k].release();
      set[k] = Set();
    }
    n_sets = 0;
  }
  // this stream's set, or a new one; more streams than sets: wait for the device and start over
  hipError_t find(hipStream_t st, Set** out) {
    for (int k = 0; k < n_sets; k++)
      if (stream[k] == st) {
        *out = &set[k];
        return hipSuccess;
      }
    if (n_sets == kMaxSets) {
      const hipError_t e = hipDeviceSynchronize();
      if (e != hipSuccess) return e;
      release();
    }
    stream[n_sets] = st;
    set[n_sets] = Set();
    *out = &set[n_sets++];
    return hipSuccess;
  }
};
// the device buffer `d` of `have` bytes grown to at least n, its contents dropped (hipFree waits
// for the launches still using it)
template <class T>
inline hipError_t grow(T*& d, int64_t& have, int64_t n) {
  if (have >= n) return hipSuccess;
  if (d) {
    const hipError_t e = hipFree(d);
    if (e != hipSuccess) return e;
  }
  d = nullptr;
  have = 0;
  const hipError_t e = hipMalloc((void**)&d, (size_t)n);
  if (e == hipSuccess) have = n;
  return e;
}
// The TIFF decoder's set (lt_chunks.hip; lt_tiff_decode_strips_dev and lt_tiff_decode_chunks_dev
// share it).
struct DecodeSet {
  uint32_t* d_tables = nullptr;  // LZW images: the lanes' string tables,
  int64_t tables_bytes = 0;      // [waves][4096 entries][64 lanes]
  uint8_t* d_chunks = nullptr;   // tiles and chunky chunks: one decoded chunk per lane (copied
  int64_t chunks_bytes = 0;      // into the planes from there)
  void release() {
    if (d_tables) (void)hipFree(d_tables);
    if (d_chunks) (void)hipFree(d_chunks);
  }
};
using DecodeScratch = StreamSets<DecodeSet>;
// The strip encoder's set (lt_encode.hip, lt_tiff_encode_strips_dev).
struct EncodeSet {
  static constexpr int64_t kMaxLanes = 32768;  // in flight: 1 GiB of dictionaries
  uint32_t* d_tables = nullptr;  // the lanes' LZW dictionaries: [waves][8192 slots][64 lanes]
  int64_t tables_bytes = 0;
  uint8_t* d_slots = nullptr;    // one worst-case encoded strip per lane
  int64_t slots_bytes = 0;
  void* d_meta = nullptr;        // per lane a size and an offset, per job a total and an error
  void release() {
    if (d_tables) (void)hipFree(d_tables);
    if (d_slots) (void)hipFree(d_slots);
    if (d_meta) (void)hipFree(d_meta);
  }
};
using EncodeScratch = StreamSets<EncodeSet>;
// What lt_chunks.hip and lt_encode.hip need of a context (defined in lt_abi.hip beside lt_ctx).
DecodeScratch& ctx_decode(lt_ctx* c);
EncodeScratch& ctx_encode(lt_ctx* c);
int ctx_device(const lt_ctx* c);
// the context's x-set factor table (lt_lapack.h), as the fit-to-vertex kernel reads it (lt_ftv.hip)
const lsq_xf* ctx_xtab(const lt_ctx* c);
int ctx_fail(lt_ctx* c, int code, const char* fmt, const char* detail);
// (in the entry points: a failing HIP call ends the entry with LT_ERR_HIP and its message)
#define HIP_OR_FAIL(ctx, expr)                                                   \
  do {                                                                           \
    hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess)                                                        \
      return lt::ctx_fail(ctx, LT_ERR_HIP, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

// Stage 1: the analyze kernel over every pixel of the tile, on l.stream.
hipError_t launch_analyze(const TileLaunch& l);
// Stage 2: the resolve kernels over the pixels stage 1 deferred, on l.stream.
hipError_t launch_resolve(const TileLaunch& l);

}  // namespace lt
