// lt_launch.h — what lt_abi.hip hands the analyze-stage dispatch for one tile, and what it shares
// with the strip decoder (lt_decode.hip) and the strip encoder (lt_encode.hip).
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

// The strip decoder's share of a context (lt_decode.hip, lt_tiff_decode_strips_dev): scratch grown
// on demand, freed with the context (decode_release, called by lt_ctx_destroy). One set per stream
// the decoder was called on: launches on one stream run one after the other and share a set, while
// several rasters decode side by side on streams of their own.
struct DecodeScratch {
  struct Set {
    uint32_t* d_tables = nullptr;  // the lanes' LZW string tables: [waves][4096 entries][64 lanes]
    int64_t table_lanes = 0;
    uint8_t* d_strips = nullptr;   // chunky images: one decoded strip per lane (de-interleaved
    int64_t strips_bytes = 0;      // from there)
  };
  static constexpr int kMaxSets = 16;
  hipStream_t stream[kMaxSets] = {};
  Set set[kMaxSets];
  int n_sets = 0;
};
void decode_release(DecodeScratch& s);
// The strip encoder's share of a context (lt_encode.hip, lt_tiff_encode_strips_dev): scratch grown
// on demand, freed with the context (encode_release), one set per stream like the decoder's.
struct EncodeScratch {
  struct Set {
    uint32_t* d_tables = nullptr;  // the lanes' LZW dictionaries: [waves][8192 slots][64 lanes]
    int64_t table_lanes = 0;
    uint8_t* d_slots = nullptr;    // one worst-case encoded strip per lane
    int64_t slots_bytes = 0;
    void* d_meta = nullptr;        // per lane a size and an offset, per job a total and an error
  };
  static constexpr int kMaxSets = 16;
  static constexpr int64_t kMaxLanes = 32768;  // in flight: 1 GiB of dictionaries
  hipStream_t stream[kMaxSets] = {};
  Set set[kMaxSets];
  int n_sets = 0;
};
void encode_release(EncodeScratch& s);
// The chunk decoder's share of a context (lt_chunks.hip, lt_tiff_decode_chunks_dev): scratch grown
// on demand, freed with the context (chunks_release), one set per stream like the strip decoder's.
struct ChunkScratch {
  struct Set {
    uint32_t* d_tables = nullptr;  // LZW images: the lanes' string tables, as DecodeScratch's
    int64_t table_lanes = 0;
    uint8_t* d_chunks = nullptr;   // tiles and chunky chunks: one decoded chunk per lane
    int64_t chunks_bytes = 0;
  };
  static constexpr int kMaxSets = 16;
  hipStream_t stream[kMaxSets] = {};
  Set set[kMaxSets];
  int n_sets = 0;
};
void chunks_release(ChunkScratch& s);
// What lt_decode.hip and lt_encode.hip need of a context (defined in lt_abi.hip beside lt_ctx).
DecodeScratch& ctx_decode(lt_ctx* c);
EncodeScratch& ctx_encode(lt_ctx* c);
ChunkScratch& ctx_chunks(lt_ctx* c);
int ctx_device(const lt_ctx* c);
// the context's x-set factor table (lt_lapack.h), as the fit-to-vertex kernel reads it (lt_ftv.hip)
const lsq_xf* ctx_xtab(const lt_ctx* c);
int ctx_fail(lt_ctx* c, int code, const char* fmt, const char* detail);

// Stage 1: the analyze kernel over every pixel of the tile, on l.stream.
hipError_t launch_analyze(const TileLaunch& l);
// Stage 2: the resolve kernels over the pixels stage 1 deferred, on l.stream.
hipError_t launch_resolve(const TileLaunch& l);

}  // namespace lt
