// lt_sieve.h — the MMU sieve's phase bodies and argument checks (lt_abi.h lt_sieve_labels), host
// and device: one source for the kernels (lt_sieve.hip) and for their serial host twin
// (tests/native/sieve_host_check.hip, tests/native/sieve_core_check.cpp).
//
// Connected-component labelling by union-find in four launches:
//   1 local    one workgroup per kSvTW x kSvTH raster tile: unions in LDS, the root the tile-local
//              minimum index; writes parent[q] as a global index (-1 unmatched), the local
//              component's pixel count at its local root (in `size`), 0 in size_at_root
//   2 merge    one lane per tile-border pixel: union across the border on the global parent array
//   3 resolve  every local root finds its global root, writes root[] there and adds its local count
//              to size_at_root[root]: one atomic per local component
//   4 expand   root[q] = root[parent[q]], size[q] = size_at_root[root[q]], the optional clear
//
// The invariant behind every loop: parent[x] <= x for every matched x at all times, and a word
// only ever decreases (a link is a min with a smaller index). find() therefore walks a strictly
// decreasing chain of non-negative indices and stops within x steps; unite() either ends or goes
// on with a strictly smaller larger-root (the value its min returned, which is below the root it
// tried), so the sum of its two indices strictly decreases: bounded by construction, whatever other
// lanes do meanwhile. The final root of a patch is its smallest index, the sizes are integer sums:
// the outputs are functions of the input alone.
//
// A phase is a sequence of steps between workgroup barriers; a step is a __host__ __device__
// function of (arguments, block, lane, the block's shared words). The kernel runs a step in every
// lane and then meets the barrier; the host twin runs it lane after lane, block after block.
#pragma once
#include <stdint.h>

#include "../../include/lt_abi.h"

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

// Atomics: on the device relaxed HIP atomics (LDS words at workgroup scope; global parent /
// counter words at agent scope, so no load is served from a stale L1 / L2 line while other
// workgroups write the array in the same launch); on the host, where lanes run in turn, plain code.
#if defined(__HIP_DEVICE_COMPILE__)
#define LT_SV_LOAD_L(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define LT_SV_STORE_L(p, v) \
  __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define LT_SV_MIN_L(p, v) \
  __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define LT_SV_ADD_L(p, v) \
  __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define LT_SV_LOAD_G(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define LT_SV_MIN_G(p, v) \
  __hip_atomic_fetch_min((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define LT_SV_ADD_G(p, v) \
  __hip_atomic_fetch_add((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#else
namespace lt {
inline int32_t sv_host_min(int32_t* p, int32_t v) {
  const int32_t o = *p;
  if (v < o) *p = v;
  return o;
}
inline int32_t sv_host_add(int32_t* p, int32_t v) {
  const int32_t o = *p;
  *p = o + v;
  return o;
}
}  // namespace lt
#define LT_SV_LOAD_L(p) (*(p))
#define LT_SV_STORE_L(p, v) (*(p) = (v))
#define LT_SV_MIN_L(p, v) lt::sv_host_min((p), (v))
#define LT_SV_ADD_L(p, v) lt::sv_host_add((p), (v))
#define LT_SV_LOAD_G(p) (*(p))
#define LT_SV_MIN_G(p, v) lt::sv_host_min((p), (v))
#define LT_SV_ADD_G(p, v) lt::sv_host_add((p), (v))
#endif

namespace lt {

// The tile: 64 columns (a row of int32 keys is one 256-byte run) by 16 rows, 1024 pixels, four
// neighbouring pixels of a row per lane of a 256-lane block. Two int32 words of LDS per pixel
// (8 KiB a block: the CU's LDS holds many blocks, the wave slots are the limit).
constexpr int kSvTW = 64, kSvTH = 16, kSvTile = kSvTW * kSvTH;
constexpr int kSvBlock = 256, kSvPer = kSvTile / kSvBlock;
// the border lanes of a tile: its first row, and rows 1.. of its first and last column
constexpr int kSvBorder = kSvTW + 2 * (kSvTH - 1);

struct SieveShared {
  int32_t lab[kSvTile];  // tile-local parent (-1: unmatched or outside the raster)
  int32_t aux[kSvTile];  // the key during the unions, then the local component counts
};

struct SieveArgs {
  int32_t H, W;        // raster rows / columns (P = H * W <= LT_MAX_TILE_PIX < 2^31)
  int32_t tx, ty;      // tiles per row / per column
  int32_t conn8, min_pixels, apply;
  uint8_t* matched;
  const int32_t* key;
  int32_t* root;
  int32_t* size;       // launches 1-3: the local count at each local root, 0 elsewhere
  int32_t* parent;     // workspace [P]
  int32_t* at_root;    // workspace [P]: size_at_root
};

inline int64_t sieve_workspace_bytes(int64_t rows, int64_t cols) {
  if (rows < 0 || cols < 0) return -1;
  if (rows == 0 || cols == 0) return 8;
  if (rows > LT_MAX_TILE_PIX / cols) return -1;
  return 8 * rows * cols;
}

// the argument checks of lt_sieve_labels, shared with the host twin: LT_OK or the LT_ERR_* code and
// what to say (rows * cols == 0 is LT_OK too: the caller returns before it launches anything).
// Nothing is dereferenced but the two structs.
inline int sieve_check(const lt_sieve_in* in, const lt_sieve_out* out, const char** why) {
  *why = "";
  if (!in || !out) return *why = "null argument", LT_ERR_ARG;
  if (in->rows < 0 || in->cols < 0) return *why = "negative rows or cols", LT_ERR_ARG;
  if (in->rows == 0 || in->cols == 0) return LT_OK;
  if (in->rows > LT_MAX_TILE_PIX / in->cols)
    return *why = "rows * cols above LT_MAX_TILE_PIX", LT_ERR_LIMIT;
  if (!in->matched || !out->root || !out->size || !out->workspace)
    return *why = "matched, root, size and workspace required", LT_ERR_ARG;
  if (in->connectivity != 4 && in->connectivity != 8)
    return *why = "connectivity must be 4 or 8", LT_ERR_ARG;
  if (in->min_pixels < 1) return *why = "min_pixels below 1", LT_ERR_ARG;
  if (in->phases < 0 || in->phases > 15) return *why = "phases outside [0, 15]", LT_ERR_ARG;
  if (out->workspace_bytes < sieve_workspace_bytes(in->rows, in->cols))
    return *why = "workspace below lt_sieve_workspace_bytes", LT_ERR_ARG;
  return LT_OK;
}

inline void sieve_args(const lt_sieve_in* in, const lt_sieve_out* out, SieveArgs& A) {
  A.H = (int32_t)in->rows;
  A.W = (int32_t)in->cols;
  A.tx = (A.W + kSvTW - 1) / kSvTW;
  A.ty = (A.H + kSvTH - 1) / kSvTH;
  A.conn8 = in->connectivity == 8;
  A.min_pixels = in->min_pixels;
  A.apply = in->apply != 0;
  A.matched = in->matched;
  A.key = in->key;
  A.root = out->root;
  A.size = out->size;
  A.parent = (int32_t*)out->workspace;
  A.at_root = A.parent + (int64_t)A.H * A.W;
}
__host__ __device__ inline int64_t sieve_tiles(const SieveArgs& A) { return (int64_t)A.tx * A.ty; }
__host__ __device__ inline int64_t sieve_pixels(const SieveArgs& A) { return (int64_t)A.H * A.W; }

// ---- union-find on a block's LDS words ----
__host__ __device__ inline int32_t sv_find_l(int32_t* lab, int32_t x) {
  for (;;) {  // a strictly decreasing chain of non-negative indices
    const int32_t p = LT_SV_LOAD_L(&lab[x]);
    if (p >= x || p < 0) return x;
    x = p;
  }
}
__host__ __device__ inline void sv_unite_l(int32_t* lab, int32_t a, int32_t b) {
  for (;;) {  // a + b strictly decreases
    a = sv_find_l(lab, a);
    b = sv_find_l(lab, b);
    if (a == b) return;
    if (a < b) { const int32_t t = a; a = b; b = t; }
    const int32_t old = LT_SV_MIN_L(&lab[a], b);
    if (old == a) return;  // a was still a root: linked
    a = old;               // linked in the meantime (old < a): old and b are still to be joined
  }
}
// ---- and on the global parent array (every access an agent-scope atomic) ----
__host__ __device__ inline int32_t sv_find_g(int32_t* parent, int32_t x) {
  for (;;) {
    const int32_t p = LT_SV_LOAD_G(&parent[x]);
    if (p >= x || p < 0) return x;
    x = p;
  }
}
__host__ __device__ inline void sv_unite_g(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = sv_find_g(parent, a);
    b = sv_find_g(parent, b);
    if (a == b) return;
    if (a < b) { const int32_t t = a; a = b; b = t; }
    const int32_t old = LT_SV_MIN_G(&parent[a], b);
    if (old == a) return;
    a = old;
  }
}

// the raster index of local pixel i of tile `block`, or -1 outside the raster
__host__ __device__ inline int32_t sv_global(const SieveArgs& A, int64_t block, int32_t i) {
  const int32_t y = (int32_t)(block / A.tx) * kSvTH + i / kSvTW;
  const int32_t x = (int32_t)(block % A.tx) * kSvTW + i % kSvTW;
  return (y < A.H && x < A.W) ? y * A.W + x : -1;
}

// ---- launch 1: the local phase, five steps ----
__host__ __device__ inline void sieve_local_load(const SieveArgs& A, int64_t block, int lane,
                                                 SieveShared& S) {
  for (int k = 0; k < kSvPer; k++) {
    const int32_t i = lane * kSvPer + k;
    const int32_t q = sv_global(A, block, i);
    const bool m = q >= 0 && A.matched[q] != 0;
    S.lab[i] = m ? i : -1;
    S.aux[i] = (m && A.key) ? A.key[q] : 0;
  }
}
// is local pixel j matched with key k?
__host__ __device__ inline bool sv_same_l(SieveShared& S, int32_t j, int32_t k) {
  return LT_SV_LOAD_L(&S.lab[j]) >= 0 && S.aux[j] == k;
}
// Each pixel joins its west and north neighbours in the tile; with 8-connectivity the north-east
// one unless the north one qualifies (those two are west-east neighbours, joined by that link),
// and the north-west one unless the north or the west one does.
__host__ __device__ inline void sieve_local_unite(const SieveArgs& A, int lane, SieveShared& S) {
  for (int k = 0; k < kSvPer; k++) {
    const int32_t i = lane * kSvPer + k;
    if (LT_SV_LOAD_L(&S.lab[i]) < 0) continue;
    const int32_t key = S.aux[i];
    const int lx = i % kSvTW, ly = i / kSvTW;
    const bool w = lx > 0 && sv_same_l(S, i - 1, key);
    const bool n = ly > 0 && sv_same_l(S, i - kSvTW, key);
    if (w) sv_unite_l(S.lab, i, i - 1);
    if (n) sv_unite_l(S.lab, i, i - kSvTW);
    if (A.conn8 && ly > 0 && !n) {
      if (lx + 1 < kSvTW && sv_same_l(S, i - kSvTW + 1, key)) sv_unite_l(S.lab, i, i - kSvTW + 1);
      if (!w && lx > 0 && sv_same_l(S, i - kSvTW - 1, key)) sv_unite_l(S.lab, i, i - kSvTW - 1);
    }
  }
}
// Every pixel points at its local root (roots keep their word: only non-roots are written, with
// an ancestor, so a lane that walks through a word meanwhile still arrives); the keys are done
// with: aux becomes the counters.
__host__ __device__ inline void sieve_local_flatten(int lane, SieveShared& S) {
  for (int k = 0; k < kSvPer; k++) {
    const int32_t i = lane * kSvPer + k;
    S.aux[i] = 0;
    if (LT_SV_LOAD_L(&S.lab[i]) < 0) continue;
    const int32_t r = sv_find_l(S.lab, i);
    if (r != i) LT_SV_STORE_L(&S.lab[i], r);
  }
}
// The local counts: a lane's neighbouring pixels that share a root make one add.
__host__ __device__ inline void sieve_local_count(int lane, SieveShared& S) {
  int32_t run_root = -1, run = 0;
  for (int k = 0; k < kSvPer; k++) {
    const int32_t r = S.lab[lane * kSvPer + k];
    if (r != run_root) {
      if (run > 0) LT_SV_ADD_L(&S.aux[run_root], run);
      run_root = r;
      run = 0;
    }
    if (r >= 0) run++;
  }
  if (run > 0) LT_SV_ADD_L(&S.aux[run_root], run);
}
__host__ __device__ inline void sieve_local_store(const SieveArgs& A, int64_t block, int lane,
                                                  const SieveShared& S) {
  for (int k = 0; k < kSvPer; k++) {
    const int32_t i = lane * kSvPer + k;
    const int32_t q = sv_global(A, block, i);
    if (q < 0) continue;
    const int32_t r = S.lab[i];
    A.parent[q] = r < 0 ? -1 : sv_global(A, block, r);
    A.size[q] = r == i ? S.aux[i] : 0;
    A.at_root[q] = 0;
  }
}

// ---- launch 2: the border merge; g counts (tile, border lane) pairs ----
// A border pixel joins the neighbours of its west / north side that lie in another tile, by the
// rules of the local phase (a link those rules leave out is made by the lane that owns the
// west-east or north-south link it rests on, in this launch or in the tile). Whether a neighbour
// is matched is read from parent (>= 0), whose every access here is atomic.
__host__ __device__ inline bool sv_same_g(const SieveArgs& A, int32_t n, int32_t key) {
  return LT_SV_LOAD_G(&A.parent[n]) >= 0 && (A.key ? A.key[n] : 0) == key;
}
__host__ __device__ inline void sieve_merge(const SieveArgs& A, int64_t g) {
  const int64_t tile = g / kSvBorder;
  const int l = (int)(g % kSvBorder);
  if (tile >= sieve_tiles(A)) return;
  int lx, ly;
  if (l < kSvTW) { ly = 0; lx = l; }
  else if (l < kSvTW + kSvTH - 1) { ly = l - kSvTW + 1; lx = 0; }
  else { ly = l - (kSvTW + kSvTH - 1) + 1; lx = kSvTW - 1; }
  const int32_t y = (int32_t)(tile / A.tx) * kSvTH + ly;
  const int32_t x = (int32_t)(tile % A.tx) * kSvTW + lx;
  if (y >= A.H || x >= A.W) return;
  const int32_t q = y * A.W + x;
  if (LT_SV_LOAD_G(&A.parent[q]) < 0) return;
  const int32_t key = A.key ? A.key[q] : 0;
  const bool w = x > 0 && sv_same_g(A, q - 1, key);
  const bool n = y > 0 && sv_same_g(A, q - A.W, key);
  if (w && lx == 0) sv_unite_g(A.parent, q, q - 1);
  if (n && ly == 0) sv_unite_g(A.parent, q, q - A.W);
  if (A.conn8 && y > 0 && !n) {
    if ((ly == 0 || lx == kSvTW - 1) && x + 1 < A.W && sv_same_g(A, q - A.W + 1, key))
      sv_unite_g(A.parent, q, q - A.W + 1);
    if (!w && (ly == 0 || lx == 0) && x > 0 && sv_same_g(A, q - A.W - 1, key))
      sv_unite_g(A.parent, q, q - A.W - 1);
  }
}

// ---- launch 3: every local root (the pixels with a local count) resolves its global root ----
// parent is only read here (plain loads: an earlier launch wrote it).
__host__ __device__ inline void sieve_resolve(const SieveArgs& A, int64_t q) {
  if (q >= sieve_pixels(A)) return;
  const int32_t c = A.size[q];
  if (c == 0) return;
  int32_t r = (int32_t)q;
  for (;;) {  // strictly decreasing, as sv_find_g
    const int32_t p = A.parent[r];
    if (p >= r || p < 0) break;
    r = p;
  }
  A.root[q] = r;
  LT_SV_ADD_G(&A.at_root[r], c);
}

// ---- launch 4: every pixel takes its root and size from its local root's ----
// parent[q] of a matched pixel is a local root (its tile's, or for a local root that was linked,
// the root it was linked to), whose root[] launch 3 wrote; only pixels that are no local root
// write root[] here, so no word is read and written in this launch.
__host__ __device__ inline void sieve_expand(const SieveArgs& A, int64_t q) {
  if (q >= sieve_pixels(A)) return;
  const int32_t p = A.parent[q];
  if (p < 0) {
    A.root[q] = -1;
    A.size[q] = 0;
    return;
  }
  const bool local_root = A.size[q] != 0;
  const int32_t r = A.root[p];
  if (!local_root) A.root[q] = r;
  const int32_t s = A.at_root[r];
  A.size[q] = s;
  if (A.apply && s < A.min_pixels) A.matched[q] = 0;
}

// The serial twin of the four launches: each step over a block's lanes in turn, block after block
// (reverse: the blocks of every launch from the last to the first).
inline void sieve_host(const SieveArgs& A, bool reverse) {
  const int64_t T = sieve_tiles(A), P = sieve_pixels(A);
  SieveShared S;
  for (int64_t k = 0; k < T; k++) {
    const int64_t b = reverse ? T - 1 - k : k;
    for (int l = 0; l < kSvBlock; l++) sieve_local_load(A, b, l, S);
    for (int l = 0; l < kSvBlock; l++) sieve_local_unite(A, l, S);
    for (int l = 0; l < kSvBlock; l++) sieve_local_flatten(l, S);
    for (int l = 0; l < kSvBlock; l++) sieve_local_count(l, S);
    for (int l = 0; l < kSvBlock; l++) sieve_local_store(A, b, l, S);
  }
  const int64_t mb = (T * kSvBorder + kSvBlock - 1) / kSvBlock;
  const int64_t pb = (P + kSvBlock - 1) / kSvBlock;
  for (int64_t k = 0; k < mb; k++) {
    const int64_t b = reverse ? mb - 1 - k : k;
    for (int l = 0; l < kSvBlock; l++) sieve_merge(A, b * kSvBlock + l);
  }
  for (int64_t k = 0; k < pb; k++) {
    const int64_t b = reverse ? pb - 1 - k : k;
    for (int l = 0; l < kSvBlock; l++) sieve_resolve(A, b * kSvBlock + l);
  }
  for (int64_t k = 0; k < pb; k++) {
    const int64_t b = reverse ? pb - 1 - k : k;
    for (int l = 0; l < kSvBlock; l++) sieve_expand(A, b * kSvBlock + l);
  }
}

}  // namespace lt
