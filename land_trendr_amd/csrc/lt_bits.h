// lt_bits.h — the per-pixel point masks of the analyze / resolve kernels (lt_fast.h, lt_pixel.h
// RuleCands): sets of year slots, present points, non-spike points or vertex numbers of ONE
// pixel, one bit each, held per lane.
//
// Every index of such a set is below the instance's MAXY, so an instance of at most 32 years
// needs 32 bits. The compiler cannot see that (the shift amounts are run-time values) and emits
// full 64-bit code for a uint64_t mask: v_lshlrev_b64 for a per-lane 1 << k, two selects and two
// ORs for a conditional |=, two find-first-bit instructions, an add and a min for ctz, a carry
// chain for m & (m - 1). PointBits<MAXY>::type is uint32_t for MAXY <= 32 (LT_MASK32, default on)
// and uint64_t otherwise; the LT_PB_* helpers below hold every operation that depends on the
// width, and are the only place that knows it.
//
// The helpers are macros over the mask type M, not functions: with M = uint64_t each expands to
// the expression the kernels had ((uint64_t)1 << k is the constant 1ull; of the two arms of a
// sizeof test only the live one is compiled), so with LT_MASK32=0, and in the instances above 32
// years, the kernels compile to the code they had, instruction for instruction. (Inlined functions
// did not: the backtrack loop of the lazy DP came out with its n - 1 computed twice and its
// instructions in another order.) Their arguments are evaluated more than once: plain variables
// and side-effect-free expressions only.
//
// What stays 64-bit whatever the instance: wave masks (__ballot), DevScene::feb29_mask, and the
// yflags / tl_bits planes of the ABI (a mask is widened at its store).
//
// Conditions the callers keep (all shifts are on unsigned types by amounts below the width):
//   BIT(k), m >> k     0 <= k < MAXY
//   BELOW(k)           (1 << k) - 1, 0 <= k < MAXY (never the width itself)
//   ABOVE(k)           ~((2 << k) - 1), 0 <= k < MAXY; k = width - 1 gives 0: 2 << k drops its bit,
//                      0 - 1 is all ones, and the complement is empty (no vertex above the last
//                      point)
//   TWO(k)             2 << k, 0 <= k < MAXY; k = width - 1 gives 0: the dropped bit would describe
//                      point index MAXY, which no series has
//   CTZ(m), TOP(m)     m != 0 where the result is used (a lane that does not use it passes a
//                      nonzero placeholder or discards the result in a select)
#pragma once
#ifndef __HIPCC_RTC__  // hiprtc (the JIT kernels, lt_jit.h) brings its own
#include <stdint.h>
#endif

// 32-bit point masks in the instances of at most 32 years (A/B runs: LT_JIT_DEFINES=LT_MASK32=0,
// or -DLT_MASK32=0 at build time, keeps 64 bits everywhere)
#ifndef LT_MASK32
#define LT_MASK32 1
#endif

namespace lt {

template <bool NARROW>
struct PointBitsSel {
  typedef uint64_t type;
};
template <>
struct PointBitsSel<true> {
  typedef uint32_t type;
};

template <int MAXY>
struct PointBits {
  typedef typename PointBitsSel<(MAXY <= 32) && (LT_MASK32 != 0)>::type type;
};

}  // namespace lt

#define LT_PB_BIT(M, k) ((M)1 << (k))
#define LT_PB_TWO(M, k) ((M)2 << (k))
#define LT_PB_BELOW(M, k) (((M)1 << (k)) - 1)
#define LT_PB_ABOVE(M, k) (~(((M)2 << (k)) - 1))
#define LT_PB_CTZ(M, m) \
  (sizeof(M) == 8 ? __builtin_ctzll(m) : __builtin_ctz((uint32_t)(m)))
// index of the highest set bit (63 - clzll of a 64-bit mask)
#define LT_PB_TOP(M, m) \
  (sizeof(M) == 8 ? 63 - __builtin_clzll(m) : 31 - __builtin_clz((uint32_t)(m)))
#define LT_PB_POPC(M, m) \
  (sizeof(M) == 8 ? __builtin_popcountll(m) : __builtin_popcount((uint32_t)(m)))
#define LT_PB_DROP_LOWEST(M, m) ((M)((m) & ((m) - 1)))
