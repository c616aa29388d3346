// The point-mask helpers of land_trendr_amd/csrc/lt_bits.h against the plain 64-bit expressions
// the kernels used before the mask type had a width of its own, truncated to the width. A program
// of its own (tests/test_bits_host.py builds it with AddressSanitizer and UBSan and runs it): a
// shift by the width or more, or a signed overflow in a helper, ends it.
//
// For both widths W (32, 64) and every position k in 0..W-1:
//   LT_PB_BIT(k)    == trunc(1ull << k)
//   LT_PB_TWO(k)    == trunc(2ull << k)              (k = W-1: 0, the dropped bit)
//   LT_PB_BELOW(k)  == trunc((1ull << k) - 1)
//   LT_PB_ABOVE(k)  == trunc(~((2ull << k) - 1))     (k = W-1: 0)
//   LT_PB_CTZ, _TOP, _POPC, _DROP_LOWEST of single-bit masks, of masks with a second bit at every
//   other position, and of pseudo-random masks == ctzll, 63 - clzll, popcountll, m & (m - 1)
// and the type selection of PointBits for the instances the library builds.
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "../../land_trendr_amd/csrc/lt_bits.h"

// the helper macros at one mask type, under the names the checks below use
template <class M>
struct Helpers {
  static M bit(int k) { return LT_PB_BIT(M, k); }
  static M two(int k) { return LT_PB_TWO(M, k); }
  static M bits_below(int k) { return LT_PB_BELOW(M, k); }
  static M bits_above(int k) { return LT_PB_ABOVE(M, k); }
  static int ctz(M m) { return LT_PB_CTZ(M, m); }
  static int top(M m) { return LT_PB_TOP(M, m); }
  static int popc(M m) { return LT_PB_POPC(M, m); }
  static M drop_lowest(M m) { return LT_PB_DROP_LOWEST(M, m); }
};

static int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (failures < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                    \
    }                                                                \
  } while (0)

// (the 64-bit expressions shift by k <= 63 only; for W = 64, 2ull << 63 is 0 as in the kernels)
template <class M>
static void check_mask(M m) {
  typedef Helpers<M> B;
  const uint64_t w = (uint64_t)m;  // zero-extended: the reference sees the same set
  if (m == 0) return;
  CHECK(B::ctz(m) == __builtin_ctzll(w));
  CHECK(B::top(m) == 63 - __builtin_clzll(w));
  CHECK(B::popc(m) == __builtin_popcountll(w));
  CHECK(B::drop_lowest(m) == (M)(w & (w - 1)));
  CHECK((uint64_t)B::drop_lowest(m) == (w & (w - 1)));  // no bit appears above the width
}

template <class M>
static void check_width() {
  typedef Helpers<M> B;
  const int W = 8 * (int)sizeof(M);
  uint64_t rnd = 0x9e3779b97f4a7c15ull;
  for (int k = 0; k < W; k++) {
    CHECK(B::bit(k) == (M)(1ull << k));
    CHECK(B::two(k) == (M)(2ull << k));
    CHECK(B::bits_below(k) == (M)((1ull << k) - 1));
    CHECK(B::bits_above(k) == (M)(~((2ull << k) - 1)));
    // the way the kernels use them: the vertices of a full mask below / above vertex k
    const M full = (M)~(M)0;
    CHECK(B::popc((M)(full & B::bits_below(k))) == k);
    CHECK(B::popc((M)(full & B::bits_above(k))) == W - 1 - k);
    check_mask<M>(B::bit(k));
    CHECK(B::drop_lowest(B::bit(k)) == 0);
    CHECK(B::ctz(B::bit(k)) == k && B::top(B::bit(k)) == k && B::popc(B::bit(k)) == 1);
    for (int j = 0; j < W; j++) {
      const M m = (M)(B::bit(k) | B::bit(j));
      check_mask<M>(m);
      CHECK(B::ctz(m) == (k < j ? k : j) && B::top(m) == (k > j ? k : j));
      CHECK(((m >> k) & 1) == 1);
    }
    for (int r = 0; r < 64; r++) {
      rnd = rnd * 6364136223846793005ull + 1442695040888963407ull;
      check_mask<M>((M)(rnd >> (r & 31)));
    }
  }
  CHECK(B::bits_above(W - 1) == 0);
  CHECK(B::two(W - 1) == 0);
  CHECK(B::bits_below(0) == 0);
  CHECK(B::bit(W - 1) == (M)((M)1 << (W - 1)));
  check_mask<M>((M)~(M)0);  // T = n = W: every bit of the mask in use
  CHECK(B::popc((M)~(M)0) == W && B::top((M)~(M)0) == W - 1);
}

int main() {
  check_width<uint32_t>();
  check_width<uint64_t>();
  static_assert(std::is_same<lt::PointBits<48>::type, uint64_t>::value, "MAXY 48");
  static_assert(std::is_same<lt::PointBits<64>::type, uint64_t>::value, "MAXY 64");
  static_assert(std::is_same<lt::PointBits<33>::type, uint64_t>::value, "MAXY 33");
#if LT_MASK32
  static_assert(std::is_same<lt::PointBits<32>::type, uint32_t>::value, "MAXY 32");
#else
  static_assert(std::is_same<lt::PointBits<32>::type, uint64_t>::value, "MAXY 32, LT_MASK32=0");
#endif
  if (failures) {
    printf("%d failures\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
