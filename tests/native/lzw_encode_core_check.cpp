// lzw_encode_core_check.cpp — the LZW encoder and decoder cores (land_trendr_amd/csrc/
// lt_lzw_core.h) as a stand-alone host program, meant to be compiled with
// -fsanitize=address,undefined (tests/test_lzw_encode_core_host.py): seeded inputs of several
// kinds and lengths are encoded into heap buffers of exactly `cap` bytes (so a write at or past
// out + cap is a heap overflow the sanitizer reports) at the worst-case cap, at every cap below
// the exact size for the short inputs and at a spread of short caps for the long ones, and every
// full encode is decoded back by the decoder core. Prints "ok <cases>" and exits 0, or names the
// first failing case and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../land_trendr_amd/csrc/lt_lzw_core.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

std::vector<uint8_t> make(int kind, int64_t n) {
  std::vector<uint8_t> v((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    switch (kind) {
      case 0: v[(size_t)i] = (uint8_t)rnd(); break;         // random: the table fills, Clears
      case 1: v[(size_t)i] = 0; break;                      // zeros: long strings
      case 2: v[(size_t)i] = (uint8_t)(i % 3 + 1); break;   // period 3
      case 3: v[(size_t)i] = (uint8_t)(rnd() & 3u); break;  // low entropy
      default: v[(size_t)i] = (uint8_t)i; break;            // ramp
    }
  }
  return v;
}

int64_t enc(const std::vector<uint8_t>& in, int64_t cap, std::vector<uint8_t>* keep) {
  std::vector<uint32_t> table((size_t)lt_lzw::kEncSlots, 0xdeadbeefu);  // (zeroed by the core)
  uint8_t* out = cap > 0 ? new uint8_t[(size_t)cap] : nullptr;  // exactly cap bytes
  static const uint8_t none = 0;
  const int64_t m = lt_lzw::encode(in.empty() ? &none : in.data(), (int64_t)in.size(), out, cap,
                                   lt_lzw::FlatTable{table.data()});
  if (keep && m >= 0) keep->assign(out, out + m);
  delete[] out;
  return m;
}

}  // namespace

int main() {
  const int64_t lens[] = {0, 1, 2, 3, 255, 256, 771, 1812, 3941, 5000, 9000, 70000};
  long cases = 0;
  for (int kind = 0; kind < 5; kind++) {
    for (int64_t n : lens) {
      const std::vector<uint8_t> in = make(kind, n);
      std::vector<uint8_t> full;
      const int64_t m = enc(in, n * 3 / 2 + 16, &full);
      if (m <= 0) {
        printf("kind %d n %lld: encode gave %lld\n", kind, (long long)n, (long long)m);
        return 1;
      }
      cases++;
      // back through the decoder core (exactly n bytes of output space)
      std::vector<uint32_t> dtab(4096, 0);
      uint8_t* back = new uint8_t[(size_t)(n > 0 ? n : 1)];
      const int64_t d = lt_lzw::decode(full.data(), m, back, n, lt_lzw::FlatTable{dtab.data()});
      const bool same = d == n && (n == 0 || memcmp(back, in.data(), (size_t)n) == 0);
      delete[] back;
      if (!same) {
        printf("kind %d n %lld: round trip gave %lld\n", kind, (long long)n, (long long)d);
        return 1;
      }
      // the exact size fits; every shorter cap is LT_IO_ERR_SPACE (all of them for the short
      // inputs, a spread for the long ones)
      std::vector<uint8_t> again;
      if (enc(in, m, &again) != m || again != full) {
        printf("kind %d n %lld: the exact cap failed\n", kind, (long long)n);
        return 1;
      }
      const int64_t step = m <= 1500 ? 1 : m / 97;
      for (int64_t cap = 0; cap < m; cap += step) {
        const int64_t r = enc(in, cap, nullptr);
        cases++;
        if (r != lt_lzw::kErrSpace) {
          printf("kind %d n %lld cap %lld: %lld, not LT_IO_ERR_SPACE\n", kind, (long long)n,
                 (long long)cap, (long long)r);
          return 1;
        }
      }
      if (enc(in, m - 1, nullptr) != lt_lzw::kErrSpace) {
        printf("kind %d n %lld: cap = size - 1 was accepted\n", kind, (long long)n);
        return 1;
      }
    }
  }
  printf("ok %ld\n", cases);
  return 0;
}
