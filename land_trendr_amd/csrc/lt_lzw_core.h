// lt_lzw_core.h — one TIFF LZW strip decoder, compiled for the host (g++: lt_io.cpp's
// lt_lzw_decode_core) and for the device (hipcc: lt_decode.hip, one lane per strip).
//
// The stream rules are those at the top of lt_io.cpp: codes MSB first, 9 to 12 bits wide, Clear 256,
// EOI 257, first free code 258, libtiff's early change, a strip may end without EOI, data starts
// with a Clear or a literal, KwKwK only for code == free_ent < 4096. Same contract as lt_lzw_decode:
// the bytes written, or LT_IO_ERR_DATA / LT_IO_ERR_SPACE, never a write at or past out + cap — and,
// unlike lt_lzw_decode's 16-byte copies, never a write past the returned count either.
//
// Table: as in lt_lzw_decode an entry is (position in this strip's output, length) and a new entry
// is (the previous emission's start, its length + 1): no chain walk. One 32-bit word, position in
// the upper 20 bits, length in the lower 12 (fewer than 3838 entries exist between two Clears, so a
// length stays below 4096); a strip therefore decodes to less than 1 MiB (kLzwCoreMaxOut). The
// caller owns the table and hands it in through an accessor with get(code) / set(code, word) for
// codes 258..4095, so the device lays it out its own way. Entries below free_ent were all written
// since the strip's last Clear (or its start): nothing is read that this call did not write.
//
// Every loop is bounded by the arguments alone: the code loop takes at least 9 input bits per
// turn, the refill at most two bytes, a copy at most min(len, cap - n_out) bytes; len and
// pos + len <= n_out are checked before a copy, whatever the table holds.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LT_LZW_HD __host__ __device__
#else
#define LT_LZW_HD
#endif

namespace lt_lzw {

constexpr int64_t kCoreMaxOut = (int64_t)1 << 20;  // decoded strip size: below this
constexpr int kErrArg = -1, kErrData = -2, kErrSpace = -3;  // LT_IO_ERR_* (include/lt_io.h)

// the host's table: 4096 words in a row
struct FlatTable {
  uint32_t* t;
  LT_LZW_HD uint32_t get(int code) const { return t[code]; }
  LT_LZW_HD void set(int code, uint32_t w) const { t[code] = w; }
};

// entry-major with a stride: entry e of this decoder at t[e * stride] (the device: stride 64, the
// 64 lanes of a wave side by side, so the one entry every lane adds per code is one coalesced store)
struct StridedTable {
  uint32_t* t;
  int64_t stride;
  LT_LZW_HD uint32_t get(int code) const { return t[(int64_t)code * stride]; }
  LT_LZW_HD void set(int code, uint32_t w) const { t[(int64_t)code * stride] = w; }
};

// out[dst .. dst + len) = out[src .. src + len), src + len <= dst (a string of earlier output: no
// overlap). Byte by byte: staging eight bytes in registers between the loads and the stores was
// not faster on the device for a stack of near-random rasters, whose strings are 1-2 bytes.
LT_LZW_HD inline void copy_earlier(uint8_t* out, int64_t dst, int64_t src, int len) {
  for (int k = 0; k < len; k++) out[dst + k] = out[src + k];
}

template <class Table>
LT_LZW_HD inline int64_t decode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap,
                                const Table tab) {
  constexpr int kClear = 256, kEoi = 257, kFirst = 258, kMaxBits = 12;
  if (!in || n_in < 0 || cap < 0 || (cap > 0 && !out) || cap >= kCoreMaxOut) return kErrArg;
  int nbits = 9, free_ent = kFirst, grow_at = (1 << 9) - 1;
  int64_t n_out = 0, ip = 0;
  uint32_t acc = 0;  // the pending input bits, the oldest most significant (at most 7 + 16)
  int nacc = 0;
  uint32_t old_pos = 0;  // the previous code's emission
  int old_len = 0;
  bool have_old = false, after_clear = false;
  for (;;) {
    while (nacc < nbits && ip < n_in) {  // at most two bytes
      acc = ((acc << 8) | in[ip++]) & 0xffffffu;
      nacc += 8;
    }
    if (nacc < nbits) break;  // the input cannot fill a whole code: the strip's end
    nacc -= nbits;
    const int code = (int)((acc >> nacc) & ((1u << nbits) - 1u));
    if (code == kEoi) break;
    if (code == kClear && !after_clear) {
      nbits = 9;
      grow_at = (1 << 9) - 1;
      free_ent = kFirst;
      after_clear = true;
      continue;
    }
    if (after_clear || !have_old) {  // the first code of a table: a literal
      if (code >= 256) return kErrData;
      if (n_out >= cap) return kErrSpace;
      out[n_out] = (uint8_t)code;
      old_pos = (uint32_t)n_out++;
      old_len = 1;
      have_old = true;
      after_clear = false;
      continue;
    }
    int L;
    if (code < 256) {
      L = 1;
      if (n_out + L > cap) return kErrSpace;
      out[n_out] = (uint8_t)code;
    } else if (code < free_ent) {  // a table string: L bytes of earlier output
      const uint32_t e = tab.get(code);
      const int64_t pos = (int64_t)(e >> 12);
      L = (int)(e & 0xfffu);
      if (n_out + L > cap) return kErrSpace;
      if (L == 0 || pos + L > n_out) return kErrData;  // (never with a table this call wrote)
      copy_earlier(out, n_out, pos, L);
    } else if (code == free_ent && free_ent < 4096) {
      // KwKwK: the previous string + its own first byte
      L = old_len + 1;
      if (n_out + L > cap) return kErrSpace;
      if ((int64_t)old_pos + old_len > n_out) return kErrData;  // (never: it was emitted)
      copy_earlier(out, n_out, (int64_t)old_pos, old_len);
      out[n_out + old_len] = out[old_pos];
    } else {
      return kErrData;
    }
    if (free_ent < 4096) {  // previous string + this one's first byte: contiguous in out
      tab.set(free_ent, (old_pos << 12) | (uint32_t)(old_len + 1));
      free_ent++;
    }
    old_pos = (uint32_t)n_out;
    old_len = L;
    n_out += L;
    if (free_ent >= grow_at && nbits < kMaxBits) {
      nbits++;
      grow_at = (1 << nbits) - 1;
    }
  }
  return n_out;
}

}  // namespace lt_lzw
