// lt_lzw_core.h — one TIFF LZW strip decoder and one encoder (below it), compiled for the host
// (g++: lt_io.cpp's lt_lzw_decode_core / lt_lzw_encode_core) and for the device (hipcc:
// lt_chunks.hip and lt_encode.hip, one lane per strip).
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

// ---- the encoder ---------------------------------------------------------------------------------
// lt_lzw_encode's code stream (lt_io.cpp), byte for byte: Clear first, 9..12-bit codes MSB first,
// libtiff's early change, a Clear when free_ent reaches 4094, after the final code a Clear when the
// table just filled or else the width step, then EOI; n_in == 0 gives Clear, EOI. Greedy LZW under
// these rules is deterministic, so only the dictionary differs from the host's 4096 x 256 direct
// table: open addressing (linear probing) over kEncSlots 32-bit words, one word per string:
// prefix code (12 bits) | byte (8 bits) | code (12 bits). A code is at least 258, so 0 is an empty
// slot. At most 3836 strings exist between two Clears (codes 258..4093): the load stays at or below
// 3836 / 8192 and an empty slot always ends a probe sequence. The caller owns the table and hands
// it in through an accessor with get(slot) / set(slot, word) for slots 0..kEncSlots-1 (FlatTable,
// StridedTable); it is zeroed here at the start and at each Clear, slot by slot in order, which on
// the device is one coalesced store per slot for the lanes of a wave.
//
// The input is read through a byte source, byte(k) for k in [0, n_in), so the device applies
// predictor 2 on the fly (never to the raster). Every loop is bounded by the arguments alone: the
// byte loop by n_in, a probe sequence by kEncSlots with an explicit counter, the zeroing by
// kEncSlots, the bit writer by cap. Never a write at or past out + cap. Returns the byte count, or
// kErrArg / kErrSpace (cap too small: out's contents are then unspecified).
constexpr int kEncSlots = 8192;  // per encoder: 32 KB

struct PlainBytes {
  const uint8_t* p;
  LT_LZW_HD uint8_t byte(int64_t k) const { return p[k]; }
};

// the pending bits, the oldest most significant; whole bytes leave as soon as they are complete
struct EncBits {
  uint8_t* out;
  int64_t cap, n;
  uint32_t acc;
  int nacc;  // below 8 between two puts
  LT_LZW_HD bool put(int code, int nbits) {  // false: out of space
    acc = (acc << nbits) | (uint32_t)code;  // at most 7 + 12 bits
    nacc += nbits;
    while (nacc >= 8) {  // at most two bytes
      if (n >= cap) return false;
      nacc -= 8;
      out[n++] = (uint8_t)(acc >> nacc);
    }
    acc &= (1u << nacc) - 1u;
    return true;
  }
  LT_LZW_HD bool flush() {
    if (nacc > 0) {
      if (n >= cap) return false;
      out[n++] = (uint8_t)(acc << (8 - nacc));
    }
    nacc = 0;
    acc = 0;
    return true;
  }
};

template <class Table>
LT_LZW_HD inline void enc_zero(const Table tab) {
  for (int s = 0; s < kEncSlots; s++) tab.set(s, 0u);
}

template <class Src, class Table>
LT_LZW_HD inline int64_t encode_from(const Src src, int64_t n_in, uint8_t* out, int64_t cap,
                                     const Table tab) {
  constexpr int kClear = 256, kEoi = 257, kFirst = 258, kMaxBits = 12;
  if (n_in < 0 || cap < 0 || (cap > 0 && !out)) return kErrArg;
  EncBits w{out, cap, 0, 0u, 0};
  int nbits = 9, free_ent = kFirst;
  if (!w.put(kClear, nbits)) return kErrSpace;
  if (n_in == 0) {
    if (!w.put(kEoi, nbits) || !w.flush()) return kErrSpace;
    return w.n;
  }
  enc_zero(tab);
  int ent = src.byte(0);
  for (int64_t k = 1; k < n_in; k++) {
    const int c = src.byte(k);
    const uint32_t key = ((uint32_t)ent << 8) | (uint32_t)c;  // 20 bits
    uint32_t h = (key * 2654435761u) >> 19;                   // 13 bits
    int found = -1;
    int probes = 0;
    for (; probes < kEncSlots; probes++) {
      const uint32_t e = tab.get((int)h);
      if (e == 0u) break;
      if ((e >> 12) == key) {
        found = (int)(e & 0xfffu);
        break;
      }
      h = (h + 1u) & (uint32_t)(kEncSlots - 1);
    }
    if (found >= 0) {  // the string ent + c is in the table
      ent = found;
      continue;
    }
    if (probes == kEncSlots) return kErrArg;  // (never: the table is at most 3836 / 8192 full)
    if (!w.put(ent, nbits)) return kErrSpace;
    tab.set((int)h, (key << 12) | (uint32_t)free_ent);  // ent + c gets the next code
    free_ent++;
    ent = c;
    if (free_ent == (1 << kMaxBits) - 2) {  // table full (4094 codes): Clear, restart at 9 bits
      if (!w.put(kClear, nbits)) return kErrSpace;
      nbits = 9;
      free_ent = kFirst;
      enc_zero(tab);
    } else if (free_ent > (1 << nbits) - 1) {
      nbits++;
    }
  }
  if (!w.put(ent, nbits)) return kErrSpace;
  free_ent++;
  if (free_ent == (1 << kMaxBits) - 2) {
    if (!w.put(kClear, nbits)) return kErrSpace;
    nbits = 9;
  } else if (free_ent > (1 << nbits) - 1) {
    nbits++;
  }
  if (!w.put(kEoi, nbits) || !w.flush()) return kErrSpace;
  return w.n;
}

template <class Table>
LT_LZW_HD inline int64_t encode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap,
                                const Table tab) {
  if (!in) return kErrArg;
  return encode_from(PlainBytes{in}, n_in, out, cap, tab);
}

}  // namespace lt_lzw
