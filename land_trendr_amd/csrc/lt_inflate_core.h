// lt_inflate_core.h — one zlib / Deflate decoder (RFC 1950 wrapper, RFC 1951 blocks), compiled for
// the host (g++: lt_io.cpp's lt_inflate_core) and for the device (hipcc: lt_chunks.hip, one lane
// per strip or tile). TIFF Compression 8 and the old 32946.
//
// Contract (zlib's, read lazily): decode until the final block ends, then check the Adler-32
// trailer; bytes behind the trailer are ignored. The stream is followed as zlib's inflate()
// follows it when offered room for cap + 1 bytes, which is how a caller of zlib tells a stream of
// cap bytes from a longer one: byte cap is decoded but never stored, and a symbol that needs space
// past it ends the call with success and returns cap (a match that straddles cap is copied up to
// cap), as inflate() stops at the first symbol it has no room for and reports nothing that lies
// behind it. A stream of at most cap + 1 bytes is therefore checked to its end, trailer included.
// Everything zlib rejects before that point gives kErrData: a bad header (CM != 8,
// CINFO > 7, FCHECK, FDICT), BTYPE 3, LEN != ~NLEN, HLIT > 286, HDIST > 30, an over-subscribed or
// incomplete code-length code, a repeat without a previous length or past HLIT + HDIST, no code
// for symbol 256, an over-subscribed set, an incomplete set whose longest code is not 1 bit (an
// all-zero distance set is legal), literal/length symbols 286 / 287, distance symbols 30 / 31, a
// code the set does not contain, a distance before the start of this call's output, input that
// ends before the final block does or inside the trailer (while the room is not full), a wrong
// Adler-32.
// Never a write at or past out + cap, never one past the returned count; never a read at or past
// in + n_in (the bit reader pads a peek with zeros; consuming a bit it did not have is the
// truncation error). The window is this call's own earlier output: distances up to 32768,
// lengths up to 258, overlapping copies byte by byte.
//
// Tables: canonical Huffman decoding from per-length counts and a symbol list, 16-bit entries:
// count[16] + symbol[288] for literals / lengths, count[16] + symbol[30] for distances, kEntries
// in all (700 bytes). The caller owns them and hands them in through an accessor with get(i) /
// set(i, v), so the device lays them out its own way (LDS, the lanes of a wave side by side).
// Nothing is read that this call did not write. The code lengths of a block header (at most 320
// bytes) and the code-length code live in the function's own frame.
//
// Every loop is bounded by the arguments alone: a symbol consumes at least one input bit, a block
// at least three, a copy is at most min(len, cap + 1 - n_out) bytes, a table build runs over at most
// 320 lengths and 15 bit counts, the Adler-32 over the bytes written.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LT_INF_HD __host__ __device__
#else
#define LT_INF_HD
#endif

namespace lt_inflate {

constexpr int kErrArg = -1, kErrData = -2;  // LT_IO_ERR_* (include/lt_io.h)
constexpr int kBadCode = -1, kShortInput = -2;  // symbol()
constexpr int kLitCount = 0, kLitSym = 16, kDistCount = 304, kDistSym = 320, kEntries = 350;

// the host's tables: kEntries 16-bit words in a row
struct FlatTable {
  uint16_t* t;
  LT_INF_HD int get(int i) const { return t[i]; }
  LT_INF_HD void set(int i, int v) const { t[i] = (uint16_t)v; }
};

// entry-major with a stride: entry i of this decoder at t[i * stride] (the device: stride 64)
struct StridedTable {
  uint16_t* t;
  int stride;
  LT_INF_HD int get(int i) const { return t[i * stride]; }
  LT_INF_HD void set(int i, int v) const { t[i * stride] = (uint16_t)v; }
};

// the input bits, LSB first; acc holds nacc <= 32 pending bits, the oldest least significant
struct Bits {
  const uint8_t* in;
  int64_t n_in, ip;
  uint32_t acc;
  int nacc;
  // at least n <= 24 bits pending, unless the input ends first (the missing ones read as zero)
  LT_INF_HD void need(int n) {
    while (nacc < n && ip < n_in) {  // at most three bytes
      acc |= (uint32_t)in[ip++] << nacc;
      nacc += 8;
    }
  }
  // n <= 16 bits, or -1 when the input does not hold them
  LT_INF_HD int get(int n) {
    need(n);
    if (nacc < n) return -1;
    const int v = (int)(acc & ((1u << n) - 1u));
    acc >>= n;
    nacc -= n;
    return v;
  }
};

// Canonical code of `n` symbols with the lengths lens[0..n) (0: unused, at most 15): counts at
// tab[cbase + len], the symbols in code order at tab[sbase ..]. Returns what zlib's inflate_table
// looks at: *left < 0 over-subscribed, > 0 incomplete; *max the longest length (0: no code).
template <class Table>
LT_INF_HD inline void build(const Table tab, int cbase, int sbase, const uint8_t* lens, int n,
                            int* left_out, int* max_out) {
  for (int len = 0; len < 16; len++) tab.set(cbase + len, 0);
  for (int i = 0; i < n; i++) tab.set(cbase + (lens[i] & 15), tab.get(cbase + (lens[i] & 15)) + 1);
  uint16_t offs[16];
  int left = 1, max = 0;
  offs[0] = 0;
  offs[1] = 0;
  for (int len = 1; len < 16; len++) {
    const int c = tab.get(cbase + len);
    if (c) max = len;
    if (left >= 0) {  // (stays negative once over-subscribed)
      left <<= 1;
      left -= c;
    }
    if (len < 15) offs[len + 1] = (uint16_t)(offs[len] + c);
  }
  *left_out = left;
  *max_out = max;
  if (left < 0) return;  // never decoded from
  for (int i = 0; i < n; i++) {
    const int len = lens[i] & 15;
    if (len) tab.set(sbase + offs[len]++, i);
  }
}

// One symbol of the code at (cbase, sbase): kBadCode for a code the set does not contain,
// kShortInput for input that ends inside the code. At most 15 bits, peeked once; only the code's
// own bits are consumed. (A set with a missing code is the fixed distance set, a set whose only
// code has one bit, or an empty one: zlib knows a missing code by the set's longest length.)
template <class Table>
LT_INF_HD inline int symbol(Bits& b, const Table tab, int cbase, int sbase) {
  b.need(15);
  uint32_t v = b.acc;
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= 15; len++) {
    code |= (int)(v & 1u);
    v >>= 1;
    const int count = tab.get(cbase + len);
    if (code - count < first) {
      if (len > b.nacc) return kShortInput;  // the code's last bits lie behind the input's end
      b.acc >>= len;
      b.nacc -= len;
      return tab.get(sbase + index + (code - first));
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  int max = 1;
  for (int len = 2; len <= 15; len++)
    if (tab.get(cbase + len)) max = len;
  return b.nacc < max ? kShortInput : kBadCode;
}

// of p[0 .. n), then of `extra` when has_extra
LT_INF_HD inline uint32_t adler32(const uint8_t* p, int64_t n, bool has_extra, uint8_t extra) {
  uint32_t a = 1, b = 0;
  while (n > 0) {
    const int64_t m = n < 5552 ? n : 5552;  // sums stay below 2^32 for this many bytes
    for (int64_t i = 0; i < m; i++) {
      a += p[i];
      b += a;
    }
    a %= 65521u;
    b %= 65521u;
    p += m;
    n -= m;
  }
  if (has_extra) {
    a = (a + extra) % 65521u;
    b = (b + a) % 65521u;
  }
  return (b << 16) | a;
}

template <class Table>
LT_INF_HD inline int64_t decode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap,
                                const Table tab) {
  if (!in || n_in < 0 || cap < 0 || (cap > 0 && !out)) return kErrArg;
  Bits b{in, n_in, 0, 0u, 0};
  const int cmf = b.get(8), flg = b.get(8);
  if (cmf < 0 || flg < 0) return kErrData;
  if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20))
    return kErrData;
  const int64_t room = cap + 1;  // byte cap is decoded into `last`, not stored
// the input ended: the truncation error, unless the room is full (inflate() then waits for input
// and reports nothing: the caller has its cap + 1 bytes)
#define LT_INF_SHORT return n_out >= room ? cap : (int64_t)kErrData
  uint8_t last = 0;
  int64_t n_out = 0;
  bool fixed_built = false;
  for (;;) {  // a block: at least three bits
    const int hdr = b.get(3);
    if (hdr < 0) LT_INF_SHORT;
    const int type = hdr >> 1;
    if (type == 0) {  // stored: to the byte boundary, LEN, ~LEN, the bytes
      b.get(b.nacc & 7);
      const int len = b.get(16), nlen = b.get(16);
      if (len < 0 || nlen < 0) LT_INF_SHORT;
      if (len != (nlen ^ 0xffff)) return kErrData;
      b.ip -= b.nacc >> 3;  // whole pending bytes go back: the copy reads the input directly
      b.acc = 0;
      b.nacc = 0;
      int64_t m = len;
      if (m > n_in - b.ip) m = n_in - b.ip;
      if (m > room - n_out) m = room - n_out;
      for (int64_t i = 0; i < m; i++) {
        if (n_out + i < cap) out[n_out + i] = in[b.ip + i];
        else last = in[b.ip + i];
      }
      n_out += m;
      b.ip += m;
      if (m < len) {
        LT_INF_SHORT;  // no room for the next byte, or the input ended inside the block
      }
    } else if (type == 3) {
      return kErrData;
    } else {
      if (type == 1) {
        if (!fixed_built) {
          uint8_t lens[288];
          int left, max;
          for (int i = 0; i < 288; i++) lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
          build(tab, kLitCount, kLitSym, lens, 288, &left, &max);
          for (int i = 0; i < 30; i++) lens[i] = 5;  // (codes 30 and 31: not in the set)
          build(tab, kDistCount, kDistSym, lens, 30, &left, &max);
          fixed_built = true;
        }
      } else {
        fixed_built = false;
        const int hlit = b.get(5), hdist = b.get(5), hclen = b.get(4);
        if (hlit < 0 || hdist < 0 || hclen < 0) LT_INF_SHORT;
        const int nlen = hlit + 257, ndist = hdist + 1, ncode = hclen + 4;
        if (nlen > 286 || ndist > 30) return kErrData;
        uint8_t lens[320];
        uint16_t cl[16 + 19];  // the code-length code: counts, symbols
        const FlatTable clt{cl};
        {
          // (the order of RFC 1951 3.2.7, packed: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15)
          const uint64_t lo = 0x8796a5b4c3d2e1full;  // the last 15 entries, 4 bits each
          for (int i = 0; i < 19; i++) lens[i] = 0;
          for (int i = 0; i < ncode; i++) {
            const int v = b.get(3);
            if (v < 0) LT_INF_SHORT;
            const int s = i < 3 ? 16 + i : i == 3 ? 0 : (int)((lo >> (4 * (18 - i))) & 15u);
            lens[s] = (uint8_t)v;
          }
          int left, max;
          build(clt, 0, 16, lens, 19, &left, &max);
          // (no code at all: zlib reads every length as zero, then misses symbol 256)
          if (max == 0 || left != 0) return kErrData;
        }
        int idx = 0;
        while (idx < nlen + ndist) {  // at least one bit a turn
          const int s = symbol(b, clt, 0, 16);
          if (s == kShortInput) LT_INF_SHORT;
          if (s < 0) return kErrData;
          if (s < 16) {
            lens[idx++] = (uint8_t)s;
            continue;
          }
          int rep, val = 0;
          if (s == 16) {
            if (idx == 0) return kErrData;
            val = lens[idx - 1];
            rep = b.get(2);
            if (rep < 0) LT_INF_SHORT;
            rep += 3;
          } else if (s == 17) {
            rep = b.get(3);
            if (rep < 0) LT_INF_SHORT;
            rep += 3;
          } else {
            rep = b.get(7);
            if (rep < 0) LT_INF_SHORT;
            rep += 11;
          }
          if (idx + rep > nlen + ndist) return kErrData;
          for (int i = 0; i < rep; i++) lens[idx++] = (uint8_t)val;
        }
        if (lens[256] == 0) return kErrData;
        int left, max;
        build(tab, kLitCount, kLitSym, lens, nlen, &left, &max);
        if (left < 0 || (left > 0 && max != 1)) return kErrData;
        build(tab, kDistCount, kDistSym, lens + nlen, ndist, &left, &max);
        if (left < 0 || (left > 0 && max > 1)) return kErrData;
      }
      for (;;) {  // a symbol: at least one bit
        const int s = symbol(b, tab, kLitCount, kLitSym);
        if (s == kShortInput) LT_INF_SHORT;
        if (s < 0) return kErrData;
        if (s < 256) {
          if (n_out >= room) return cap;
          if (n_out < cap) out[n_out] = (uint8_t)s;
          else last = (uint8_t)s;
          n_out++;
          continue;
        }
        if (s == 256) break;
        if (s > 285) return kErrData;
        int len;
        if (s < 265) {
          len = s - 254;
        } else if (s == 285) {
          len = 258;
        } else {
          const int e = (s - 261) >> 2, x = b.get(e);
          if (x < 0) LT_INF_SHORT;
          len = 3 + ((4 + ((s - 261) & 3)) << e) + x;
        }
        const int d = symbol(b, tab, kDistCount, kDistSym);
        if (d == kShortInput) LT_INF_SHORT;
        if (d < 0 || d > 29) return kErrData;
        int64_t dist;
        if (d < 4) {
          dist = 1 + d;
        } else {
          const int e = (d - 2) >> 1, x = b.get(e);
          if (x < 0) LT_INF_SHORT;
          dist = 1 + ((int64_t)(2 + (d & 1)) << e) + x;
        }
        if (n_out >= room) return cap;
        if (dist > n_out) return kErrData;
        int64_t m = len;
        if (m > room - n_out) m = room - n_out;
        for (int64_t i = 0; i < m; i++) {  // (the source lies below the destination: below cap)
          if (n_out + i < cap) out[n_out + i] = out[n_out + i - dist];
          else last = out[n_out + i - dist];
        }
        n_out += m;
        if (m < len) return cap;
      }
    }
    if (hdr & 1) break;
  }
  b.get(b.nacc & 7);
  uint32_t want = 0;
  for (int i = 0; i < 4; i++) {
    const int v = b.get(8);
    if (v < 0) LT_INF_SHORT;
    want = (want << 8) | (uint32_t)v;
  }
  if (want != adler32(out, n_out < cap ? n_out : cap, n_out > cap, last)) return kErrData;
  return n_out < cap ? n_out : cap;
#undef LT_INF_SHORT
}

}  // namespace lt_inflate
