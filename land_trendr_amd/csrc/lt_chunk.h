// lt_chunk.h — one strip or tile of one TIFF image, decoded into the image's band planes: the one
// per-chunk decoder, for both layouts, uncompressed, LZW or Deflate.
// Compiled for the host (g++: lt_io.cpp's lt_tiff_decode_chunks, a pool of threads) and for the
// device (hipcc: lt_chunks.hip, one lane per chunk).
//
// Layouts. Strips: a chunk is as wide as the image, chunk_h rows, the last strip of a band holds
// only the remaining rows. Tiles (tags 322-325): every tile is chunk_w x chunk_h in full, there are
// ceil(W / chunk_w) * ceil(H / chunk_h) of them per band (times the bands for planar 2), and an
// edge tile is clipped on both axes when it is copied into the raster.
// Compression 1, 5 or 8 (the caller maps 32946 to 8); predictor 1 or 2, the differencing along
// the chunk's own row, padding included, with the samples per pixel as the stride; either byte
// order; planar 1 (de-interleaved here) or 2; samples of 1, 2, 4 or 8 bytes.
// A tile, or a chunky chunk, is decoded into `tmp` (the caller's buffer of chunk_bytes() bytes)
// and copied from there; a planar-2 strip goes straight to its rows.
// A short chunk is zero-padded (compression 8: a stream that ends early but validly); a stream
// the decoder rejects, or an offset / count outside the file, returns LT_IO_ERR_DATA for this
// chunk and leaves its pixels unspecified. A chunk decodes to less than 1 MiB (the LZW core's
// limit, lt_lzw_core.h), which bounds `tmp`.
#pragma once
#include <stdint.h>

#include "lt_inflate_core.h"
#include "lt_lzw_core.h"

namespace lt_chunk {

struct Image {
  const uint8_t* file;
  int64_t file_size;
  const uint64_t* offsets;
  const uint64_t* counts;
  int32_t compression, predictor, bps, big_endian;
  int64_t width, height;
  int32_t bands, planar;
  int64_t chunk_w, chunk_h;
  int32_t tiled;
  uint8_t* out;  // [bands][height][width]
};

// the one place an Image is filled: lt_tiff_decode_chunks's arguments, lt_chunks_job's fields
LT_LZW_HD inline Image make_image(const uint8_t* file, int64_t file_size, const uint64_t* offsets,
                                  const uint64_t* counts, int compression, int predictor, int bps,
                                  int big_endian, int64_t width, int64_t height, int bands,
                                  int planar, int64_t chunk_w, int64_t chunk_h, int tiled,
                                  void* out) {
  Image I;
  I.file = file;
  I.file_size = file_size;
  I.offsets = offsets;
  I.counts = counts;
  I.compression = compression;
  I.predictor = predictor;
  I.bps = bps;
  I.big_endian = big_endian;
  I.width = width;
  I.height = height;
  I.bands = bands;
  I.planar = planar;
  I.chunk_w = chunk_w;
  I.chunk_h = chunk_h;
  I.tiled = tiled ? 1 : 0;
  I.out = (uint8_t*)out;
  return I;
}

LT_LZW_HD inline int64_t chunks_per_band(const Image& J) {
  const int64_t ty = (J.height + J.chunk_h - 1) / J.chunk_h;
  return J.tiled ? ty * ((J.width + J.chunk_w - 1) / J.chunk_w) : ty;
}

// the chunks the image itself has
LT_LZW_HD inline int64_t image_chunks(const Image& J) {
  return J.planar == 1 ? chunks_per_band(J) : chunks_per_band(J) * J.bands;
}

// decoded bytes of a full chunk, or -1 when it is not below 1 MiB
LT_LZW_HD inline int64_t chunk_bytes(const Image& J) {
  const int64_t rows = (!J.tiled && J.chunk_h > J.height) ? J.height : J.chunk_h;
  const int64_t cols = J.tiled ? J.chunk_w : J.width;
  const int spp = J.planar == 1 ? J.bands : 1;
  const double sz = (double)rows * (double)cols * (double)spp * (double)J.bps;
  if (sz >= (double)lt_lzw::kCoreMaxOut) return -1;
  return rows * cols * spp * J.bps;
}

// whether the image's chunks are decoded through `tmp` (else straight into the planes)
LT_LZW_HD inline bool staged(const Image& J) {
  return J.tiled || (J.planar == 1 && J.bands > 1);
}

// what lt_tiff_decode_chunks and lt_tiff_decode_chunks_dev reject before decoding anything
LT_LZW_HD inline bool bad_image(const Image& J, int64_t n_chunks) {
  if (!J.file || !J.offsets || !J.counts || !J.out || J.file_size < 0 || J.width <= 0 ||
      J.height <= 0 || J.bands <= 0 || J.chunk_w <= 0 || J.chunk_h <= 0 ||
      !(J.bps == 1 || J.bps == 2 || J.bps == 4 || J.bps == 8))
    return true;
  if (J.compression != 1 && J.compression != 5 && J.compression != 8) return true;
  if (J.predictor != 1 && J.predictor != 2) return true;
  if (J.planar != 1 && J.planar != 2) return true;
  if (!J.tiled && J.chunk_w != J.width) return true;
  // (the chunk counts as doubles first: they must not overflow)
  const double per = ((double)J.height / (double)J.chunk_h + 1.0) *
                     (J.tiled ? (double)J.width / (double)J.chunk_w + 1.0 : 1.0) * (double)J.bands;
  if (per >= 9e18) return true;
  if (n_chunks < image_chunks(J)) return true;
  return chunk_bytes(J) < 0;
}

template <class T>
LT_LZW_HD inline void undo_pred2(uint8_t* buf, int64_t rows, int64_t width, int spp) {
  T* a = (T*)buf;
  for (int64_t y = 0; y < rows; y++) {
    T* r = a + y * width * spp;
    for (int64_t x = spp; x < width * spp; x++) r[x] = (T)(r[x] + r[x - spp]);
  }
}

// Chunk k of image J. Returns 0 or the decoder's negative LT_IO_ERR_*. kInflate false: compiled
// without the Deflate core (its frame and Huffman tables cost the device every lane's registers,
// scratch and LDS), for callers that hold no compression 8 image; one met all the same fails.
template <bool kInflate = true, class LzwTable, class InfTable>
LT_LZW_HD inline int decode_chunk(const Image& J, int64_t k, const LzwTable lzw,
                                  const InfTable inf, uint8_t* tmp) {
  const int bps = J.bps;
  const int spp = J.planar == 1 ? J.bands : 1;
  const int64_t per_band = chunks_per_band(J);
  const int64_t b = J.planar == 1 ? 0 : k / per_band, r = J.planar == 1 ? k : k % per_band;
  if (b >= J.bands || r >= per_band) return 0;  // chunks past the image: ignored
  const int64_t tx = J.tiled ? (J.width + J.chunk_w - 1) / J.chunk_w : 1;
  const int64_t y0 = (r / tx) * J.chunk_h, x0 = (r % tx) * J.chunk_w;
  const int64_t left_h = J.height - y0, left_w = J.width - x0;
  const int64_t rows_in = J.chunk_h < left_h ? J.chunk_h : left_h;  // rows that reach the raster
  const int64_t cols_in = J.chunk_w < left_w ? J.chunk_w : left_w;
  const int64_t rows = J.tiled ? J.chunk_h : rows_in;  // rows the chunk holds
  const int64_t cols = J.chunk_w;
  const int64_t size = rows * cols * spp * bps;
  const int64_t plane = J.width * J.height * bps;
  const uint64_t off = J.offsets[k], cnt = J.counts[k];
  if (off > (uint64_t)J.file_size || cnt > (uint64_t)J.file_size - off) return lt_lzw::kErrData;
  const uint8_t* src = J.file + off;
  const bool direct = !staged(J);  // a planar-2 strip: straight into the band's rows
  uint8_t* dst = direct ? J.out + b * plane + y0 * J.width * bps : tmp;
  int64_t n;
  if (J.compression == 5) {
    n = lt_lzw::decode(src, (int64_t)cnt, dst, size, lzw);
  } else if (J.compression == 8) {
    if constexpr (kInflate) n = lt_inflate::decode(src, (int64_t)cnt, dst, size, inf);
    else return lt_lzw::kErrData;
  } else {
    n = size < (int64_t)cnt ? size : (int64_t)cnt;
    for (int64_t i = 0; i < n; i++) dst[i] = src[i];
  }
  if (n < 0) return (int)n;
  for (int64_t i = n; i < size; i++) dst[i] = 0;  // a short chunk: zero-padded (libtiff)
  const int64_t samples = rows * cols * spp;
  if (J.big_endian && bps > 1) {
    for (int64_t i = 0; i < samples; i++) {
      uint8_t* p = dst + i * bps;
      for (int a = 0; a < bps / 2; a++) {
        const uint8_t t = p[a];
        p[a] = p[bps - 1 - a];
        p[bps - 1 - a] = t;
      }
    }
  }
  if (J.predictor == 2) {
    switch (bps) {
      case 1: undo_pred2<uint8_t>(dst, rows, cols, spp); break;
      case 2: undo_pred2<uint16_t>(dst, rows, cols, spp); break;
      case 4: undo_pred2<uint32_t>(dst, rows, cols, spp); break;
      default: undo_pred2<uint64_t>(dst, rows, cols, spp); break;
    }
  }
  if (!direct) {  // the part of the chunk inside the raster, sample by sample into the planes
    for (int bb = 0; bb < spp; bb++) {
      uint8_t* o = J.out + (b + bb) * plane + (y0 * J.width + x0) * bps;
      const uint8_t* i = dst + bb * bps;
      for (int64_t y = 0; y < rows_in; y++)
        for (int64_t x = 0; x < cols_in; x++)
          for (int a = 0; a < bps; a++)
            o[(y * J.width + x) * bps + a] = i[(y * cols + x) * spp * bps + a];
    }
  }
  return 0;
}

}  // namespace lt_chunk
