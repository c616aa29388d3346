/*
 * lt_io.h — host codecs of the raster IO around the hot path (land_trendr_amd/liblt_io.so).
 *
 * The reference reads and writes GeoTIFFs through GDAL: ds2array (/root/reference/utils.py:
 * 272-282) decodes whatever compression the input rasters carry, array2raster (utils.py:374-412)
 * writes every output raster with COMPRESS=LZW (utils.py:386). GDAL is absent here; these are the
 * LZW halves of that (Deflate goes through zlib). Plain pointers and sizes; the caller owns both
 * buffers. Return: bytes written (>= 0) or a negative LT_IO_ERR_*.
 */
#ifndef LT_IO_H
#define LT_IO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { LT_IO_ERR_ARG = -1, LT_IO_ERR_DATA = -2, LT_IO_ERR_SPACE = -3 };

/* One TIFF LZW strip or tile (Compression = 5) -> its raw bytes (at most cap; bytes of out past
 * the returned count may be overwritten, never past cap). */
int64_t lt_lzw_decode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);
/* Raw bytes -> one TIFF LZW strip (libtiff's code stream: Clear first, 9..12-bit codes, early
 * change, Clear when the table is full). cap >= n_in * 3 / 2 + 16 always suffices. */
int64_t lt_lzw_encode(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);
/* lt_lzw_decode's contract by the decoder core the device runs (land_trendr_amd/csrc/
 * lt_lzw_core.h, one lane per strip in lt_tiff_decode_strips_dev), compiled for the host: same
 * counts, bytes and errors; LT_IO_ERR_ARG for cap >= 1 MiB (its table packs 20-bit positions);
 * no byte of out past the returned count is written. */
int64_t lt_lzw_decode_core(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);
/* lt_lzw_encode's contract by the encoder core the device runs (lt_lzw_core.h, one lane per strip
 * in lt_tiff_encode_strips_dev), compiled for the host: the same bytes for every input; no byte
 * of out at or past cap, and none past the returned count, is written. */
int64_t lt_lzw_encode_core(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);

/* Every strip of one strip-organised TIFF image decoded on `threads` threads into `out`, the
 * [bands, height, width] samples in native byte order (what ds2array gives per band,
 * /root/reference/utils.py:272-282): compression 1 or 5, predictor 1 or 2 (integer horizontal
 * differencing, undone with wrap), planar 1 (chunky: de-interleaved here) or 2; a short strip is
 * zero-padded as libtiff pads it. Strip k of `file` is file[offsets[k] : offsets[k] + counts[k]].
 * Returns 0 or a negative LT_IO_ERR_*. */
int64_t lt_tiff_decode_strips(const uint8_t* file, int64_t file_size, const uint64_t* offsets,
                              const uint64_t* counts, int64_t n_strips, int compression,
                              int predictor, int bps, int big_endian, int64_t width,
                              int64_t height, int bands, int planar, int64_t rows_per_strip,
                              uint8_t* out, int threads);
/* [bands, rows, cols] samples (little-endian) -> the strips of a planar-2 TIFF image, band by
 * band, rows_per_strip rows each, compression 1 or 5 (array2raster's COMPRESS=LZW,
 * utils.py:386), predictor 1 or 2, encoded on `threads` threads and laid back to back in `out`
 * (cap bytes); strip_sizes[k] gets each strip's length. Returns the total bytes or a negative
 * LT_IO_ERR_*. */
int64_t lt_tiff_encode_strips(const uint8_t* in, int bands, int64_t rows, int64_t cols, int bps,
                              int64_t rows_per_strip, int compression, int predictor, uint8_t* out,
                              int64_t cap, int64_t* strip_sizes, int threads);

/* One zlib stream (RFC 1950 / 1951: TIFF Compression 8 and 32946) -> its raw bytes, by the decoder
 * core the device runs (land_trendr_amd/csrc/lt_inflate_core.h, one lane per chunk in
 * lt_tiff_decode_chunks_dev), compiled for the host. zlib's lazy rule, as a caller of zlib sees it
 * who offers room for cap + 1 bytes to tell a stream of cap bytes from a longer one: the stream is
 * decoded to the end of its final block and its Adler-32 checked (LT_IO_ERR_DATA for anything
 * zlib rejects, truncation included; trailing bytes ignored); byte cap is decoded and checked but
 * not stored, and a symbol that needs space past it ends the call with success and returns cap
 * (so a fault exactly one byte behind cap is an error, one further behind is not seen). No byte
 * at or past out + cap, and none past the returned count, is written; no byte at or past
 * in + n_in is read. */
int64_t lt_inflate_core(const uint8_t* in, int64_t n_in, uint8_t* out, int64_t cap);

/* Every chunk (strip or tile) of one TIFF image decoded on `threads` threads into `out`, the
 * [bands, height, width] samples in native byte order, by the chunk decoder the device runs
 * (land_trendr_amd/csrc/lt_chunk.h; lt_tiff_decode_chunks_dev of include/lt_abi.h, whose
 * lt_chunks_job these arguments spell out, every pointer a host pointer). tiled 0: strips of
 * chunk_h rows, chunk_w == width, the last one short; tiled 1: chunk_w x chunk_h tiles, all full
 * size, ceil(W / chunk_w) * ceil(H / chunk_h) per band (times the bands for planar 2), edge tiles
 * clipped on both axes. Compression 1, 5 or 8 (map 32946 to 8), predictor 1 or 2 (along the
 * chunk's row, padding included), either byte order, planar 1 or 2, bps 1, 2, 4 or 8; a chunk
 * decodes to less than 1 MiB. A short chunk is zero-padded (compression 8: a stream that ends
 * early but validly). Returns 0; LT_IO_ERR_ARG (nothing decoded) for anything outside this list
 * or fewer chunks than the image has; else the LT_IO_ERR_* of some failing chunk (a stream the
 * decoder rejects, an offset or count outside the file): its pixels are unspecified, every other
 * chunk is decoded. */
int64_t lt_tiff_decode_chunks(const uint8_t* file, int64_t file_size, const uint64_t* offsets,
                              const uint64_t* counts, int64_t n_chunks, int compression,
                              int predictor, int bps, int big_endian, int64_t width,
                              int64_t height, int bands, int planar, int64_t chunk_w,
                              int64_t chunk_h, int tiled, uint8_t* out, int threads);

/* One raster sampled at the grid points of a job in raster order: what pt2val / apply_grid do per
 * point (utils.py:285-297, 328-359 of the reference), by the sampling core the device runs
 * (land_trendr_amd/csrc/lt_sample.h; lt_grid_sample_dev of include/lt_abi.h, whose lt_sample_job
 * these arguments spell out, every pointer a host pointer) on `threads` threads. mode 0 (bands):
 * out[b][i] = on ? src[sel[b]][yoff[r] * src_w + xoff[c]] : 0 and valid[i] = on for grid pixel
 * p0 + i = r * grid_w + c, on = both offsets inside the source; mode 1 (mask): valid[i] &=
 * !(on && the sample of band sel[0] is zero). Returns 0, or LT_IO_ERR_ARG (nothing written) for
 * what lt_grid_sample_dev rejects. */
int64_t lt_grid_sample(const void* src, int bps, int src_bands, int64_t src_h, int64_t src_w,
                       const int32_t* xoff, const int32_t* yoff, int64_t grid_w, int64_t grid_h,
                       int64_t p0, int64_t n, int n_sel, const int32_t* sel, void* out,
                       int64_t out_stride, uint8_t* valid, int mode, int threads);

#ifdef __cplusplus
}
#endif
#endif
