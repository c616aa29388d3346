"""TIFF files written by hand for the chunk decoder's tests (test_chunks_host.py on the host,
test_gpu_chunks.py on the device): strips or tiles, either byte order, planar 1 or 2, predictor 1
or 2, compression 1, 5 or 8, with edited chunks and tag lists."""
import os
import struct

import numpy as np

from land_trendr_amd import tiffcodec
from land_trendr_amd.geotiff import GeoTiff
from land_trendr_amd.raster import write_geotiff

# (dtype, byte order, planar, predictor, compression): the sample types spread over the layouts
# (float with predictor 1 only), each compression with both byte orders and both planar values
MATRIX = [('int16', '<', 2, 1, 8), ('int16', '>', 2, 2, 8), ('uint16', '<', 1, 2, 8),
          ('int32', '>', 1, 1, 1), ('uint8', '<', 2, 2, 5), ('int16', '<', 1, 1, 5),
          ('int64', '>', 1, 2, 8), ('int64', '<', 2, 2, 5), ('float64', '>', 2, 1, 8),
          ('uint8', '>', 1, 1, 8), ('int32', '<', 2, 2, 1)]


def rand(rng, dtype, shape):
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        return rng.standard_normal(shape).astype(dt)
    info = np.iinfo(dt)
    # (a narrow range now and then, so that Deflate finds matches and LZW long strings)
    a = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
    a[..., : shape[-1] // 2] = a[..., : shape[-1] // 2] % 5
    return a


def chunk_tiff(path, a, bo='<', planar=2, predictor=1, compression=8, tile=None, rps=4,
               replace=None, edit=None, width=None):
    """A TIFF of the [bands, rows, cols] array `a`, written by hand. tile=(th, tw): tiles, all full
    size with zero padding, else strips of rps rows. replace: {chunk index: its bytes instead};
    edit(offsets, counts, file size): changes the two tag lists in place. width: the ImageWidth
    written (strips whose rows are given ready-made through `replace`)."""
    nb, rows, cols = a.shape
    a = a.astype(a.dtype.newbyteorder(bo))
    if tile is not None:
        th, tw = tile
        ext = np.zeros((nb, -(-rows // th) * th, -(-cols // tw) * tw), a.dtype)
        ext[:, :rows, :cols] = a
        boxes = [(y, y + th, x, x + tw) for y in range(0, rows, th) for x in range(0, cols, tw)]
    else:
        ext, tw = a, cols
        boxes = [(y, min(y + rps, rows), 0, cols) for y in range(0, rows, rps)]
    if planar == 2:
        blocks = [ext[b, y0:y1, x0:x1] for b in range(nb) for y0, y1, x0, x1 in boxes]
        spp = 1
    else:
        blocks = [ext[:, y0:y1, x0:x1].transpose(1, 2, 0) for y0, y1, x0, x1 in boxes]
        spp = nb
    chunks = []
    for blk in blocks:
        blk = np.ascontiguousarray(blk).reshape(blk.shape[0], -1)
        if predictor == 2:
            nat = blk.astype(blk.dtype.newbyteorder('='))
            d = nat.reshape(blk.shape[0], tw, spp).copy()
            d[:, 1:] = d[:, 1:] - d[:, :-1]
            blk = d.reshape(blk.shape).astype(blk.dtype)
        chunks.append(tiffcodec.encode(compression, np.ascontiguousarray(blk).tobytes()))
    for k, s in (replace or {}).items():
        chunks[k] = s
    fmt_code = 2 if a.dtype.kind == 'i' else (3 if a.dtype.kind == 'f' else 1)
    n_extra = 8 * len(chunks) + 64
    off_tag, cnt_tag = (324, 325) if tile is not None else (273, 279)
    tags = [(256, 4, [width or cols]), (257, 4, [rows]), (258, 3, [a.dtype.itemsize * 8] * nb),
            (259, 3, [compression]), (262, 3, [1]), (277, 3, [nb]), (284, 3, [planar]),
            (317, 3, [predictor]), (339, 3, [fmt_code] * nb)]
    if tile is not None:
        tags += [(322, 4, [tile[1]]), (323, 4, [tile[0]])]
    else:
        tags += [(278, 4, [rps])]
    n = len(tags) + 2
    extra_off = 8 + 2 + 12 * n + 4
    data_off = extra_off + n_extra
    offs, o = [], data_off
    for c in chunks:
        offs.append(o)
        o += len(c)
    counts = [len(c) for c in chunks]
    if edit is not None:
        edit(offs, counts, o)
    tags += [(off_tag, 4, offs), (cnt_tag, 4, counts)]
    tags.sort()
    fmt = {3: 'H', 4: 'I'}
    extra = b''
    ifd = struct.pack(bo + 'H', n)
    for tag, typ, vals in tags:
        payload = struct.pack(bo + fmt[typ] * len(vals), *vals)
        if len(payload) <= 4:
            ifd += struct.pack(bo + 'HHI', tag, typ, len(vals)) + payload.ljust(4, b'\x00')
        else:
            ifd += struct.pack(bo + 'HHII', tag, typ, len(vals), extra_off + len(extra))
            extra += payload
    ifd += struct.pack(bo + 'I', 0)
    assert len(extra) <= n_extra
    with open(path, 'wb') as f:
        f.write((b'II' if bo == '<' else b'MM') + struct.pack(bo + 'HI', 42, 8))
        f.write(ifd)
        f.write(extra.ljust(n_extra, b'\x00'))
        for c in chunks:
            f.write(c)
    return path


def host_chunks(g, threads=2, check=True):
    """tiffcodec.decode_chunks of an open GeoTiff: (array, return code)."""
    otag, ctag, cw, ch, tiled, _ = g.chunk_layout()
    return tiffcodec.decode_chunks(g._d, g.tags[otag], g.tags[ctag], g.compression, g.predictor,
                                   g.dtype, g._bo == '>', g.width, g.height, g.bands, g.planar,
                                   cw, ch, tiled, threads=threads, check=check)


def chunk_pixels(g, k):
    """The (band slice, row slice, column slice) of the raster that chunk k of g covers."""
    _, _, cw, ch, tiled, _ = g.chunk_layout()
    tx = -(-g.width // cw) if tiled else 1
    per = tx * -(-g.height // ch)
    b, r = (slice(None), k) if g.planar == 1 else (slice(k // per, k // per + 1), k % per)
    y0, x0 = (r // tx) * ch, (r % tx) * cw
    return b, slice(y0, min(y0 + ch, g.height)), slice(x0, min(x0 + cw, g.width))


def retile(root, job='synth'):
    """Every plain raster of a make_job directory (not the cloud masks) rewritten as 16 x 16
    Deflate tiles; returns their paths."""
    rdir = os.path.join(root, job, 'input', 'rasters')
    done = []
    for fn in sorted(os.listdir(rdir)):
        p = os.path.join(rdir, fn)
        if not fn.endswith('.tif') or 'cloudmask' in fn:
            continue
        g = GeoTiff(p)
        a = g.read()
        write_geotiff(p + '.new', a, template=g, nodata=None, compress='deflate', tile=(16, 16))
        del g
        os.replace(p + '.new', p)
        assert np.array_equal(GeoTiff(p).read(), a)
        done.append(p)
    return done
