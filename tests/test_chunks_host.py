"""The host side of the device chunk decoder: lt_chunks_job's ctypes mirror against the header, the
chunk decoder the device runs (lt_chunk.h) built for the host (tiffcodec.decode_chunks) against
the per-chunk Python path on every geometry, the tiled writer, GeoTiff.device_chunks_eligible and
LocalJob's device_formats. The device itself: tests/test_gpu_chunks.py."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

import inflatefixture
from chunkfixture import MATRIX, chunk_pixels, chunk_tiff, host_chunks, rand, retile
from jobfixture import make_job
from land_trendr_amd import _abi, ingest, tiffcodec
from land_trendr_amd.geotiff import GeoTiff, TiffError
from land_trendr_amd.job import LocalJob
from land_trendr_amd.raster import device_encodable, write_geotiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_DATA = -2


def test_chunks_job_layout_matches_header(tmp_path):
    cls = _abi.LtChunksJob
    lines = ['#include <stdio.h>', '#include <stddef.h>',
             '#include "%s"' % os.path.join(ROOT, 'include', 'lt_abi.h'), 'int main(void){',
             'printf("size %zu\\n", sizeof(lt_chunks_job));']
    for f, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(lt_chunks_job, %s));' % (f, f))
    lines.append('return 0;}')
    c = tmp_path / 'l.c'
    c.write_text('\n'.join(lines))
    exe = str(tmp_path / 'l')
    subprocess.check_call(['gcc', '-o', exe, str(c)])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(got['size']) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert _abi.LT_ABI_VERSION == 8 and 'lt_tiff_decode_chunks_dev' in _abi.EXPORTS


def _same(path, chunks):
    g = GeoTiff(path)
    assert g.device_chunks_eligible()
    assert g.chunk_layout()[5] == chunks
    want = g.read(native=False)
    got, rc = host_chunks(g)
    assert rc == 0 and got.dtype == want.dtype
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    return g, want


@pytest.mark.parametrize('dtype,bo,planar,predictor,compression', MATRIX)
def test_tiles(tmp_path, dtype, bo, planar, predictor, compression):
    """(3, 37, 41) in 16 x 16 tiles: 3 x 3 tiles per band, the edge tiles clipped on both axes."""
    a = rand(np.random.default_rng(1), dtype, (3, 37, 41))
    p = chunk_tiff(str(tmp_path / 't.tif'), a, bo, planar, predictor, compression, tile=(16, 16))
    _, want = _same(p, 27 if planar == 2 else 9)
    assert np.array_equal(want.view(np.uint8), a.view(np.uint8))


@pytest.mark.parametrize('dtype,bo,planar,predictor,compression', MATRIX)
def test_strips(tmp_path, dtype, bo, planar, predictor, compression):
    """The same image in strips of 4 rows: a short last strip."""
    a = rand(np.random.default_rng(2), dtype, (3, 37, 41))
    p = chunk_tiff(str(tmp_path / 's.tif'), a, bo, planar, predictor, compression, rps=4)
    g, want = _same(p, 30 if planar == 2 else 10)
    assert np.array_equal(want.view(np.uint8), a.view(np.uint8))
    if compression != 8:  # the strip decoder's files: the native strip path agrees too
        assert g.device_eligible() and np.array_equal(g.read(), want)


def test_non_square_tiles_and_old_deflate_code(tmp_path):
    a = rand(np.random.default_rng(3), 'int16', (2, 50, 33))
    p = chunk_tiff(str(tmp_path / 'r.tif'), a, '<', 2, 2, 8, tile=(32, 16))
    _same(p, 2 * 2 * 3)
    raw = bytearray(open(p, 'rb').read())
    k = raw.index(b'\x03\x01\x03\x00\x01\x00\x00\x00\x08\x00')  # tag 259 SHORT 1 = 8
    raw[k + 8:k + 10] = (32946).to_bytes(2, 'little')
    q = str(tmp_path / 'old.tif')
    open(q, 'wb').write(bytes(raw))
    assert GeoTiff(q).compression == 32946
    _same(q, 12)


@pytest.mark.parametrize('planar', [1, 2])
def test_failing_chunks_leave_the_others(tmp_path, planar):
    """One tile count set to 0 and one Deflate tile replaced by too_far_back: LT_IO_ERR_DATA, and
    every other tile's pixels are the intact file's."""
    a = rand(np.random.default_rng(4), 'int16', (3, 37, 41))
    good = chunk_tiff(str(tmp_path / 'g.tif'), a, '<', planar, 2, 8, tile=(16, 16))
    want = GeoTiff(good).read(native=False)

    def edit(offs, counts, size):
        counts[1] = 0
    bad = chunk_tiff(str(tmp_path / 'b.tif'), a, '<', planar, 2, 8, tile=(16, 16),
                     replace={5: inflatefixture.too_far_back()}, edit=edit)
    g = GeoTiff(bad)
    with pytest.raises((TiffError, zlib.error)):
        g.read(native=False)  # host zlib raises on the same file
    got, rc = host_chunks(g, check=False)
    assert rc == ERR_DATA
    with pytest.raises(ValueError):
        host_chunks(g)
    ok = np.ones(a.shape, bool)
    for k in (1, 5):
        b, ys, xs = chunk_pixels(g, k)
        ok[b, ys, xs] = False
    assert (~ok).any() and np.array_equal(got[ok], want[ok])

    def past(offs, counts, size):
        offs[2] = size + 5
    bad = chunk_tiff(str(tmp_path / 'p.tif'), a, '<', planar, 2, 8, tile=(16, 16), edit=past)
    g = GeoTiff(bad)
    got, rc = host_chunks(g, check=False)
    assert rc == ERR_DATA
    ok = np.ones(a.shape, bool)
    b, ys, xs = chunk_pixels(g, 2)
    ok[b, ys, xs] = False
    assert np.array_equal(got[ok], want[ok])


def test_short_valid_stream_is_zero_padded(tmp_path):
    """A Deflate strip that ends early but validly: zero-padded, as tiffcodec.decode pads it."""
    a = rand(np.random.default_rng(5), 'uint8', (1, 8, 40))
    p = chunk_tiff(str(tmp_path / 'z.tif'), a, rps=4, compression=8,
                   replace={1: zlib.compress(a[0, 4:6].tobytes())})
    g = GeoTiff(p)
    got, rc = host_chunks(g)
    assert rc == 0 and np.array_equal(got, g.read(native=False))
    assert np.array_equal(got[0, :6], a[0, :6]) and not got[0, 6:].any()


def test_rejected_arguments():
    L = tiffcodec._lib()
    buf = np.zeros(64, np.uint8)
    tab = np.zeros(4, np.uint64)
    out = np.zeros(64, np.uint8)

    def call(**kw):
        a = dict(file=buf.ctypes.data, size=64, offs=tab.ctypes.data, cnts=tab.ctypes.data, n=4,
                 comp=8, pred=1, bps=1, be=0, w=8, h=8, bands=1, planar=2, cw=4, ch=4, tiled=1,
                 out=out.ctypes.data)
        a.update(kw)
        return L.lt_tiff_decode_chunks(a['file'], a['size'], a['offs'], a['cnts'], a['n'],
                                       a['comp'], a['pred'], a['bps'], a['be'], a['w'], a['h'],
                                       a['bands'], a['planar'], a['cw'], a['ch'], a['tiled'],
                                       a['out'], 1)
    assert call() == ERR_DATA  # (four empty streams: accepted arguments)
    for kw in (dict(file=None), dict(offs=None), dict(cnts=None), dict(out=None), dict(w=0),
               dict(h=-1), dict(bands=0), dict(cw=0), dict(ch=0), dict(bps=3), dict(comp=32773),
               dict(comp=7), dict(pred=3), dict(planar=3), dict(n=3),
               dict(tiled=0, cw=4),                       # strips narrower than the image
               dict(w=2048, h=512, cw=1024, ch=1024)):    # a chunk of 1 MiB
        assert call(**kw) == -1, kw
    assert call(w=2048, h=512, cw=1024, ch=1023, n=2) == ERR_DATA


@pytest.mark.parametrize('compress', ['lzw', 'deflate', None])
def test_tiled_writer(tmp_path, compress):
    a = rand(np.random.default_rng(6), 'int16', (2, 37, 70))
    p = str(tmp_path / 'w.tif')
    write_geotiff(p, a, nodata=None, compress=compress, predictor=2, tile=(16, 32))
    g = GeoTiff(p)
    assert (int(g.tags[323][0]), int(g.tags[322][0])) == (16, 32) and 273 not in g.tags
    assert g.planar == 2 and len(g.tags[324]) == 2 * 3 * 3
    assert np.array_equal(g.read(), a)
    got, rc = host_chunks(g)
    assert rc == 0 and np.array_equal(got, a)
    write_geotiff(p, a[0], nodata=None, compress=compress, tile=(16, 16))
    assert np.array_equal(GeoTiff(p).read()[0], a[0])
    with pytest.raises(ValueError):
        write_geotiff(p, a, nodata=None, tile=(16, 24))
    assert device_encodable(a.dtype, a.shape) and not device_encodable(a.dtype, a.shape,
                                                                       tile=(16, 16))


def test_tile_none_writes_the_same_bytes(tmp_path):
    a = rand(np.random.default_rng(7), 'int16', (2, 20, 30))
    p, q = str(tmp_path / 'a.tif'), str(tmp_path / 'b.tif')
    for kw in (dict(), dict(compress='deflate', predictor=2), dict(compress=None)):
        write_geotiff(p, a, geotransform=(0, 30, 0, 0, 0, -30), **kw)
        write_geotiff(q, a, geotransform=(0, 30, 0, 0, 0, -30), tile=None, **kw)
        assert open(p, 'rb').read() == open(q, 'rb').read()


def test_device_chunks_eligible(tmp_path):
    a = np.arange(2 * 40 * 50, dtype=np.int16).reshape(2, 40, 50)
    cases = [(dict(), True, True), (dict(predictor=2), True, True),
             (dict(compress=None), True, True), (dict(compress='deflate'), True, False),
             (dict(tile=(16, 16)), True, False), (dict(compress='deflate', tile=(16, 16)), True,
                                                  False)]
    for k, (kw, chunks, strips) in enumerate(cases):
        p = str(tmp_path / ('a%d.tif' % k))
        write_geotiff(p, a, nodata=None, **kw)
        g = GeoTiff(p)
        assert g.device_chunks_eligible() is chunks and g.device_eligible() is strips, kw
    f = a.astype(np.float32)
    p = chunk_tiff(str(tmp_path / 'p3.tif'), f, predictor=3, compression=8, tile=(16, 16))
    g = GeoTiff(p)
    assert not g.device_chunks_eligible() and not g.device_eligible()
    with pytest.raises(TiffError):
        g.read_device_chunks(None)  # refused before an engine is touched
    p = chunk_tiff(str(tmp_path / 'pb.tif'), a, compression=1, rps=4)
    raw = bytearray(open(p, 'rb').read())
    k = raw.index(b'\x03\x01\x03\x00\x01\x00\x00\x00\x01\x00')
    raw[k + 8:k + 10] = (32773).to_bytes(2, 'little')
    open(p, 'wb').write(bytes(raw))
    g = GeoTiff(p)
    assert g.compression == 32773 and not g.device_chunks_eligible() and not g.device_eligible()
    # a tile that decodes to 1 MiB: the host path's
    p = str(tmp_path / 'big.tif')
    write_geotiff(p, np.zeros((1, 1024, 1024), np.uint8), nodata=None, tile=(1024, 1024))
    assert not GeoTiff(p).device_chunks_eligible()
    write_geotiff(p, np.zeros((1, 1024, 1024), np.uint8), nodata=None, tile=(1024, 1008))
    assert GeoTiff(p).device_chunks_eligible() and not GeoTiff(p).device_eligible()


def test_device_formats_argument(monkeypatch):
    monkeypatch.delenv('LT_JOB_DEVICE_FORMATS', raising=False)
    monkeypatch.delenv('LT_JOB_DECODE', raising=False)
    assert LocalJob('r', 'j', engine=object()).device_formats == 'strips'
    assert LocalJob('r', 'j', engine=object(), decode='device').device_formats == 'strips'
    assert LocalJob('r', 'j', engine=object(), decode='device',
                    device_formats='all').device_formats == 'all'
    with pytest.raises(ValueError):
        LocalJob('r', 'j', engine=object(), device_formats='all')  # needs decode='device'
    with pytest.raises(ValueError):
        LocalJob('r', 'j', engine=object(), decode='host', device_formats='all')
    with pytest.raises(ValueError):
        LocalJob('r', 'j', engine=object(), decode='device', device_formats='tiles')
    monkeypatch.setenv('LT_JOB_DEVICE_FORMATS', 'all')
    assert LocalJob('r', 'j', engine=object(), decode='device').device_formats == 'all'
    assert LocalJob('r', 'j', engine=object(), decode='device',
                    device_formats='strips').device_formats == 'strips'


def test_ingest_offers_tiles_only_with_all(tmp_path):
    """ingest_stack's device_decode hook, driven by a host stand-in that takes what the job's
    device_formats takes: the rasters rewritten as Deflate tiles are taken with 'all' and left to
    the host with 'strips'; the stack is the same either way."""
    root = str(tmp_path)
    make_job(root)
    j0 = LocalJob(root, 'synth', engine=object())
    j0.setup()
    want = ingest.ingest_stack(j0.rast_fns, j0.grid_xy, j0.mask_fns, raster_grid=j0.raster_grid)
    tiled = retile(root)
    assert len(tiled) >= 3
    for fmt, taken_want in (('all', True), ('strips', False)):
        j = LocalJob(root, 'synth', engine=object(), decode='device', device_formats=fmt)
        j.setup()
        offered, planes = [], {}

        def dec(k, ds):
            offered.append(k)
            if not j.device_takes(ds):
                return False
            a, rc = host_chunks(ds)
            assert rc == 0
            planes[k] = a.reshape(ds.bands, -1)
            return True
        got = ingest.ingest_stack(j.rast_fns, j.grid_xy, j.mask_fns, raster_grid=j.raster_grid,
                                  device_decode=dec)
        assert all(GeoTiff(j.rast_fns[k]).device_chunks_eligible() for k in offered)
        # the rewritten rasters among the offered ones (the others are still LZW strips)
        tiles = [k for k in offered if 324 in GeoTiff(j.rast_fns[k]).tags]
        assert len(tiles) >= 3 and not any(GeoTiff(j.rast_fns[k]).device_eligible() for k in tiles)
        strips = [k for k in offered if k not in tiles]
        assert all(GeoTiff(j.rast_fns[k]).device_eligible() for k in strips)
        assert sorted(planes) == sorted(offered if taken_want else strips)
        assert np.array_equal(got['valid'], want['valid'])
        for k in range(len(j.rast_fns)):
            b = planes[k] if k in planes else got['bands'][k]
            assert np.array_equal(b, want['bands'][k]), k
