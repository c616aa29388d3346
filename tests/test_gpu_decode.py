"""The HIP strip decoder (lt_tiff_decode_strips_dev, lt_decode.hip) through GeoTiff.read_device,
Engine.decode_strips and LocalJob(decode='device'), against the host decoders: the native strip
path (GeoTiff.read) and, on intact files, the per-strip Python path (read(native=False)). The strip
TIFFs are written by hand here (any byte order, chunky or planar, predictor 2, edited strips)."""
import os
import struct

import numpy as np
import pytest

import lzwfixture
from land_trendr_amd import tiffcodec
from land_trendr_amd.geotiff import GeoTiff, TiffError

pytestmark = pytest.mark.gpu


def _strip_tiff(path, a, bo='<', planar=2, predictor=1, compression=5, rps=3, replace=None,
                edit=None, tiled=False):
    """A strip TIFF written by hand. replace: {strip index: its bytes instead}; edit(offsets,
    counts, file size): changes the two tag lists in place; tiled: one tile per band instead."""
    nb, rows, cols = a.shape
    a = a.astype(a.dtype.newbyteorder(bo))
    if tiled:
        rps = rows
    if planar == 2:
        blocks = [a[b, y:y + rps] for b in range(nb) for y in range(0, rows, rps)]
        spp = 1
    else:
        blocks = [a[:, y:y + rps].transpose(1, 2, 0) for y in range(0, rows, rps)]
        spp = nb
    strips = []
    for blk in blocks:
        blk = np.ascontiguousarray(blk).reshape(blk.shape[0], -1)
        if predictor == 2:
            nat = blk.astype(blk.dtype.newbyteorder('='))
            d = nat.reshape(blk.shape[0], cols, spp).copy()
            d[:, 1:] = d[:, 1:] - d[:, :-1]
            blk = d.reshape(blk.shape).astype(blk.dtype)
        strips.append(tiffcodec.encode(compression, np.ascontiguousarray(blk).tobytes()))
    for k, s in (replace or {}).items():
        strips[k] = s
    fmt_code = 2 if a.dtype.kind == 'i' else (3 if a.dtype.kind == 'f' else 1)
    n_extra = 8 * len(strips) + 64
    off_tag, cnt_tag = (324, 325) if tiled else (273, 279)
    tags = [(256, 4, [cols]), (257, 4, [rows]), (258, 3, [a.dtype.itemsize * 8] * nb),
            (259, 3, [compression]), (262, 3, [1]), (277, 3, [nb]), (284, 3, [planar]),
            (317, 3, [predictor]), (339, 3, [fmt_code] * nb)]
    if tiled:
        tags += [(322, 4, [cols]), (323, 4, [rows])]
    else:
        tags += [(278, 4, [rps])]
    n = len(tags) + 2
    extra_off = 8 + 2 + 12 * n + 4
    data_off = extra_off + n_extra
    offs, o = [], data_off
    for st in strips:
        offs.append(o)
        o += len(st)
    counts = [len(s) for s in strips]
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
        for st in strips:
            f.write(st)
    return path


@pytest.fixture(scope='module')
def eng():
    from land_trendr_amd.engine import get_engine
    return get_engine(0)


def _rand(rng, dtype, shape):
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        return rng.standard_normal(shape).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)


def _same(eng, path, per_strip=True):
    g = GeoTiff(path)
    assert g.device_eligible()
    want = g.read()
    got, err = g.read_device(eng)
    assert got.shape == want.shape and int(err.item()) == 0
    assert np.array_equal(got.cpu().numpy(), want)
    if per_strip:
        assert np.array_equal(want, g.read(native=False))
    return g, want


MATRIX = [('int16', '<', 2, 1, 5), ('int16', '>', 2, 2, 5), ('uint16', '<', 1, 2, 5),
          ('int32', '>', 1, 1, 1), ('uint8', '<', 2, 2, 5), ('int16', '<', 1, 1, 1),
          ('int64', '>', 1, 2, 5), ('int64', '<', 2, 2, 5), ('float64', '>', 2, 1, 5)]


@pytest.mark.parametrize('dtype,bo,planar,predictor,compression', MATRIX)
def test_layout_matrix(eng, tmp_path, dtype, bo, planar, predictor, compression):
    """(3, 11, 7) with 4 rows per strip: 9 strips (3 when chunky), a partial wave, a short last
    strip."""
    a = _rand(np.random.default_rng(1), dtype, (3, 11, 7))
    p = _strip_tiff(str(tmp_path / 'm.tif'), a, bo, planar, predictor, compression, rps=4)
    _, want = _same(eng, p)
    assert np.array_equal(want, a)


def test_more_than_two_waves(eng, tmp_path):
    a = _rand(np.random.default_rng(2), 'int16', (2, 65, 300))
    g, _ = _same(eng, _strip_tiff(str(tmp_path / 'w.tif'), a, rps=1))
    assert len(g.tags[273]) == 130


def test_table_full_clear_and_12_bit_codes(eng, tmp_path):
    a = _rand(np.random.default_rng(3), 'int16', (1, 70, 4200))
    p = _strip_tiff(str(tmp_path / 'c.tif'), a, rps=1)
    g, _ = _same(eng, p)
    raw = open(p, 'rb').read()
    codes = lzwfixture.read_codes(raw[g.tags[273][0]:g.tags[273][0] + g.tags[279][0]])
    assert any(c == lzwfixture.CLEAR for c, _ in codes[1:]) and max(w for _, w in codes) == 12


@pytest.mark.parametrize('kind', ['zeros', 'const', 'period3'])
def test_long_strings_and_kwkwk(eng, tmp_path, kind):
    a = {'zeros': np.zeros((1, 4, 5000), np.uint8), 'const': np.full((1, 4, 5000), 201, np.uint8),
         'period3': np.resize(np.array([1, 2, 3], np.uint8), (1, 4, 5000))}[kind]
    _same(eng, _strip_tiff(str(tmp_path / 'k.tif'), a, rps=1))


def test_divergent_lanes_short_and_cut_strips(eng, tmp_path):
    """Random and constant rows alternate (code counts differ across a wave), height % rps != 0,
    one strip of byte count 0 (zeros), one strip cut by two bytes (no EOI): the host native path's
    values."""
    rng = np.random.default_rng(4)
    a = _rand(rng, 'int16', (2, 70, 600))
    a[:, 1::2] = 77
    a[:, 4:8] = _rand(rng, 'int16', (2, 4, 600))

    def edit(offs, counts, size):
        counts[5] = 0
        counts[9] -= 2
    p = _strip_tiff(str(tmp_path / 'd.tif'), a, rps=3, edit=edit)
    g, want = _same(eng, p, per_strip=False)
    assert 70 % 3 and len(g.tags[273]) == 48
    assert not want[0, 15:18].any() and np.array_equal(want[0, :15], a[0, :15])
    raw = open(p, 'rb').read()
    cut = lzwfixture.read_codes(raw[g.tags[273][9]:g.tags[273][9] + g.tags[279][9]])
    assert cut[-1][0] != lzwfixture.EOI  # the cut strip ends without EOI
    assert np.array_equal(want[1], a[1])


def _job_of(eng, path, out=None):
    import torch
    g = GeoTiff(path)
    rps = min(int(g.tags.get(278, (g.height,))[0]), g.height)
    dev = eng.device
    return dict(file=torch.from_numpy(np.frombuffer(open(path, 'rb').read(), np.uint8).copy()).to(dev),
                offsets=torch.tensor(g.tags[273], dtype=torch.int64, device=dev),
                counts=torch.tensor(g.tags[279], dtype=torch.int64, device=dev),
                compression=g.compression, predictor=g.predictor, dtype=g.dtype, width=g.width,
                height=g.height, bands=g.bands, planar=g.planar, rows_per_strip=rps, out=out)


def test_batch_of_three_images(eng, tmp_path):
    import torch
    rng = np.random.default_rng(5)
    specs = [(_rand(rng, 'int16', (2, 33, 40)), '<', 2, 2, 5, 1),
             (_rand(rng, 'uint8', (3, 10, 129)), '<', 1, 1, 5, 4),
             (_rand(rng, 'int32', (1, 7, 50)), '>', 2, 2, 1, 2)]
    paths = [_strip_tiff(str(tmp_path / ('b%d.tif' % k)), a, bo, pl, pr, co, rps)
             for k, (a, bo, pl, pr, co, rps) in enumerate(specs)]
    pre = torch.empty((3, 10, 129), dtype=torch.uint8, device=eng.device)
    jobs = [_job_of(eng, p, out=pre if k == 1 else None) for k, p in enumerate(paths)]
    outs, err = eng.decode_strips(jobs)
    torch.cuda.synchronize()
    assert outs[1] is pre and err.cpu().tolist() == [0, 0, 0]
    for p, o, (a, *_) in zip(paths, outs, specs):
        want = GeoTiff(p).read()
        assert np.array_equal(o.cpu().numpy(), want) and np.array_equal(want, a)


def _others_decode(eng, g, good, bad_rows):
    import torch
    out, err = g.read_device(eng, check=False)
    torch.cuda.synchronize()
    assert int(err.item()) == -2  # LT_IO_ERR_DATA
    got = out.cpu().numpy()
    keep = np.ones(good.shape[1], bool)
    keep[bad_rows] = False
    assert np.array_equal(got[:, keep], good[:, keep])  # (nothing is asserted about bad_rows)


def test_errors(eng, tmp_path):
    a = _rand(np.random.default_rng(6), 'int16', (1, 20, 90))
    # a code above free_ent in strip 3 (rows 6..7)
    p = _strip_tiff(str(tmp_path / 'e1.tif'), a, rps=2, replace={3: lzwfixture.bad_code_strip()})
    g = GeoTiff(p)
    with pytest.raises(TiffError):
        g.read()
    with pytest.raises(TiffError):
        g.read_device(eng)
    _others_decode(eng, g, a, slice(6, 8))

    # strip 7's offset past the end of the file (rows 14..15)
    def edit(offs, counts, size):
        offs[7] = size + 1000
    g = GeoTiff(_strip_tiff(str(tmp_path / 'e2.tif'), a, rps=2, edit=edit))
    with pytest.raises(TiffError):
        g.read()
    with pytest.raises(TiffError):
        g.read_device(eng)
    _others_decode(eng, g, a, slice(14, 16))


def test_eligibility(tmp_path):
    from land_trendr_amd.raster import write_geotiff
    a = _rand(np.random.default_rng(7), 'int16', (2, 12, 16))
    tiled = GeoTiff(_strip_tiff(str(tmp_path / 't.tif'), a, tiled=True))
    assert np.array_equal(tiled.read(), a)
    p = str(tmp_path / 'z.tif')
    write_geotiff(p, a, nodata=None, compress='deflate')
    deflate = GeoTiff(p)
    assert deflate.compression == 8 and np.array_equal(deflate.read(), a)
    big = GeoTiff(_strip_tiff(str(tmp_path / 'g.tif'), np.zeros((1, 2, 1 << 19), np.uint8), rps=2))
    for g in (tiled, deflate, big):
        assert not g.device_eligible()
        with pytest.raises(TiffError):  # before anything reaches an engine: none is given
            g.read_device(None)
    assert GeoTiff(_strip_tiff(str(tmp_path / 's.tif'), a)).device_eligible()


def test_job_device_decode_equals_host_decode(tmp_path):
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    jobs, files = {}, {}
    for mode in ('host', 'device'):
        root = str(tmp_path / mode)
        make_job(root)
        kw = {} if mode == 'host' else {'decode': 'device'}
        j = jobs[mode] = LocalJob(root, 'synth', device=0, tile_pixels=50, on_error='skip', **kw)
        files[mode] = j.run()
    h, d = jobs['host'], jobs['device']
    assert h.decode == 'host' and h.decode_stats['device'] == 0
    assert d.decode_stats['device'] >= 1 and d.decode_stats['host'] >= 1
    assert sum(d.decode_stats.values()) == len(d.rast_fns)
    assert sorted(h.planes) == sorted(d.planes)
    for k in h.planes:
        assert h.planes[k].dtype == d.planes[k].dtype, k
        assert np.asarray(h.planes[k]).tobytes() == np.asarray(d.planes[k]).tobytes(), k
    assert sorted(files['host']) == sorted(files['device'])
    for k, paths in files['host'].items():
        for ph, pd in zip(paths, files['device'][k]):
            assert os.path.basename(ph) == os.path.basename(pd)
            assert open(ph, 'rb').read() == open(pd, 'rb').read(), k
    assert np.array_equal(h.stack['valid'], d.stack['valid'])
    assert np.array_equal(h.stack['bands'], d.stack['bands'])
