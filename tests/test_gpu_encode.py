"""The device strip encoder (lt_tiff_encode_strips_dev, land_trendr_amd/csrc/lt_encode.hip) through
Engine.encode_strips, raster.write_geotiff_device and LocalJob(encode='device'), against the host
encoder (tiffcodec.encode_strips, write_geotiff): every comparison is == on bytes."""
import os

import numpy as np
import pytest
import torch

import lzwfixture
from land_trendr_amd import tiffcodec
from land_trendr_amd.geotiff import GeoTiff
from land_trendr_amd.raster import write_geotiff, write_geotiff_device

pytestmark = pytest.mark.gpu

ERR_SPACE = -3
SCAN = np.random.default_rng(7).integers(0, 256, 9000, dtype=np.uint8)


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


def _job(eng, a, rps, comp=5, pred=1):
    return {'data': torch.from_numpy(np.ascontiguousarray(a)).to(eng.device),
            'rows_per_strip': rps, 'compression': comp, 'predictor': pred}


def _check(eng, specs):
    """specs: [(array, rows_per_strip, compression, predictor)] encoded in one call; each job's
    strips, sizes and total against the host encoder's. Returns the host strips per job."""
    res = eng.encode_strips([_job(eng, *s) for s in specs])
    assert len(res) == len(specs)
    strips = []
    for k, ((a, rps, comp, pred), (out, sizes, total)) in enumerate(zip(specs, res)):
        a3 = a if a.ndim == 3 else a[None]
        want, want_sizes = tiffcodec.encode_strips(a3, rps, comp, pred, 2)
        assert sizes.dtype == torch.int64 and total.dtype == torch.int64 and total.numel() == 1
        assert int(total.item()) == len(want), k
        assert np.array_equal(sizes.cpu().numpy(), want_sizes), k
        assert out[:len(want)].cpu().numpy().tobytes() == want.tobytes(), k
        b = np.concatenate([[0], np.cumsum(want_sizes)])
        strips.append([want[b[i]:b[i + 1]].tobytes() for i in range(len(want_sizes))])
    return strips


MATRIX = [('uint8', 1), ('int16', 1), ('int32', 1), ('int64', 1), ('float64', 1),
          ('uint8', 2), ('int16', 2), ('int64', 2)]


@pytest.mark.parametrize('compression', [1, 5])
@pytest.mark.parametrize('dtype,predictor', MATRIX)
def test_layout_matrix(eng, dtype, predictor, compression):
    """(3, 11, 7) with 4 rows per strip: 9 strips, a partial wave, a short last strip."""
    a = _rand(np.random.default_rng(1), dtype, (3, 11, 7))
    before = a.copy()
    j = _job(eng, a, 4, compression, predictor)
    (out, sizes, total), = eng.encode_strips([j])
    want, want_sizes = tiffcodec.encode_strips(a, 4, compression, predictor, 2)
    assert len(want_sizes) == 9
    assert int(total.item()) == len(want) and np.array_equal(sizes.cpu().numpy(), want_sizes)
    assert out[:len(want)].cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(j['data'].cpu().numpy(), before)  # predictor 2 works on a copy


def test_two_dimensional_input(eng):
    a = _rand(np.random.default_rng(2), 'int16', (11, 7))
    _check(eng, [(a, 4, 5, 2)])


def test_more_than_two_waves(eng):
    a = _rand(np.random.default_rng(2), 'int16', (2, 65, 300))
    assert len(_check(eng, [(a, 1, 5, 1)])[0]) == 130


def test_table_full_clear_and_12_bit_codes(eng):
    a = _rand(np.random.default_rng(3), 'int16', (1, 70, 4200))
    strips = _check(eng, [(a, 1, 5, 1)])[0]
    codes = lzwfixture.read_codes(strips[0])
    assert codes[0][0] == lzwfixture.CLEAR
    assert any(c == lzwfixture.CLEAR for c, _ in codes[1:]) and max(w for _, w in codes) == 12


def test_end_of_strip_rule_cases(eng):
    """One-row uint8 rasters: the table fills on the final code (3941: a Clear before EOI) and the
    final code takes the width step (255, 771, 1812: EOI one bit wider), in one call."""
    ns = (3941, 255, 771, 1812)
    strips = _check(eng, [(SCAN[:n].reshape(1, 1, n), 1, 5, 1) for n in ns])
    codes = lzwfixture.read_codes(strips[0][0])
    assert codes[-1][0] == lzwfixture.EOI and codes[-2][0] == lzwfixture.CLEAR
    for st in strips[1:]:
        codes = lzwfixture.read_codes(st[0])
        assert codes[-1][0] == lzwfixture.EOI and codes[-1][1] == codes[-2][1] + 1


@pytest.mark.parametrize('kind', ['zeros', 'const', 'period3'])
def test_long_strings(eng, kind):
    a = {'zeros': np.zeros((1, 4, 5000), np.uint8), 'const': np.full((1, 4, 5000), 7, np.uint8),
         'period3': (np.arange(20000, dtype=np.int64) % 3 + 1).astype(np.uint8)
         .reshape(1, 4, 5000)}[kind]
    _check(eng, [(a, 1, 5, 1)])


def test_divergent_lanes(eng):
    """Random and constant rows alternate, 3 rows per strip, a short last strip (70 % 3 != 0)."""
    a = _rand(np.random.default_rng(4), 'int16', (2, 70, 600))
    a[:, 1::2] = 1234
    assert len(_check(eng, [(a, 3, 5, 1)])[0]) == 48


def test_grid_stride_loop(eng):
    """40000 strips: more than the 32768 lanes in flight."""
    a = _rand(np.random.default_rng(5), 'uint8', (1, 40000, 3))
    assert len(_check(eng, [(a, 1, 5, 1)])[0]) == 40000


def test_batch_of_17(eng):
    """One more raster than one launch takes (16 in the kernels' argument block)."""
    rng = np.random.default_rng(6)
    dts = ['uint8', 'int16', 'int32', 'int64', 'float64', 'uint16', 'float32']
    specs = []
    for k in range(17):
        dt = dts[k % len(dts)]
        shape = (1 + k % 3, 3 + k, 5 + 2 * (k % 4))
        pred = 2 if (k % 2 and np.dtype(dt).kind != 'f') else 1
        specs.append((_rand(rng, dt, shape), 1 + k % 4, 1 if k % 5 == 4 else 5, pred))
    _check(eng, specs)


def test_small_cap(eng):
    """A job whose cap is too small gives LT_IO_ERR_SPACE and writes nothing at or past cap; its
    neighbours in the same call are still correct."""
    rng = np.random.default_rng(8)
    a = _rand(rng, 'int16', (2, 9, 200))
    b = _rand(rng, 'uint8', (1, 7, 50))
    want, want_sizes = tiffcodec.encode_strips(a, 2, 5, 1, 2)
    for cap in (len(want) - 1, len(want) // 2, 1):
        out = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device=eng.device)
        ja = dict(_job(eng, a, 2), out=out, cap=cap)
        r = eng.encode_strips([_job(eng, b, 3), ja, _job(eng, b, 2, 5, 2)])
        assert int(r[1][2].item()) == ERR_SPACE, cap
        got = out.cpu().numpy()
        assert (got[cap:] == 0xA5).all(), cap  # the canary tail
        fit = int(np.searchsorted(np.cumsum(want_sizes), cap, side='right'))
        n = int(np.cumsum(want_sizes)[fit - 1]) if fit else 0
        assert got[:n].tobytes() == want[:n].tobytes(), cap  # the strips that fit whole
        for (o, s, t), rps, pred in ((r[0], 3, 1), (r[2], 2, 2)):
            w, ws = tiffcodec.encode_strips(b, rps, 5, pred, 2)
            assert int(t.item()) == len(w) and np.array_equal(s.cpu().numpy(), ws)
            assert o[:len(w)].cpu().numpy().tobytes() == w.tobytes()
    out = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device=eng.device)
    (o, s, t), = eng.encode_strips([dict(_job(eng, a, 2), out=out, cap=len(want))])
    assert int(t.item()) == len(want)  # the exact size fits
    assert out.cpu().numpy()[:len(want)].tobytes() == want.tobytes()
    assert (out.cpu().numpy()[len(want):] == 0xA5).all()


def test_argument_checks(eng):
    from land_trendr_amd.engine import LtError
    a = np.zeros((1, 4, 1 << 18), np.uint8)
    with pytest.raises(LtError):  # a strip of 1 MiB of raw bytes: the host path's
        eng.encode_strips([_job(eng, a, 4)])
    with pytest.raises(LtError):
        eng.encode_strips([_job(eng, a[:, :, :8], 1, 8)])  # Deflate
    with pytest.raises(LtError):
        eng.encode_strips([_job(eng, a[:, :, :8].astype(np.float32), 1, 5, 2)])
    with pytest.raises(LtError):
        eng.encode_strips([dict(_job(eng, a[:, :, :8], 1), data=torch.zeros(4, 8))])  # on the host
    assert eng.encode_strips([]) == []


def test_eligibility_falls_back_to_the_host_path(eng, tmp_path):
    """What the device encoder refuses goes through write_geotiff without the caller noticing."""
    rng = np.random.default_rng(9)
    cases = [(_rand(rng, 'int16', (2, 9, 13)), dict(compress='deflate')),
             (np.zeros((1, 4, 1 << 18), np.uint8), dict(rows_per_strip=4))]  # 1 MiB strips
    for k, (a, kw) in enumerate(cases):
        ph, pd = str(tmp_path / ('h%d.tif' % k)), str(tmp_path / ('d%d.tif' % k))
        write_geotiff(ph, a, **kw)
        write_geotiff_device(pd, torch.from_numpy(a).to(eng.device), eng, **kw)
        assert open(ph, 'rb').read() == open(pd, 'rb').read(), kw
    f = _rand(rng, 'float32', (9, 13))
    for fn, arg, extra in ((write_geotiff, f, ()),
                           (write_geotiff_device, torch.from_numpy(f).to(eng.device), (eng,))):
        with pytest.raises(ValueError):  # float samples with predictor 2: refused by both
            fn(str(tmp_path / 'f.tif'), arg, *extra, predictor=2)


@pytest.mark.parametrize('dtype,shape,kw', [
    ('uint8', (40, 300), dict()),
    ('int16', (3, 11, 7), dict(predictor=2, rows_per_strip=4)),
    ('float64', (2, 5, 6), dict(compress=None, nodata=None)),
    ('int32', (1, 70, 4200), dict(geotransform=(5e5, 30.0, 0.0, 4.2e6, 0.0, -30.0)))])
def test_write_geotiff_device_and_round_trip(eng, tmp_path, dtype, shape, kw):
    a = _rand(np.random.default_rng(10), dtype, shape)
    ph, pd = str(tmp_path / 'h.tif'), str(tmp_path / 'd.tif')
    write_geotiff(ph, a, **kw)
    write_geotiff_device(pd, torch.from_numpy(a).to(eng.device), eng, **kw)
    assert open(ph, 'rb').read() == open(pd, 'rb').read()
    g = GeoTiff(pd)
    got, err = g.read_device(eng)
    assert int(err.item()) == 0
    assert np.array_equal(got.cpu().numpy(), a if a.ndim == 3 else a[None])


def test_small_cap_uncompressed(eng):
    """Compression 1 takes the direct kernel: the same cap rule (whole strips that fit, nothing at
    or past cap), also with predictor 2."""
    a = _rand(np.random.default_rng(12), 'int16', (2, 9, 50))
    for pred in (1, 2):
        want, want_sizes = tiffcodec.encode_strips(a, 2, 1, pred, 2)
        ends = np.cumsum(want_sizes)
        for cap in (len(want), len(want) - 1, int(ends[3]) + 7, 1):
            out = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device=eng.device)
            (o, sz, t), = eng.encode_strips([dict(_job(eng, a, 2, 1, pred), out=out, cap=cap)])
            got = out.cpu().numpy()
            n = int(ends[ends <= cap][-1]) if (ends <= cap).any() else 0
            assert int(t.item()) == (len(want) if cap >= len(want) else ERR_SPACE), (pred, cap)
            assert np.array_equal(sz.cpu().numpy(), want_sizes), (pred, cap)
            assert got[:n].tobytes() == want[:n].tobytes(), (pred, cap)
            assert (got[max(n, cap):] == 0xA5).all() and (got[n:cap] == 0xA5).all(), (pred, cap)


def test_write_geotiff_device_on_a_side_stream(eng, tmp_path):
    """The raster is produced on a stream that is not the current one; the encode and the copies
    down follow it there."""
    a = _rand(np.random.default_rng(13), 'int16', (2, 300, 700))
    ph, pd = str(tmp_path / 'h.tif'), str(tmp_path / 'd.tif')
    write_geotiff(ph, a)
    side = torch.cuda.Stream(eng.device)
    src = torch.from_numpy(a).to(eng.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t = src.clone()
    write_geotiff_device(pd, t, eng, stream=side)
    assert open(ph, 'rb').read() == open(pd, 'rb').read()


@pytest.mark.parametrize('raster_mode', ['reference', 'typed'])
def test_job_device_encode_equals_host_encode(tmp_path, monkeypatch, raster_mode):
    """'typed' batches mix int32, float64 and uint8 rasters: each gets its own sample type and
    rows per strip."""
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    monkeypatch.delenv('LT_JOB_ENCODE', raising=False)
    jobs, files = {}, {}
    for mode in ('host', 'device'):
        root = str(tmp_path / mode)
        make_job(root)
        kw = {} if mode == 'host' else {'encode': 'device'}
        j = jobs[mode] = LocalJob(root, 'synth', device=0, tile_pixels=50, on_error='skip',
                                  raster_mode=raster_mode, **kw)
        files[mode] = j.run()
    h, d = jobs['host'], jobs['device']
    assert h.encode == 'host' and d.encode == 'device'
    assert len(files['host']) > 0 and sorted(files['host']) == sorted(files['device'])
    n, kinds = 0, set()
    for k, paths in files['host'].items():
        for ph, pd in zip(paths, files['device'][k]):
            assert os.path.basename(ph) == os.path.basename(pd)
            assert open(ph, 'rb').read() == open(pd, 'rb').read(), k
            kinds.add(GeoTiff(pd).dtype.str)
            n += 1
    assert d.encode_stats == {'device': n, 'host': 0}
    assert h.encode_stats == {'device': 0, 'host': n}
    if raster_mode == 'typed':
        assert len(kinds) == 3, kinds  # int32, float64 and uint8 rasters
    else:
        assert len(kinds) == 1, kinds
