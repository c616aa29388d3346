"""The host side of the device strip decoder: lt_strips_job's ctypes mirror against the header,
GeoTiff.device_eligible, ingest_stack's device_decode hook (driven by a host stand-in) and the
lazily completed stack of a decode='device' job. The decoder itself: tests/test_gpu_decode.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from land_trendr_amd import _abi, ingest
from land_trendr_amd.geotiff import GeoTiff, TiffError
from land_trendr_amd.job import LocalJob, _LazyBands
from land_trendr_amd.raster import write_geotiff

from jobfixture import make_job

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_strips_job_layout_matches_header(tmp_path):
    cls = _abi.LtStripsJob
    lines = ['#include <stdio.h>', '#include <stddef.h>',
             '#include "%s"' % os.path.join(ROOT, 'include', 'lt_abi.h'), 'int main(void){',
             'printf("size %zu\\n", sizeof(lt_strips_job));']
    for f, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(lt_strips_job, %s));' % (f, f))
    lines.append('return 0;}')
    c = tmp_path / 'l.c'
    c.write_text('\n'.join(lines))
    exe = str(tmp_path / 'l')
    subprocess.check_call(['gcc', '-o', exe, str(c)])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(got['size']) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert _abi.LT_ABI_VERSION == 8 and 'lt_tiff_decode_strips_dev' in _abi.EXPORTS


def test_device_eligible(tmp_path):
    a = np.arange(2 * 6 * 10, dtype=np.int16).reshape(2, 6, 10)
    cases = [(dict(), True), (dict(predictor=2), True), (dict(compress=None), True),
             (dict(compress='deflate'), False)]
    for k, (kw, want) in enumerate(cases):
        p = str(tmp_path / ('a%d.tif' % k))
        write_geotiff(p, a, nodata=None, **kw)
        g = GeoTiff(p)
        assert g.device_eligible() is want, kw
        if not want:
            with pytest.raises(TiffError):
                g.read_device(None)  # refused before an engine is touched
    # a strip that decodes to 1 MiB: the host path's (the device table packs 20-bit positions)
    p = str(tmp_path / 'big.tif')
    write_geotiff(p, np.zeros((1, 4, 1 << 18), np.uint8), nodata=None, rows_per_strip=4)
    assert not GeoTiff(p).device_eligible()
    write_geotiff(p, np.zeros((1, 4, 1 << 18), np.uint8), nodata=None, rows_per_strip=3)
    assert GeoTiff(p).device_eligible()
    f = str(tmp_path / 'f.tif')
    write_geotiff(f, a.astype(np.float32), nodata=None)
    assert GeoTiff(f).device_eligible()  # predictor 1: any sample format


def test_ingest_offers_only_in_place_rasters(tmp_path):
    """device_decode sees the rasters read in place (raster order, every band) and no other (the
    shifted raster is gathered by offsets); an accepted raster's host planes are left alone and
    on_raster gets None for them; a refused one takes the host path."""
    root = str(tmp_path)
    make_job(root)
    j = LocalJob(root, 'synth', engine=object())
    j.setup()
    assert j.raster_grid is not None
    want = ingest.ingest_stack(j.rast_fns, j.grid_xy, j.mask_fns, raster_grid=j.raster_grid)
    K, P = len(j.rast_fns), want['n_pix']
    # one full range, a job's tiles back to back, and a rank's share of the tiles (never offered)
    for pixels, offer in ((None, True), ([(0, 50), (50, P)], True), ([(0, 50)], False)):
        offered, planes, seen = [], {}, {}

        def dec(k, ds):
            offered.append(k)
            assert isinstance(ds, GeoTiff) and ds.device_eligible()
            if k % 2:
                return False
            planes[k] = ds.read().reshape(ds.bands, -1)
            return True

        def on_raster(k, b, v):
            seen[k] = b is None
        got = ingest.ingest_stack(j.rast_fns, j.grid_xy, j.mask_fns, raster_grid=j.raster_grid,
                                  pixels=pixels, on_raster=on_raster, device_decode=dec)
        Q = got['valid'].shape[1]
        # (jobfixture shifts raster 3: gathered by offsets)
        assert sorted(offered) == ([k for k in range(K) if k != 3] if offer else [])
        assert seen == {k: (k in planes) for k in range(K)}
        assert np.array_equal(got['valid'], want['valid'][:, :Q]) and got['dates'] == want['dates']
        for k in range(K):
            if k in planes:
                assert np.array_equal(planes[k], want['bands'][k])
            else:
                assert np.array_equal(got['bands'][k], want['bands'][k][:, :Q])


def test_lazy_bands_complete_once():
    calls = []

    def fill(host):
        calls.append(1)
        host[1] = 7
    st = _LazyBands({'bands': np.zeros((2, 1, 3), np.int16), 'valid': np.ones((2, 3), np.uint8),
                     'n_pix': 3}, fill)
    assert st['n_pix'] == 3 and st['valid'].all() and not calls  # nothing but 'bands' fills
    assert (st['bands'][1] == 7).all() and not st['bands'][0].any()
    assert (st.get('bands')[1] == 7).all() and calls == [1]
    assert isinstance(st, dict) and set(st) == {'bands', 'valid', 'n_pix'}


def test_job_decode_argument(tmp_path, monkeypatch):
    monkeypatch.delenv('LT_JOB_DECODE', raising=False)
    assert LocalJob(str(tmp_path), 'j', engine=object()).decode == 'host'
    assert LocalJob(str(tmp_path), 'j', engine=object(), decode='device').decode == 'device'
    monkeypatch.setenv('LT_JOB_DECODE', 'device')
    assert LocalJob(str(tmp_path), 'j', engine=object()).decode == 'device'
    assert LocalJob(str(tmp_path), 'j', engine=object(), decode='host').decode == 'host'
    with pytest.raises(ValueError):
        LocalJob(str(tmp_path), 'j', engine=object(), decode='gpu')
