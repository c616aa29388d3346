"""The host side of the device strip encoder: lt_encode_job's ctypes mirror against the header,
LocalJob's encode argument and its fallback to the host encoder on a CPU engine, and the TIFF
layout helper split out of write_geotiff. The encoder itself: tests/test_gpu_encode.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from land_trendr_amd import _abi, raster, tiffcodec
from land_trendr_amd.job import LocalJob
from land_trendr_amd.raster import write_geotiff

from engine_double import OracleEngine
from jobfixture import make_job

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_encode_job_layout_matches_header(tmp_path):
    cls = _abi.LtEncodeJob
    c_name = {'in_': 'in'}  # (`in` is a Python keyword)
    lines = ['#include <stdio.h>', '#include <stddef.h>',
             '#include "%s"' % os.path.join(ROOT, 'include', 'lt_abi.h'), 'int main(void){',
             'printf("size %zu\\n", sizeof(lt_encode_job));']
    for f, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(lt_encode_job, %s));' % (f, c_name.get(f, f)))
    lines.append('return 0;}')
    c = tmp_path / 'l.c'
    c.write_text('\n'.join(lines))
    exe = str(tmp_path / 'l')
    subprocess.check_call(['gcc', '-o', exe, str(c)])
    got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(got['size']) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert _abi.LT_ABI_VERSION == 8 and 'lt_tiff_encode_strips_dev' in _abi.EXPORTS


def test_job_encode_argument(tmp_path, monkeypatch):
    monkeypatch.delenv('LT_JOB_ENCODE', raising=False)
    assert LocalJob(str(tmp_path), 'j', engine=object()).encode == 'host'
    assert LocalJob(str(tmp_path), 'j', engine=object(), encode='device').encode == 'device'
    monkeypatch.setenv('LT_JOB_ENCODE', 'device')
    assert LocalJob(str(tmp_path), 'j', engine=object()).encode == 'device'
    assert LocalJob(str(tmp_path), 'j', engine=object(), encode='host').encode == 'host'
    with pytest.raises(ValueError):
        LocalJob(str(tmp_path), 'j', engine=object(), encode='gpu')
    assert LocalJob(str(tmp_path), 'j', engine=object()).encode_stats == {'device': 0, 'host': 0}


def test_device_encode_falls_back_on_a_cpu_engine(tmp_path, monkeypatch):
    monkeypatch.delenv('LT_JOB_ENCODE', raising=False)
    jobs, files = {}, {}
    for mode in ('host', 'device'):
        root = str(tmp_path / mode)
        make_job(root)
        j = jobs[mode] = LocalJob(root, 'synth', tile_pixels=40, on_error='skip',
                                  engine=OracleEngine(), encode=mode)
        files[mode] = j.run()
    assert len(files['host']) > 0 and sorted(files['host']) == sorted(files['device'])
    for k, paths in files['host'].items():
        for ph, pd in zip(paths, files['device'][k]):
            assert os.path.basename(ph) == os.path.basename(pd)
            assert open(ph, 'rb').read() == open(pd, 'rb').read(), k
    for mode in ('host', 'device'):
        assert jobs[mode].encode_stats == {'device': 0, 'host': len(files[mode])}, mode


@pytest.mark.parametrize('dtype,shape,kw', [
    ('uint8', (9, 13), dict()),
    ('int16', (3, 11, 7), dict(predictor=2, rows_per_strip=4)),
    ('float64', (2, 5, 6), dict(compress=None, rows_per_strip=2)),
    ('int32', (1, 40, 300), dict(nodata=None, geotransform=(5e5, 30.0, 0.0, 4.2e6, 0.0, -30.0)))])
def test_layout_helper_reproduces_write_geotiff(tmp_path, dtype, shape, kw):
    rng = np.random.default_rng(4)
    a = (rng.standard_normal(shape) * 100).astype(dtype)
    want = str(tmp_path / 'w.tif')
    write_geotiff(want, a, **kw)
    b = a if a.ndim == 3 else a[None]
    nb, rows, cols = b.shape
    comp = {None: 1, 'lzw': 5}[kw.get('compress', 'lzw')]
    pred = kw.get('predictor', 1)
    rps = raster._strip_rows(rows, cols, b.dtype.itemsize, kw.get('rows_per_strip'))
    data, sizes = tiffcodec.encode_strips(b, rps, comp, pred, 2)
    assert len(sizes) == nb * -(-rows // rps)
    got = str(tmp_path / 'g.tif')
    raster.write_tiff_strips(got, data, sizes, (nb, rows, cols), b.dtype, comp, pred, rps, None,
                             kw.get('geotransform'), kw.get('nodata', raster.NODATA))
    assert open(got, 'rb').read() == open(want, 'rb').read()
    with pytest.raises(ValueError):  # the bytes and the sizes must agree
        raster.write_tiff_strips(got, data[:-1], sizes, (nb, rows, cols), b.dtype, comp, pred,
                                 rps)


def test_device_encodable():
    ok = raster.device_encodable
    assert ok(np.uint8, (9, 13)) and ok(np.int16, (3, 11, 7), 'lzw', 2) and ok('f8', (5, 6), None)
    assert not ok(np.uint8, (9, 13), 'deflate')
    assert not ok(np.float32, (9, 13), 'lzw', 2)
    assert not ok(np.uint8, (4, 1 << 18), rows_per_strip=4)  # a strip of 1 MiB raw: the host's
    assert ok(np.uint8, (4, 1 << 18), rows_per_strip=3)
