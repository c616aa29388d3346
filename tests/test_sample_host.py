"""Grid sampling on the host: ingest.axis_offsets against grid_offsets, and the host build of the
sampling core the device runs (land_trendr_amd/csrc/lt_sample.h, liblt_io.so lt_grid_sample)
against the numpy path ingest_stack takes (np.take at grid_offsets' indices, zero where pt2val
raises, the mask rule); the same core stand-alone under AddressSanitizer / UBSan
(tests/native/grid_sample_check.cpp). Every comparison is exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import samplefixture as sf
from land_trendr_amd import ingest, tiffcodec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _axis(n, origin, size):
    """Coordinates along one axis of a raster of n pixels: centres, exact edges, the neighbours of
    the edges on either side, points before, after and far off the raster, NaN and inf."""
    with np.errstate(all='ignore'):
        edges = origin + np.arange(n + 1) * size
        centres = origin + (np.arange(n) + 0.5) * size
        near = np.concatenate([np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])
        off = origin + np.array([-0.5, -1.0, -1.5, -n + 0.5, -n, -n - 0.5, n + 0.5, n + 1.0,
                                 -2.0 * n, 3.0 * n, 1e9, -1e9, 1e300, -1e300]) * size
    return np.concatenate([centres, edges, near, off, [np.nan, np.inf, -np.inf, 0.0]])


GEOTRANSFORMS = [
    (500000.0, 30.0, 0.0, 4200000.0, 0.0, -30.0),
    (0.05, 0.1, 0.0, 7.3, 0.0, -0.1),
    (-1234.5, 28.5, 0.0, 98765.25, 0.0, -28.5),
    (2.0, 1.0 / 3.0, 0.0, -5.0, 0.0, -1.0 / 3.0),
    (10.0, 0.1, 0.0, 20.0, 0.0, 0.1),           # a positive pixel height
    (3.0, -28.5, 0.0, 4.0, 0.0, -1.0 / 3.0),    # a negative pixel width
    (1.0, 0.0, 0.0, 2.0, 0.0, -30.0),           # a zero pixel width
    (1.0, 30.0, 0.0, 2.0, 0.0, 0.0),            # a zero pixel height
]


@pytest.mark.parametrize('gt', GEOTRANSFORMS)
@pytest.mark.parametrize('shape', [(7, 11), (1, 1), (29, 61)])
def test_axis_offsets_equal_grid_offsets(gt, shape):
    rows, cols = shape
    xv = _axis(cols, gt[0], gt[1] if gt[1] else 30.0)
    yv = _axis(rows, gt[3], gt[5] if gt[5] else -30.0)
    xoff, yoff = ingest.axis_offsets(gt, shape, xv, yv)
    assert xoff.dtype == np.int32 and yoff.dtype == np.int32
    assert xoff.shape == xv.shape and yoff.shape == yv.shape
    assert xoff.min() >= -1 and xoff.max() < cols and yoff.min() >= -1 and yoff.max() < rows
    with np.errstate(all='ignore'):
        idx, ok = ingest.grid_offsets(gt, shape, np.tile(xv, len(yv)), np.repeat(yv, len(xv)))
    on = ((xoff >= 0)[None, :] & (yoff >= 0)[:, None]).ravel()
    flat = (yoff.astype(np.int64)[:, None] * cols + xoff.astype(np.int64)[None, :]).ravel()
    assert np.array_equal(ok, on)
    assert np.array_equal(idx, np.where(on, flat, 0))  # (grid_offsets gives 0 where not ok)
    if gt[1] and gt[5]:
        assert on.any() and not on.all()


def test_axis_offsets_refuses_huge_rasters():
    with pytest.raises(ValueError):
        ingest.axis_offsets(sf.GT, (1 << 31, 4), np.zeros(1), np.zeros(1))


def test_corpus_offsets_cover_the_cases():
    """The corpus wraps, falls off on both sides and hits the last row and column."""
    for spec in (sf.SRC_A, sf.SRC_SMALL):
        src, gt = sf.make_src(0, 'uint8', spec, bands=1)
        xo, yo = sf.offsets(src, gt)
        assert (yo == -1).any() and (yo == spec[0] - 1).any()
        assert (np.diff(yo.astype(np.int64)) < 0).any()  # a wrap
    src, gt = sf.make_src(0, 'uint8', sf.SRC_SMALL, bands=1)
    xo, yo = sf.offsets(src, gt)
    for o, n in ((xo, sf.SRC_SMALL[1]), (yo, sf.SRC_SMALL[0])):
        assert o[0] == -1 and o[-1] == -1 and (o == n - 1).any()


@pytest.mark.parametrize('dtype', sf.DTYPES)
@pytest.mark.parametrize('name', sorted(sf.SOURCES))
def test_host_build_equals_numpy_bands(name, dtype):
    src, gt = sf.make_src(1, dtype, sf.SOURCES[name])
    for sel in sf.SELS:
        for p0, p1 in sf.RANGES:
            want, wv = sf.numpy_bands(src, gt, p0, p1, sel)
            for threads in (1, 3):
                got, gv = sf.host_bands(src, gt, p0, p1, sel, threads=threads)
                assert sf.same(got, want), (sel, p0, p1)
                assert sf.same(gv, wv), (sel, p0, p1)


def test_host_build_many_chunks():
    """More groups than one work item of the pool holds (a grid of 300 x 300)."""
    rng = np.random.default_rng(3)
    src = rng.integers(-30000, 30000, (2, 290, 310), dtype=np.int16)
    gt = sf.source_gt(4, -7)
    n = 300
    xv = sf.GT[0] + (np.arange(n) + 0.5) * sf.GT[1]
    yv = sf.GT[3] + (np.arange(n) + 0.5) * sf.GT[5]
    xo, yo = ingest.axis_offsets(gt, src.shape[1:], xv, yv)
    idx, ok = ingest.grid_offsets(gt, src.shape[1:], np.tile(xv, n), np.repeat(yv, n))
    want = np.take(src.reshape(2, -1), idx, axis=-1)
    want[:, ~ok] = 0
    out = np.empty((2, n * n), np.int16)
    valid = np.empty(n * n, np.uint8)
    tiffcodec.grid_sample(src, xo, yo, 0, n * n, [0, 1], out, n * n, valid, 0, threads=4)
    assert np.array_equal(out, want) and np.array_equal(valid, ok.astype(np.uint8))


@pytest.mark.parametrize('dtype', sf.INT_DTYPES)
def test_host_build_equals_numpy_mask(dtype):
    """A mask with an extent of its own over a validity row that is already partly 0."""
    src, gt = sf.make_src(2, 'int16', sf.SRC_A)
    mask, mgt = sf.make_src(5, dtype, sf.SRC_MASK, bands=2, zeros=0.4)
    for p0, p1 in sf.RANGES:
        _, valid = sf.numpy_bands(src, gt, p0, p1, [0])
        valid[np.random.default_rng(p0).random(len(valid)) < 0.2] = 0
        want = sf.numpy_mask(valid, mask, mgt, p0, p1)
        got = sf.host_mask(valid, mask, mgt, p0, p1)
        assert sf.same(got, want), (p0, p1)
        if p1 - p0 > 100:
            assert 0 < valid.sum() < len(valid) and 0 < want.sum() < valid.sum()


def _raw_call(**kw):
    """lt_grid_sample with every argument spelt out (kw: the ones to replace; None: a null
    pointer); returns (rc, out, valid, the arrays behind the pointers)."""
    L = tiffcodec._lib()
    src = np.arange(6 * 29 * 61, dtype=np.int16).reshape(6, 29, 61)
    xo, yo = sf.offsets(src, sf.source_gt(-5, 3))
    n = 64
    out = np.full(2 * n + 8, 0x5A5A, np.uint16)
    valid = np.full(n, sf.CANARY, np.uint8)
    sel = kw.pop('sel', [1, 0])
    sel_a = np.array(sel if sel is not None else [0], np.int32)
    a = dict(src=src.ctypes.data, bps=2, src_bands=6, src_h=29, src_w=61, xoff=xo.ctypes.data,
             yoff=yo.ctypes.data, grid_w=sf.W, grid_h=sf.H, p0=10, n=n, n_sel=len(sel_a),
             sel=sel_a.ctypes.data if sel is not None else None, out=out.ctypes.data,
             out_stride=n, valid=valid.ctypes.data, mode=0, threads=2)
    for key, v in kw.items():
        a[key] = a[key] + 1 if v == 'misaligned' else v
    vp = ctypes.c_void_p
    rc = L.lt_grid_sample(vp(a['src']), a['bps'], a['src_bands'], a['src_h'], a['src_w'],
                          vp(a['xoff']), vp(a['yoff']), a['grid_w'], a['grid_h'], a['p0'], a['n'],
                          a['n_sel'], vp(a['sel']), vp(a['out']), a['out_stride'],
                          vp(a['valid']), a['mode'], a['threads'])
    return rc, out, valid, (src, xo, yo)


BAD_ARGS = [dict(bps=3), dict(bps=0), dict(bps=16), dict(mode=2), dict(mode=-1), dict(n_sel=0),
            dict(n_sel=17), dict(sel=[6, 0]), dict(sel=[0, -1]), dict(src_h=-1), dict(src_w=-1),
            dict(grid_w=-1), dict(grid_h=-1), dict(p0=-1), dict(n=-1), dict(out_stride=-1),
            dict(out_stride=63), dict(p0=sf.P - 63), dict(n=sf.P), dict(src_bands=0),
            dict(src_h=1 << 31), dict(grid_w=1 << 31), dict(src=None), dict(out=None),
            dict(valid=None), dict(xoff=None), dict(yoff=None), dict(sel=None),
            dict(src='misaligned'), dict(out='misaligned')]


@pytest.mark.parametrize('bad', BAD_ARGS, ids=[str(b) for b in BAD_ARGS])
def test_host_build_rejects(bad):
    rc, out, valid, _ = _raw_call(**bad)
    assert rc == -1  # LT_IO_ERR_ARG
    assert (out == 0x5A5A).all() and (valid == sf.CANARY).all()  # nothing written


def test_good_raw_call_writes():
    rc, out, valid, (src, xo, yo) = _raw_call()
    assert rc == 0 and (out[128:] == 0x5A5A).all()
    want, wv = sf.numpy_bands(src, sf.source_gt(-5, 3), 10, 74, [1, 0])
    assert np.array_equal(out[:128].view(np.int16).reshape(2, 64), want)
    assert np.array_equal(valid, wv)


def test_core_standalone_under_sanitizers(tmp_path):
    """The sampling core and its threaded host build in a program of their own (its own main),
    compiled with AddressSanitizer and UBSan and run as a child process over the shapes of this
    corpus: nothing is preloaded, nothing sanitized is loaded into Python."""
    src = os.path.join(ROOT, 'tests', 'native', 'grid_sample_check.cpp')
    io = os.path.join(ROOT, 'land_trendr_amd', 'csrc', 'lt_io.cpp')
    exe = str(tmp_path / 'grid_sample_check')
    base = ['g++', '-O1', '-g', '-std=c++17', '-pthread', '-fsanitize=address,undefined',
            '-fno-sanitize-recover=all', '-o', exe, src, io]
    errs = []
    for extra in (['-static-libasan', '-static-libubsan'], ['-static-libasan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
        errs.append(r.stderr)
    assert r.returncode == 0, '\n'.join(errs)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith('ok '), r.stdout
