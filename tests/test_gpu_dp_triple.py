"""The lazy DP's first start of >= 3 points priced as a triple (lt_pixel.h dp_triple_sse,
lt_fast.h column: LT_DP_TRIPLE): the closed-form residual of the three window points without
running sums, its zero test on the numerator alone, and the sums built only when a wave goes on to
a second start. Every output plane of every pixel of 64 waves, deferred pixels included, against
the oracle (oracle/lt_oracle.c prices every start with the emulated dgelsd residual), bit for bit:
through the JIT kernels specialised for the launch (index= the program), which price the triple
that way, and through the precompiled kernels (the program's linear form or its index raster),
which price it from the sums."""
import os

import numpy as np
import pytest
import torch

from land_trendr_amd import index_eqn
from land_trendr_amd.engine import Engine, pack_valid_bits
from land_trendr_amd.scene import build_scene, parse_date
from land_trendr_amd.settings import compile_params
from land_trendr_amd.synth import make_scene

pytestmark = pytest.mark.gpu
P = 4096  # 64 waves
LABELS = ('status', 'matched', 'class_val', 'onset_year', 'duration', 'magnitude')
TREND4 = ('val_fit', 'fit_m', 'fit_b', 'vertex')
GD = [{'name': 'gd', 'val': 1, 'change_type': 'GD'}]
DIFF = ('B1 - B2', None)               # int16 series, a linear form
SCALED = ('(B1 - B2) * 0.3', 'float32')  # a binary32 series of non-integer values


def _bits_equal(a, b):
    if a.dtype.kind == 'f':
        return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def _dates(years):
    # one date list per year count, so the cases of one year count, cost and mask share a kernel
    return make_scene(64, n_years=years, seed=1000).dates


def _synth(years, seed):
    sc = make_scene(P, n_years=years, seed=seed)
    return _dates(years), sc.values.numpy().astype(np.int64), None


def _gap_mask(rng, Y):
    """Keep a year, then skip 0-2 years: gaps of 1-3 between neighbours, so d1 != d2 is common."""
    valid = np.zeros((Y, P), np.uint8)
    k = rng.integers(0, 3, P)
    while (k < Y).any():
        on = np.nonzero(k < Y)[0]
        valid[k[on], on] = 1
        k = k + rng.integers(1, 4, P)
    return valid


def _gaps(seed):
    _, v, _ = _synth(30, seed)
    return _dates(30), v, _gap_mask(np.random.default_rng(seed), 30)


def _short(seed):
    """c2-like values; pixel p keeps exactly 1 + p % 4 of its years (1, 2, 3 and 4 points side by
    side in every wave), chosen at random: columns 0 and 1 price no triple, column 2 only it."""
    rng = np.random.default_rng(seed)
    _, v, _ = _synth(30, seed)
    keep = 1 + np.arange(P) % 4
    rank = np.argsort(np.argsort(rng.random((30, P)), axis=0), axis=0)
    return _dates(30), v, (rank < keep[None, :]).astype(np.uint8)


def _collinear(seed):
    """Plateaus and runs of integer slope (3-9 years each, joined by jumps) under the gap mask: the
    value is linear in the year within a run, so every triple inside one is exactly collinear at
    any gaps. A quarter of the pixels have small values (the zero path's condition on Syy holds
    at the small line cost as well), the rest values around 1000-3000."""
    rng = np.random.default_rng(seed)
    Y = 30
    v = np.zeros((Y, P), np.int64)
    level = np.where(np.arange(P) % 4 == 0, rng.integers(-8, 9, P), rng.integers(1000, 3000, P))
    slope = np.zeros(P, np.int64)
    left = np.zeros(P, np.int64)
    for t in range(Y):
        new = left == 0
        jump = np.where(np.arange(P) % 4 == 0, rng.integers(-6, 7, P), rng.integers(-300, 301, P))
        level = np.where(new & (t > 0), level + jump, level)
        slope = np.where(new, np.where(rng.random(P) < 0.4, 0, rng.integers(-20, 21, P)), slope)
        left = np.where(new, rng.integers(3, 10, P), left)
        v[t] = level
        level = level + slope
        left = left - 1
    return _dates(Y), v, _gap_mask(rng, Y)


def _extremes(seed):
    """c2-like series with a third of the values replaced by +-32767 (and a few pixels that
    alternate between them): the largest differences and numerators an int16 series has."""
    rng = np.random.default_rng(seed)
    _, v, _ = _synth(30, seed)
    ext = np.where(rng.random(v.shape) < 0.5, 32767, -32767)
    v = np.where(rng.random(v.shape) < 0.33, ext, v)
    v[:, :64] = np.where((np.arange(30)[:, None] + np.arange(64)[None, :] // 32) % 2, 32767, -32767)
    return _dates(30), v, None


CASES = {  # name: (series, line cost, output fields, program)
    'c2': (lambda: _synth(30, 2000), 10.0, LABELS, DIFF),
    'gaps': (lambda: _gaps(21), 10.0, LABELS, DIFF),
    'short_mixed': (lambda: _short(22), 10.0, LABELS, DIFF),
    'collinear_cost10': (lambda: _collinear(23), 10.0, LABELS, DIFF),
    'collinear_cost1e-4': (lambda: _collinear(23), 1e-4, LABELS, DIFF),
    'extremes': (lambda: _extremes(24), 10.0, LABELS, DIFF),
    'years40_cost1': (lambda: _synth(40, 25), 1.0, LABELS, DIFF),
    'float32_series': (lambda: _gaps(26), 10.0, LABELS, SCALED),
    'trendline4': (lambda: _synth(30, 27), 10.0, LABELS + TREND4, DIFF),
}
_want = {}  # the oracle's planes per case, computed once for both paths


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)
    yield e
    e.close()


def _case(name):
    from oracle import index_oracle, oracle
    series, cost, fields, (eqn, out) = CASES[name]
    if name not in _want:
        dates, v, valid = series()
        assert np.abs(v).max() <= 32767
        meta = build_scene(dates, parse_date('2014-07-01'))
        params, _ = compile_params(cost, GD)
        rng = np.random.default_rng(5)
        b2 = rng.integers(100, 401, v.shape)
        b2 = np.where(np.abs(v + b2) < 32768, b2, 0)
        bands = np.stack([v + b2, b2], axis=1).astype(np.int16)  # [K, 2, P]
        prog = index_eqn.IndexProgram(eqn, band_dtype='int16', out_dtype=out)
        vals = index_oracle.evaluate(prog, np.moveaxis(bands, 1, 0)).astype(np.float64)
        if out is None:
            assert (vals == v).all()
        else:
            assert (vals != np.rint(vals)).mean() > 0.5  # not an integer series
        want = oracle.analyze_tile(meta, params, np.ascontiguousarray(vals), valid,
                                   n_threads=min(os.cpu_count() or 1, 16))
        _want[name] = (meta, params, bands, valid, want, prog)
    return _want[name] + (fields,)


@pytest.mark.parametrize('path', ['jit', 'precompiled'])
@pytest.mark.parametrize('name', list(CASES))
def test_every_plane_matches_the_oracle(eng, name, path):
    meta, params, bands, valid, want, prog, fields = _case(name)
    fn = eng.compile_index(prog)
    K = bands.shape[0]
    inter = torch.empty((K, P, 2), dtype=torch.int16, device=eng.device).permute(0, 2, 1)
    inter.copy_(torch.from_numpy(bands))
    vb = None if valid is None else pack_valid_bits(torch.from_numpy(valid).to(eng.device))
    before = eng.jit_stats()
    if path == 'jit':
        got = eng.analyze_tile(meta, params, inter, vb, fields, index=fn)
    elif fn.lin is not None:
        got = eng.analyze_tile(meta, params, inter, vb, fields, lin=fn.lin)
    else:  # not a linear form: the precompiled kernels read the program's index raster
        got = eng.analyze_tile(meta, params, eng.index_tile(fn, inter), vb, fields)
    torch.cuda.synchronize()
    after = eng.jit_stats()
    if path == 'jit':
        assert after['jit_tiles'] == before['jit_tiles'] + 1, after
    else:
        assert after['jit_tiles'] == before['jit_tiles'], after
    status = got['status'].cpu().numpy()
    assert ((status & 16) == 0).all(), int(((status & 16) != 0).sum())
    for f in fields:
        g = got[f].cpu().numpy()
        w = want[f][:g.shape[0]] if g.ndim == 2 else want[f]
        assert g.shape[-1] == P and w.shape == g.shape, (f, g.shape, w.shape)
        same = _bits_equal(w, g)
        assert same.all(), (name, path, f, int((~same).sum()))
