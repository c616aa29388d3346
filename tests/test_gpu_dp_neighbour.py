"""The lazy DP's exit test with the residuals of neighbouring triples (lt_pixel.h
dp_start_bound_nb, lt_fast.h column): a column may end earlier, and a start it no longer prices
must never have been the column's first minimum. Every output plane of every pixel of 64 waves,
deferred pixels included, against the oracle (oracle/lt_oracle.c prices every start, as
segmented_least_squares does), bit for bit: through the JIT
kernels specialised for the launch (index= the program 'B1 - B2'), which use the new exit, and
through the precompiled kernels (the program's linear form, what LT_JIT_INDEX=0 makes the runner
pass), which keep the plain one."""
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


def _bits_equal(a, b):
    if a.dtype.kind == 'f':
        return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def _synth(years, seed, spike_prob=0.05):
    sc = make_scene(P, n_years=years, seed=seed, spike_prob=spike_prob)
    return sc.dates, sc.values.numpy().astype(np.int64), None


def _smooth(seed):
    """Piecewise-linear series (2-4 pieces, slopes up to +-60 per year) with noise of +-2, and a
    mask that leaves year gaps of 1-3: long segments win here, so deep starts must still be
    priced."""
    rng = np.random.default_rng(seed)
    Y = 30
    dates, _, _ = _synth(Y, seed)
    t = np.arange(Y)[:, None]
    v = rng.integers(500, 3000, (1, P)).astype(np.float64) * np.ones((Y, 1))
    for _ in range(3):
        brk = rng.integers(2, Y - 2, (1, P))
        v = v + rng.integers(-60, 61, (1, P)) * np.maximum(t - brk, 0)
    v = np.rint(v).astype(np.int64) + rng.integers(-2, 3, (Y, P))
    valid = np.zeros((Y, P), np.uint8)
    k = np.zeros(P, np.int64)
    while (k < Y).any():  # keep year k, then skip 0-2 years
        on = np.nonzero(k < Y)[0]
        valid[k[on], on] = 1
        k = k + rng.integers(1, 4, P)
    return dates, v, valid


def _mixed(seed):
    """c2-like values; pixel p keeps 2 + p % 29 of its 30 years (2..30 points), chosen at random:
    every wave holds series of every length."""
    rng = np.random.default_rng(seed)
    dates, v, _ = _synth(30, seed)
    keep = 2 + np.arange(P) % 29
    order = np.argsort(rng.random((30, P)), axis=0)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(30)[:, None] * np.ones((1, P), np.int64), axis=0)
    return dates, v, (rank < keep[None, :]).astype(np.uint8)


CASES = {  # name: (series, line cost, output fields)
    'c2': (lambda: _synth(30, 1000), 10.0, LABELS),
    'smooth_cost1': (lambda: _smooth(11), 1.0, LABELS),
    'smooth_cost10': (lambda: _smooth(11), 10.0, LABELS),
    'spikes': (lambda: _synth(30, 12, spike_prob=0.3), 10.0, LABELS),
    'mixed_lengths': (lambda: _mixed(13), 10.0, LABELS),
    'years40_cost1': (lambda: _synth(40, 14), 1.0, LABELS),
    'trendline4': (lambda: _synth(30, 15), 10.0, LABELS + TREND4),
}
_want = {}  # the oracle's planes per case, computed once for both paths


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)
    yield e
    e.close()


def _case(name):
    from oracle import oracle
    series, cost, fields = CASES[name]
    if name not in _want:
        dates, v, valid = series()
        meta = build_scene(dates, parse_date('2014-07-01'))
        params, _ = compile_params(cost, GD)
        want = oracle.analyze_tile(meta, params, v.astype(np.float64), valid,
                                   n_threads=min(os.cpu_count() or 1, 16))
        rng = np.random.default_rng(5)
        b2 = rng.integers(100, 401, v.shape)
        assert np.abs(v + b2).max() < 32768
        bands = np.stack([v + b2, b2], axis=1).astype(np.int16)  # [K, 2, P]
        _want[name] = (meta, params, bands, valid, want)
    return _want[name] + (fields,)


@pytest.mark.parametrize('path', ['jit', 'precompiled'])
@pytest.mark.parametrize('name', list(CASES))
def test_every_plane_matches_the_oracle(eng, name, path):
    meta, params, bands, valid, want, fields = _case(name)
    fn = eng.compile_index(index_eqn.IndexProgram('B1 - B2', band_dtype='int16'))
    K = bands.shape[0]
    inter = torch.empty((K, P, 2), dtype=torch.int16, device=eng.device).permute(0, 2, 1)
    inter.copy_(torch.from_numpy(bands))
    vb = None if valid is None else pack_valid_bits(torch.from_numpy(valid).to(eng.device))
    before = eng.jit_stats()
    kw = dict(index=fn) if path == 'jit' else dict(lin=fn.lin)
    got = eng.analyze_tile(meta, params, inter, vb, fields, **kw)
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
