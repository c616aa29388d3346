"""The lazy DP's trackers seeded from the column's 1- and 2-point starts (lt_fast.h column:
LT_DP_SEED): the best inexact start of points j and j-1, the group, is assigned to the interval
trackers before the starts of >= 3 points are priced, not merged into them after the last one; a
zero-residual start that becomes the group's new best replaces the group's entry. Every output
plane of every pixel of 64 waves, deferred pixels included, against the oracle (oracle/lt_oracle.c
prices every start with the emulated dgelsd residual), bit for bit, through the JIT kernels
specialised for the launch (index= the program): the only kernels that seed.

Test A: on exactly collinear series, where zero-residual starts replace the group's best in nearly
every column, the resolve stage receives as many pixels as with LT_DP_SEED=0 (the group entered at
the end of the column): the replaced entry leaves nothing behind in the trackers that would make
a decided column ambiguous."""
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
DIFF = 'B1 - B2'  # int16 series, a linear form


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
    """Keep a year, then skip 0-2 years: gaps of 1-3 between neighbours."""
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
    side in every wave), chosen at random: columns 0 and 1 seed from one and two starts and price
    nothing else."""
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
    alternate between them)."""
    rng = np.random.default_rng(seed)
    _, v, _ = _synth(30, seed)
    ext = np.where(rng.random(v.shape) < 0.5, 32767, -32767)
    v = np.where(rng.random(v.shape) < 0.33, ext, v)
    v[:, :64] = np.where((np.arange(30)[:, None] + np.arange(64)[None, :] // 32) % 2, 32767, -32767)
    return _dates(30), v, None


CASES = {  # name: (series, line cost, output fields)
    'c2': (lambda: _synth(30, 3000), 10.0, LABELS),
    'gaps': (lambda: _gaps(41), 10.0, LABELS),
    'short_mixed': (lambda: _short(42), 10.0, LABELS),
    'collinear_cost10': (lambda: _collinear(43), 10.0, LABELS),
    'collinear_cost1e-4': (lambda: _collinear(43), 1e-4, LABELS),
    'extremes': (lambda: _extremes(44), 10.0, LABELS),
    'years40_cost1': (lambda: _synth(40, 45), 1.0, LABELS),
    'trendline4': (lambda: _synth(30, 47), 10.0, LABELS + TREND4),
}
_want = {}  # the oracle's planes per case, computed once


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)
    yield e
    e.close()


def _case(name):
    from oracle import index_oracle, oracle
    series, cost, fields = CASES[name]
    if name not in _want:
        dates, v, valid = series()
        assert np.abs(v).max() <= 32767
        meta = build_scene(dates, parse_date('2014-07-01'))
        params, _ = compile_params(cost, GD)
        rng = np.random.default_rng(5)
        b2 = rng.integers(100, 401, v.shape)
        b2 = np.where(np.abs(v + b2) < 32768, b2, 0)
        bands = np.stack([v + b2, b2], axis=1).astype(np.int16)  # [K, 2, P]
        prog = index_eqn.IndexProgram(DIFF, band_dtype='int16')
        vals = index_oracle.evaluate(prog, np.moveaxis(bands, 1, 0)).astype(np.float64)
        assert (vals == v).all()
        want = oracle.analyze_tile(meta, params, np.ascontiguousarray(vals), valid,
                                   n_threads=min(os.cpu_count() or 1, 16))
        _want[name] = (meta, params, bands, valid, want, prog)
    return _want[name] + (fields,)


def _run(eng, name):
    """The case through the JIT analyze / resolve kernels: the output planes and the number of
    pixels the analyze stage handed to the resolve stage."""
    meta, params, bands, valid, want, prog, fields = _case(name)
    fn = eng.compile_index(prog)
    K = bands.shape[0]
    inter = torch.empty((K, P, 2), dtype=torch.int16, device=eng.device).permute(0, 2, 1)
    inter.copy_(torch.from_numpy(bands))
    vb = None if valid is None else pack_valid_bits(torch.from_numpy(valid).to(eng.device))
    before = eng.jit_stats()
    got = eng.analyze_tile(meta, params, inter, vb, fields, index=fn)
    torch.cuda.synchronize()
    after = eng.jit_stats()
    assert after['jit_tiles'] == before['jit_tiles'] + 1, after
    return got, eng.last_deferred()


def _check(name, got):
    _, _, _, _, want, _, fields = _case(name)
    status = got['status'].cpu().numpy()
    assert ((status & 16) == 0).all(), int(((status & 16) != 0).sum())
    for f in fields:
        g = got[f].cpu().numpy()
        w = want[f][:g.shape[0]] if g.ndim == 2 else want[f]
        assert g.shape[-1] == P and w.shape == g.shape, (f, g.shape, w.shape)
        same = _bits_equal(w, g)
        assert same.all(), (name, f, int((~same).sum()))


@pytest.mark.parametrize('name', list(CASES))
def test_every_plane_matches_the_oracle(eng, name):
    got, _ = _run(eng, name)
    _check(name, got)


@pytest.mark.parametrize('name', ['collinear_cost10', 'collinear_cost1e-4'])
def test_a_deferred_pixels_equal_the_unseeded_order(eng, name, monkeypatch):
    """LT_JIT_DEFINES is part of the module key (lt_jit.h env_switches), so one context compiles
    and runs both orders."""
    monkeypatch.delenv('LT_JIT_DEFINES', raising=False)
    got1, d1 = _run(eng, name)
    monkeypatch.setenv('LT_JIT_DEFINES', 'LT_DP_SEED=0')
    s0 = eng.jit_stats()
    got0, d0 = _run(eng, name)
    s1 = eng.jit_stats()
    print('%s: deferred %d seeded, %d with LT_DP_SEED=0' % (name, d1, d0))
    # the switch reached the kernels: its launch took a module of its own (built or read back)
    assert s1['compiles'] + s1['disk_hits'] > s0['compiles'] + s0['disk_hits'], (s0, s1)
    _check(name, got0)
    _check(name, got1)
    assert d1 == d0, (name, d1, d0)
