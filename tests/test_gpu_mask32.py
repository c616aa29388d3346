"""The per-pixel point masks held in 32 bits (lt_bits.h PointBits, LT_MASK32) in the instances of
at most 32 years: every output plane of every pixel, deferred pixels included, bit for bit against
the oracle (oracle/lt_oracle.c), through the JIT kernels specialised for the launch (index= the
program) and through the precompiled kernels (the switch of test_gpu_jit.py: LT_SRC_DIR names an
empty directory, every JIT compile fails and the tiles run on the library's own instances).

All scenes but the control have 32 years, the largest count the 32-bit masks serve, so bit 31 of
every mask is in use:
  full32            one observation per year, no mask: the lanes reach T = n = 32 (n < 32 where a
                    point is a spike); GD rule, line cost 10: the certified labels path
  full32_trendline  the same scene with every per-year plane: the year-major path
  full32_compact    the same through the compact trendline (a context created with LT_TL_SPLIT=1)
  c3_rules          1-4 observations per year, mask probability 0.2, the three rules of bench.py's
                    c3 in documented mode
  ties_cost1e-4     the tie sets of test_gpu_parity.py at line cost 1e-4: the lazy DP defers a third
                    of the pixels, so the resolve kernel's exact DP (its cand masks) decides them.
                    Seed 4242 was picked with the host model (tools/defer_diag.py's calls:
                    analyze_pixel and dp_lazy of lt_pixel.h compiled for the host), which defers
                    675 of these 2,048 pixels (33 %, the bar was 1 %)
  handmade          a spike at point 30 of 32; a flat series with two steps so that points 30 and
                    31 are vertices; a series with only the first and the last year present; each
                    at 341 levels side by side in the waves
  years33           the control: 33 years, the MAXY = 48 instances, 64-bit masks
LT_MASK32=0 (LT_JIT_DEFINES) against the default on the 32-year scenes: identical planes and equal
deferred counts."""
import datetime as dt
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
P = 2048  # 32 waves
LABELS = ('status', 'n_years', 'matched', 'class_val', 'onset_year', 'duration', 'magnitude')
TRENDLINE = ('winner', 'val_raw', 'val_fit', 'fit_m', 'fit_b', 'right_m', 'right_b', 'spike',
             'vertex')
GD = [{'name': 'gd', 'val': 1, 'change_type': 'GD'}]
C3_RULES = [{'name': 'fd', 'val': 2, 'change_type': 'FD', 'onset_year': ['>=', 1995],
             'duration': ['<', 4]},
            {'name': 'gd', 'val': 3, 'change_type': 'GD', 'pre_threshold': ['>', 500]},
            {'name': 'ld', 'val': 4, 'change_type': 'LD', 'duration': ['>', 2]}]
DIFF = 'B1 - B2'  # int16 series, a linear form


def _bits_equal(a, b):
    if a.dtype.kind == 'f':
        return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def _synth(years, seed, **kw):
    sc = make_scene(P, n_years=years, seed=seed, **kw)
    return (sc.dates, sc.values.numpy().astype(np.int64),
            None if sc.valid is None else sc.valid.numpy().astype(np.uint8))


def _yearly(years):
    return [dt.date(1985 + t, 7, 1) for t in range(years)]


def _ties(seed):
    """test_gpu_parity.py's tie-heavy small integers: multiples of 100, random walks of steps
    -1..1, and short periods of multiples of 7."""
    rng = np.random.default_rng(seed)
    T = 32
    kind = rng.integers(0, 3, P)
    v = np.where(kind[None, :] == 0, rng.integers(0, 4, (T, P)) * 100,
                 np.where(kind[None, :] == 1, np.cumsum(rng.integers(-1, 2, (T, P)), 0),
                          (np.arange(T)[:, None] % rng.integers(2, 5, P)[None, :]) * 7))
    return _yearly(T), v.astype(np.int64), None


def _handmade():
    T = 32
    t = np.arange(T)[:, None]
    p = np.arange(P)[None, :]
    level = 500 + 3 * (p // 3)
    wiggle = ((t * 7 + p) % 5) - 2  # small, never monotone for long
    spike30 = level + wiggle + np.where(t == 30, 1500, 0)
    # (300 then 200 down: points 29..31 are not collinear, so the last segment starts at 30)
    steps = np.where(t < 30, level, np.where(t == 30, level - 300, level - 500))
    ends = level + 10 * t
    v = np.where(p % 3 == 0, spike30, np.where(p % 3 == 1, steps, ends))
    valid = np.ones((T, P), np.uint8)
    valid[1:T - 1, (np.arange(P) % 3) == 2] = 0  # only the first and the last year
    return _yearly(T), v.astype(np.int64), valid


CASES = {  # name: (series, line cost, rules, mode, output fields)
    'full32': (lambda: _synth(32, 3200), 10.0, GD, 'reference', LABELS),
    'full32_trendline': (lambda: _synth(32, 3200), 10.0, GD, 'reference', LABELS + TRENDLINE),
    'c3_rules': (lambda: _synth(32, 3201, k_min=1, k_max=4, mask_prob=0.2), 10.0, C3_RULES,
                 'documented', LABELS),
    'ties_cost1e-4': (lambda: _ties(4242), 1e-4, GD, 'reference', LABELS),
    'handmade': (_handmade, 10.0, GD, 'reference', LABELS + ('val_fit', 'spike', 'vertex')),
    'years33': (lambda: _synth(33, 3300), 10.0, GD, 'reference', LABELS),
}
YEARS32 = [n for n in CASES if n != 'years33']
_want = {}  # the oracle's planes per case, computed once


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def eng_pre():
    """A context of its own for the precompiled runs: no JIT module of another test in its map."""
    e = Engine(0)
    yield e
    e.close()


def _case(name):
    from oracle import index_oracle, oracle
    series, cost, rules, mode, fields = CASES[name]
    if name not in _want:
        dates, v, valid = series()
        assert v.shape[1] == P and np.abs(v).max() <= 32767
        meta = build_scene(dates, parse_date('2014-07-01'))
        params, _ = compile_params(cost, rules, mode)
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


def _run(eng, name, jit=True):
    """The case through the JIT kernels (jit) or, with every JIT compile failing, through the
    precompiled ones: the output planes and the number of pixels handed to the resolve stage."""
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
    key = 'jit_tiles' if jit else 'fallback_tiles'
    assert after[key] == before[key] + 1, (before, after)
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


def _check_deferred(name, deferred):
    print('%s: %d of %d pixels deferred' % (name, deferred, P))
    if name == 'ties_cost1e-4':  # the resolve kernel's cand masks ran
        assert deferred > 0, deferred


def test_the_scenes_reach_the_last_bit():
    """What the cases are for: lanes with all 32 years present and no spike (T = n = 32), a spike
    at point 30, vertices at points 30 and 31, and a pixel of two points 31 years apart."""
    _, _, _, _, want, _, _ = _case('full32_trendline')
    pres = ~np.isnan(want['val_raw'])
    assert pres.all() and want['val_raw'].shape[0] == 32
    assert (want['spike'].sum(0) == 0).sum() >= P // 8  # n = 32 in many lanes
    assert (want['vertex'][31] == 1).all()
    _, _, _, _, want, _, _ = _case('handmade')
    p = np.arange(P)
    assert (want['spike'][30, p % 3 == 0] == 1).all()
    assert (want['vertex'][30, p % 3 == 1] == 1).all() and (want['vertex'][31, p % 3 == 1] == 1).all()
    assert (want['n_years'][p % 3 == 2] == 2).all()
    assert (want['vertex'][:, p % 3 == 2].sum(0) == 2).all()


@pytest.mark.parametrize('name', list(CASES))
def test_jit_kernels_match_the_oracle(eng, name):
    got, deferred = _run(eng, name)
    _check(name, got)
    _check_deferred(name, deferred)


@pytest.mark.parametrize('name', list(CASES))
def test_precompiled_kernels_match_the_oracle(eng_pre, name, tmp_path, monkeypatch):
    monkeypatch.setenv('LT_SRC_DIR', str(tmp_path))  # no kernel headers: no JIT module
    got, deferred = _run(eng_pre, name, jit=False)
    st = eng_pre.jit_stats()
    assert st['jit_tiles'] == 0 and 'not found' in st['last_error'], st
    _check(name, got)
    _check_deferred(name, deferred)


def test_compact_trendline_matches_the_oracle(monkeypatch):
    """The per-year planes through the compact trendline (tl_bits: the masks widened at the
    store) and the expand kernel."""
    monkeypatch.setenv('LT_TL_SPLIT', '1')
    e = Engine(0)
    try:
        got, _ = _run(e, 'full32_trendline')
        _check('full32_trendline', got)
    finally:
        e.close()


@pytest.mark.parametrize('name', YEARS32)
def test_mask32_off_gives_the_same_planes_and_deferred_count(eng, name, monkeypatch):
    """LT_JIT_DEFINES is part of the module key (lt_jit.h env_switches), so one context compiles
    and runs both widths."""
    monkeypatch.delenv('LT_JIT_DEFINES', raising=False)
    got1, d1 = _run(eng, name)
    monkeypatch.setenv('LT_JIT_DEFINES', 'LT_MASK32=0')
    s0 = eng.jit_stats()
    got0, d0 = _run(eng, name)
    s1 = eng.jit_stats()
    print('%s: deferred %d with 32-bit masks, %d with LT_MASK32=0' % (name, d1, d0))
    # the switch reached the kernels: its launch took a module of its own (built or read back)
    assert s1['compiles'] + s1['disk_hits'] > s0['compiles'] + s0['disk_hits'], (s0, s1)
    _check(name, got0)
    _, _, _, _, _, _, fields = _case(name)
    for f in fields:
        assert _bits_equal(got0[f].cpu().numpy(), got1[f].cpu().numpy()).all(), (name, f)
    assert d1 == d0, (name, d1, d0)
