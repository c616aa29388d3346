"""The certified labels path's trimmed pass A (lt_fast.h LT_FIT_TRIM: the vertex loop unrolled by
two over alternating state, 1/m from an LDS table, an integer |y| maximum, the vertex's point taken
from its segment's sums) in the one-rule labels-only JIT kernels, the only kernels that take it.

Tiles of 1,024 pixels (16 waves) x 30 years of int16 with bench's c2 field set and one GD rule.
Every case is compared plane by plane, bit for bit, with the oracle, and byte for byte with the same
launch compiled with LT_FIT_TRIM=0 (LT_JIT_DEFINES), deferral counts included. What each case is
meant to contain (vertex counts, segment lengths, year gaps) is computed from the oracle's planes
alone, asserted, and printed with a failing comparison."""
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
P = 1024  # 16 waves
Y = 30
LABELS = ('status', 'matched', 'class_val', 'onset_year', 'duration', 'magnitude')
GD = [{'name': 'gd', 'val': 1, 'change_type': 'GD'}]
DIFF = 'B1 - B2'  # int16 series, a linear form
OFF = 'LT_FIT_TRIM=0'


def _bits_equal(a, b):
    if a.dtype.kind == 'f':
        return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def _dates30():
    # one date list for the cases on consecutive years, so equal costs and masks share a kernel
    return make_scene(64, n_years=Y, seed=1000).dates


def _dates_by_gaps(gaps):
    years = 2014 - int(np.sum(gaps)) + np.concatenate([[0], np.cumsum(gaps)])
    return [dt.date(int(y), 7, 1) for y in years]


def _noise(seed):
    return make_scene(P, n_years=Y, seed=seed).values.numpy().astype(np.int64)


def _c2(seed):
    return _dates30(), _noise(seed), None


def _short_mixed(seed):
    """Even waves: every fourth pixel its full series, the others 1, 2 or 3 valid years; odd waves:
    1, 2 and 3 valid years only (the wave's largest vertex count is then small and, with 3-point
    series that keep their middle point as a vertex, odd)."""
    rng = np.random.default_rng(seed)
    v = _noise(seed)
    # 3 points on a sharp bend keep the middle vertex at line cost 10
    p = np.arange(P)
    keep = np.where(p % 4 == 0, Y, p % 4)
    keep = np.where((p // 64) % 2 == 1, 1 + p % 3, keep)
    rank = np.argsort(np.argsort(rng.random((Y, P)), axis=0), axis=0)
    return _dates30(), v, (rank < keep[None, :]).astype(np.uint8)


GAPS_D = np.array([2, 1, 3, 1, 1, 6, 1, 2, 1, 4, 1, 1, 5, 1, 2, 1, 3, 1, 1, 6, 1, 2, 1, 4, 1, 1,
                   2, 1, 5])


def _gap_scene(seed):
    """Calendar years 1-6 apart (span below 64): segments over small and large year gaps, and
    larger ones where despike dropped the point between, in one wave."""
    assert len(GAPS_D) == Y - 1 and GAPS_D.sum() <= 63
    return _dates_by_gaps(GAPS_D), _noise(seed), None


def _wide_scene(seed):
    """Calendar years 1-8 apart, the span past 63 year offsets (kFitWide, kZeroWide)."""
    rng = np.random.default_rng(seed)
    gaps = rng.integers(1, 9, Y - 1)
    assert 64 <= gaps.sum() <= 255
    return _dates_by_gaps(gaps), _noise(seed), None


def _steps(seed):
    """Noise-free plateaus and integer slopes with two drops of one magnitude: exactly collinear
    runs (zero residuals, n3 == 0), equal candidates of the GD rule, vertices whose left and right
    eqn give the same value."""
    rng = np.random.default_rng(seed)
    t = np.arange(Y)[:, None]
    t1 = rng.integers(4, 12, P)[None, :]
    t2 = t1 + rng.integers(4, 12, P)[None, :]
    mag = rng.integers(50, 2000, P)[None, :]
    slope = np.where(np.arange(P) % 3 == 0, rng.integers(-9, 10, P), 0)[None, :]
    v = 5000 + slope * t - mag * (t >= t1) - mag * (t >= t2)
    return _dates30(), v.astype(np.int64), None


CASES = {  # name: (series, line cost)
    'a_noise_cost10': (lambda: _c2(5000), 10.0),
    'b_cost1e3': (lambda: _c2(5000), 1e3),
    'b_cost1e9': (lambda: _c2(5000), 1e9),
    'c_short_mixed': (lambda: _short_mixed(5002), 10.0),
    'd_gap_scene': (lambda: _gap_scene(5003), 10.0),
    # (costs of their own below: a context holds few scene-specialised modules and then shares
    # one generic-scene module per configuration, and every case is to build its two modules)
    'e_wide_scene': (lambda: _wide_scene(5004), 12.0),
    'f_steps': (lambda: _steps(5005), 20.0),
}
_want = {}  # per case: the launch's inputs, the oracle's planes and the shape statistics, once


def _shape(meta_years, want, valid):
    """From the oracle's planes alone: per pixel the vertex count and the segment lengths in
    points, per wave the largest vertex count; the year gaps of neighbouring non-spike points."""
    vertex = np.asarray(want['vertex'])[:Y] != 0
    spike = np.asarray(want['spike'])[:Y] != 0
    present = np.ones((Y, P), bool) if valid is None else valid != 0
    point = present & ~spike
    nv = vertex.sum(0)
    seg, gaps = [], []
    years = np.asarray(meta_years)
    for p in range(P):
        ks = np.nonzero(point[:, p])[0]
        vi = np.nonzero(vertex[ks, p])[0]  # vertices as point indices
        seg.append(np.diff(vi) + 1)
        gaps.append(np.diff(years[ks]))
    return nv, seg, gaps, nv.reshape(-1, 64).max(1)


def _summary(name):
    nv, seg, gaps, nvmax = _want[name][6]
    allseg = np.concatenate(seg) if len(seg) else np.zeros(0, int)
    allgap = np.concatenate(gaps)
    return ('%s: nv %d-%d (odd %d, even %d), wave nvmax %s, segment points %s, year gaps %s'
            % (name, nv.min(), nv.max(), int((nv % 2 == 1).sum()), int((nv % 2 == 0).sum()),
               sorted(set(nvmax.tolist())),
               dict(zip(*[a.tolist() for a in np.unique(allseg, return_counts=True)])),
               dict(zip(*[a.tolist() for a in np.unique(allgap, return_counts=True)]))))


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)
    yield e
    e.close()


def _case(name):
    from oracle import index_oracle, oracle
    series, cost = CASES[name]
    if name not in _want:
        dates, v, valid = series()
        assert v.shape == (Y, P) and np.abs(v).max() <= 32767
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
        years = sorted({d.year for d in dates})
        _want[name] = (meta, params, bands, valid, want, prog, _shape(years, want, valid))
    return _want[name]


def _run(eng, name):
    """The case through the JIT analyze / resolve kernels: the output planes and the number of
    pixels the analyze stage handed to the resolve stage."""
    meta, params, bands, valid, want, prog, _ = _case(name)
    fn = eng.compile_index(prog)
    K = bands.shape[0]
    inter = torch.empty((K, P, 2), dtype=torch.int16, device=eng.device).permute(0, 2, 1)
    inter.copy_(torch.from_numpy(bands))
    vb = None if valid is None else pack_valid_bits(torch.from_numpy(valid).to(eng.device))
    before = eng.jit_stats()
    got = eng.analyze_tile(meta, params, inter, vb, LABELS, index=fn)
    torch.cuda.synchronize()
    after = eng.jit_stats()
    assert after['jit_tiles'] == before['jit_tiles'] + 1, after
    return {f: got[f].cpu().numpy() for f in LABELS}, eng.last_deferred()


def _check(name, got):
    want = _case(name)[4]
    status = got['status']
    assert ((status & 16) == 0).all(), int(((status & 16) != 0).sum())
    for f in LABELS:
        g = got[f]
        w = want[f][:g.shape[0]] if g.ndim == 2 else want[f]
        assert g.shape[-1] == P and w.shape == g.shape, (f, g.shape, w.shape)
        same = _bits_equal(w, g)
        assert same.all(), (f, int((~same).sum()), _summary(name))


def _expect_shape(name):
    """The case holds what it is meant to exercise (the oracle's planes only)."""
    nv, seg, gaps, nvmax = _case(name)[6]
    msg = _summary(name)
    print(msg)
    waves = [np.concatenate(seg[w * 64:(w + 1) * 64]) for w in range(P // 64)]
    wgaps = [np.concatenate(gaps[w * 64:(w + 1) * 64]) for w in range(P // 64)]
    if name == 'a_noise_cost10':
        # 3-point segments dominate; nv 10-16, odd and even in every wave
        allseg = np.concatenate(seg)
        assert (allseg == 3).mean() > 0.7 and nv.min() >= 8 and nv.max() <= 16, msg
        nvw = nv.reshape(-1, 64)
        assert ((nvw % 2 == 1).any(1) & (nvw % 2 == 0).any(1)).all(), msg
    elif name == 'b_cost1e3':
        # a segment of >= 5 points (the m > 4 tail) beside short ones in most waves
        assert np.mean([(s >= 5).any() and (s <= 4).any() for s in waves]) > 0.5, msg
    elif name == 'b_cost1e9':
        # single segments over the whole series: nv = 2
        assert (nv == 2).mean() > 0.9 and max(s.max() for s in waves) >= 25, msg
    elif name == 'c_short_mixed':
        # series of 1, 2 and 3 valid years (at most that many vertices; the oracle marks none in
        # a pixel it rejects) beside full series, and a wave whose largest vertex count is odd
        pts = (_case(name)[3] != 0).sum(0).reshape(-1, 64)
        assert all(((pts == k).any(1)).all() for k in (1, 2, 3)) and (pts == Y).any(1).any(), msg
        assert (nv == 2).any() and (nv == 3).any() and nv.max() >= 10, msg
        assert (nvmax % 2 == 1).any() and (nvmax % 2 == 0).any(), msg
    elif name == 'd_gap_scene':
        # gaps of 1..4 and larger ones in every wave
        assert all((g <= 4).any() and (g > 4).any() for g in wgaps), msg
    elif name == 'e_wide_scene':
        assert max(g.sum() for g in gaps) > 63, msg  # a pixel's points span > 63 offsets
    elif name == 'f_steps':
        # three runs: four to six vertices a pixel
        assert nv.min() >= 2 and nv.max() <= 8 and (nv >= 4).mean() > 0.5, msg


@pytest.mark.parametrize('name', list(CASES))
def test_planes_match_the_oracle_and_the_untrimmed_kernels(eng, name, monkeypatch):
    """LT_JIT_DEFINES is part of the module key (lt_jit.h env_switches), so one context compiles
    and runs both builds."""
    _expect_shape(name)
    monkeypatch.delenv('LT_JIT_DEFINES', raising=False)
    got1, d1 = _run(eng, name)
    monkeypatch.setenv('LT_JIT_DEFINES', OFF)
    s0 = eng.jit_stats()
    got0, d0 = _run(eng, name)
    s1 = eng.jit_stats()
    print('%s: deferred %d, %d with %s' % (name, d1, d0, OFF))
    # the switch reached the kernels: its launch took a module of its own (built or read back)
    assert s1['compiles'] + s1['disk_hits'] > s0['compiles'] + s0['disk_hits'], (s0, s1)
    _check(name, got1)
    _check(name, got0)
    for f in LABELS:
        assert got1[f].tobytes() == got0[f].tobytes(), (name, f, _summary(name))
    assert d1 == d0, (name, d1, d0, _summary(name))
