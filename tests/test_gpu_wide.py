"""The wide analyze / resolve instances on the GPU: scenes of 32-64 years with 1-16 label rules.

The kernels are built as nine (MAXY, RMAX) instances (year capacity 32 / 48 / 64, rule capacity
1 / 4 / 16; lt_dispatch.hip), each for int16, binary32 and binary64 series. The other GPU tests stay
at 40 years and 4 rules or fewer, so the (64, *) and (*, 16) instances run here: the second
exact-OPT DP of the resolve kernel (MAXY > LT_RESOLVE_PRIV_MAXY, lt_fast.h), the labels-only path
beyond LT_CERT_RULES rules, exactly full instances (32, 48, 64 years: the last bit of the 64-bit
year masks), LT_MAX_OBS observations, and the JIT buckets of the same sizes. Everything is compared
bit for bit, with the reference's own outputs (tests/golden/wide_*.npz) and with the oracle
(oracle/lt_oracle.c), which tests/test_wide_host.py pins to the reference at these sizes. Every
series has consecutive calendar years (x <= 63)."""
import os

import numpy as np
import pytest
import torch

import ftvfixture as fx
import golden_io
import vertexfixture as vx
import widefixture as wf
from land_trendr_amd import _abi, index_eqn
from land_trendr_amd.engine import ALL_FIELDS, Engine, LtError, pack_valid_bits
from land_trendr_amd.scene import build_scene, parse_date
from land_trendr_amd.settings import compile_params

pytestmark = pytest.mark.gpu
P = 1061  # 16 full waves and a partial one
LABELS = ('status',) + tuple(f for f, _ in _abi.RULE_FIELDS)
JIT_LABELS = ('status', 'matched', 'class_val', 'onset_year', 'duration', 'magnitude')
TREND4 = ('val_fit', 'fit_m', 'fit_b', 'vertex')
THREADS = min(os.cpu_count() or 1, 16)
_cache = {}  # a case's inputs and oracle planes, computed once for every test that uses it


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def b1_b2(eng):
    return eng.compile_index(index_eqn.IndexProgram('B1 - B2', band_dtype='int16'))


def _case(key, make):
    """(meta, params, values, valid, the oracle's planes) of make(), cached under key."""
    from oracle import oracle
    if key not in _cache:
        meta, params, vals, valid = make()
        want = oracle.analyze_tile(meta, params, vals, valid, n_threads=THREADS)
        _cache[key] = (meta, params, vals, valid, want)
    return _cache[key]


def _host(out):
    torch.cuda.synchronize()
    return {f: t.cpu().numpy() for f, t in out.items()}


def _inputs(eng, vals, valid, how):
    """The device tensors of one series in one of the forms a tile may carry: 'f64' / 'f32' values
    with a byte mask, or 'i16' pixel-interleaved band pairs (B1 - B2 = the value) with the mask as
    bit planes."""
    if how == 'i16':
        rng = np.random.default_rng(5)
        v = vals.astype(np.int64)
        assert (v == vals).all()
        b2 = rng.integers(100, 401, v.shape)
        assert np.abs(v + b2).max() < 32768
        bands = np.stack([v + b2, b2], axis=1).astype(np.int16)  # [K, 2, P]
        K, _, n = bands.shape
        t = torch.empty((K, n, 2), dtype=torch.int16, device=eng.device).permute(0, 2, 1)
        t.copy_(torch.from_numpy(bands))
        m = None if valid is None else pack_valid_bits(torch.from_numpy(valid).to(eng.device))
        return t, m
    a = np.ascontiguousarray(vals, np.float64)
    if how == 'f32':
        a = a.astype(np.float32)
        assert (a.astype(np.float64) == vals).all()
    m = None if valid is None else torch.from_numpy(np.ascontiguousarray(valid)).to(eng.device)
    return torch.from_numpy(a).to(eng.device), m


def _assert_planes(got, want, tag, fields=None):
    for f in (fields if fields is not None else want):
        g = got[f]
        w = want[f][:g.shape[0]] if g.ndim == 2 else want[f]
        assert w.shape == g.shape, (tag, f, g.shape, w.shape)
        same = wf.bits_equal(w, g)
        assert same.all(), (tag, f, int((~same).sum()), np.argwhere(~same)[:5].tolist())


def _full_and_labels(eng, case, how, tag, **kw):
    """A launch writing every plane and a labels-only launch of one case: both against the oracle,
    the labels-only rule planes against the full launch's, status 0 everywhere."""
    meta, params, vals, valid, want = case
    v, m = _inputs(eng, vals, valid, how)
    full = _host(eng.analyze_tile(meta, params, v, m, **kw))
    lab = _host(eng.analyze_tile(meta, params, v, m, LABELS, **kw))
    _assert_planes(full, want, (tag, how, 'full'))
    _assert_planes(lab, want, (tag, how, 'labels only'), LABELS)
    _assert_planes(lab, full, (tag, how, 'labels only vs full'), LABELS)
    return full


# ---- a. the reference's own outputs at the wide sizes -------------------------------------------

@pytest.mark.parametrize('how', ['f64', 'f32'])
@pytest.mark.parametrize('name', wf.wide_names())
def test_wide_golden_scene_bit_exact_and_repeatable(eng, name, how):
    g = wf.WideScene(name)
    v, m = _inputs(eng, g.values, g.valid, how)  # (asserts the values exact in binary32)
    first = _host(eng.analyze_tile(g.scene, g.params, v, m))
    bad = golden_io.compare(g, first)
    assert not bad, '\n'.join(bad[:40])
    again = _host(eng.analyze_tile(g.scene, g.params, v, m))
    for f in first:
        assert first[f].tobytes() == again[f].tobytes(), (name, how, f)


# ---- b. every (years, rules) pair against the oracle --------------------------------------------

def _matrix_runs():
    runs = [(y, r, how) for y, r in wf.MATRIX for how in ('f64', 'i16')]
    return runs + [(64, 1, 'f32'), (64, 16, 'f32')]


@pytest.mark.parametrize('years,n_rules,how', _matrix_runs())
def test_instance_matrix_matches_the_oracle(eng, b1_b2, years, n_rules, how):
    case = _case(('matrix', years, n_rules), lambda: wf.matrix_case(years, n_rules, P))
    before = eng.jit_stats()['jit_tiles']
    kw = dict(lin=b1_b2.lin) if how == 'i16' else {}
    full = _full_and_labels(eng, case, how, (years, n_rules), **kw)
    assert (full['status'] == 0).all()
    assert (full['n_years'] == years).all()
    assert full['matched'].any()
    assert eng.jit_stats()['jit_tiles'] == before  # the precompiled instances


# ---- c. the JIT buckets of the same sizes -------------------------------------------------------

@pytest.mark.parametrize('years,n_rules,fields', [(64, 1, JIT_LABELS), (64, 1, JIT_LABELS + TREND4),
                                                  (32, 16, JIT_LABELS)],
                         ids=['y64_r1_labels', 'y64_r1_trend4', 'y32_r16_labels'])
def test_jit_specialisations_match_the_oracle(eng, b1_b2, years, n_rules, fields):
    """index= the program: kernels specialised for the launch (lt_jit.h). With one rule they take
    the lazy DP's neighbour, triple and seed exits, here over 64 columns."""
    meta, params, vals, valid, want = _case(('matrix', years, n_rules),
                                            lambda: wf.matrix_case(years, n_rules, P))
    v, m = _inputs(eng, vals, valid, 'i16')
    before = eng.jit_stats()
    got = _host(eng.analyze_tile(meta, params, v, m, fields, index=b1_b2))
    after = eng.jit_stats()
    assert after['jit_tiles'] == before['jit_tiles'] + 1, after
    assert (got['status'] == 0).all()
    _assert_planes(got, want, ('jit', years, n_rules), fields)


# ---- d. series of every length in one wave at 64 years ------------------------------------------

@pytest.mark.parametrize('n_rules', [1, 16])
def test_mixed_lengths_at_64_years_match_the_oracle(eng, n_rules):
    case = _case(('mixed', n_rules), lambda: wf.mixed_case(n_rules, P))
    assert sorted(set(case[3].sum(axis=0))) == list(range(65))  # 0..64 points
    full = _full_and_labels(eng, case, 'f64', ('mixed', n_rules))
    assert (full['n_years'] == case[3].sum(axis=0)).all()


# ---- e. the resolve kernel at MAXY = 64 and at 48 / 49 years ------------------------------------

def _tie_rules(rules, T):
    return wf.GD_LD if rules == 'gd_ld' else wf.tie_rules16(T)


@pytest.mark.parametrize('rules', ['gd_ld', 'r16'])
@pytest.mark.parametrize('lc', [1e-4, 0.5])
@pytest.mark.parametrize('T', [49, 64])
def test_tie_heavy_series_through_the_resolve_kernel(eng, T, lc, rules):
    """Exact rational ties everywhere: the analyze kernel defers a large share of the pixels to the
    resolve kernel's exact-OPT DP (tests/test_wide_host.py: 163-367 of 1024 on the host build),
    which at 64 years is the variant with OPT in registers."""
    meta, params, vals, valid, want = _case(('tie', T, lc, rules),
                                            lambda: wf.tie_case(T, _tie_rules(rules, T), lc))
    v, m = _inputs(eng, vals, valid, 'f64')
    got = _host(eng.analyze_tile(meta, params, v, m))
    n_def = eng.last_deferred()
    print('T=%d lc=%g %s: last_deferred() = %d of 1024' % (T, lc, rules, n_def))
    _assert_planes(got, want, (T, lc, rules))
    assert n_def >= 32, n_def


@pytest.mark.parametrize('years', [32, 48, 64])
def test_binary64_resolve_with_16_rules_takes_every_pixel(eng, years):
    """Values binary32 cannot hold under 16 rules: the binary32 analyze instance (there is no
    binary64 one above 4 rules) hands every pixel to the binary64 resolve instance of its
    (MAXY, 16) pair, which the integer-valued cases above leave with an empty list."""
    meta, params, vals, valid, want = _case(('wide values', years),
                                            lambda: wf.wide_values_case(years, P))
    v, m = _inputs(eng, vals, valid, 'f64')
    got = _host(eng.analyze_tile(meta, params, v, m))
    n_def = eng.last_deferred()
    _assert_planes(got, want, ('wide values', years))
    assert (got['status'] == 0).all()
    assert n_def == P, n_def  # no value is exact in binary32: no pixel stays in the analyze stage


def test_analyze_tiles_batch_at_64_years(eng):
    """One analyze_tiles call over uneven tiles (an empty one, a one-pixel one) of the 64-year tie
    scene: tile t's resolve beside tile t+1's analyze. The single-tile results, and the oracle's."""
    meta, params, vals, valid, want = _case(('tie', 64, 1e-4, 'gd_ld'),
                                            lambda: wf.tie_case(64, wf.GD_LD, 1e-4))
    v, _ = _inputs(eng, vals, valid, 'f64')
    cuts = [0, 400, 400, 401, 1024]
    spans = list(zip(cuts[:-1], cuts[1:]))
    batch = eng.analyze_tiles(meta, params, [(v[:, a:b], None) for a, b in spans])
    single = [eng.analyze_tile(meta, params, v[:, a:b], None) for a, b in spans]
    torch.cuda.synchronize()
    for (a, b), ob, os_ in zip(spans, batch, single):
        x, y = _host(ob), _host(os_)
        for f in x:
            assert x[f].shape[-1] == b - a
            assert x[f].tobytes() == y[f].tobytes(), (a, b, f)
        _assert_planes(x, {f: w[..., a:b] for f, w in want.items()}, ('batch', a, b))


# ---- f. the observation limit --------------------------------------------------------------------

def test_scene_of_lt_max_obs_observations_matches_the_oracle(eng):
    case = _case('obs_limit', wf.obs_limit_case)
    meta, _, _, valid, want = case
    assert meta.n_obs == _abi.LT_MAX_OBS == 1024 and meta.n_years == 64
    for how in ('f64', 'f32'):
        v, m = _inputs(eng, case[2], valid, how)
        got = _host(eng.analyze_tile(meta, case[1], v, m))
        _assert_planes(got, want, ('K=1024', how, 'byte mask'))
        got = _host(eng.analyze_tile(meta, case[1], v, pack_valid_bits(m)))
        _assert_planes(got, want, ('K=1024', how, 'bit planes'))
    assert want['winner'].max() >= 1008 and (want['status'] == 0).all()


@pytest.mark.parametrize('what', ['n_obs_1025', 'n_years_65'])
def test_scene_above_the_limits_is_refused_and_writes_nothing(eng, monkeypatch, what):
    import datetime as dt
    # (build_scene has the same limits: lifted here so that the library's own check is reached)
    monkeypatch.setattr(_abi, 'LT_MAX_OBS', 1 << 20)
    monkeypatch.setattr(_abi, 'LT_MAX_YEARS', 1 << 10)
    if what == 'n_obs_1025':
        dates = [dt.date(1985 + k // 17, 5, 1 + k % 17) for k in range(1025)]
    else:
        dates = [dt.date(1950 + y, 7, 1) for y in range(65)]
    meta = build_scene(dates, parse_date(wf.TARGET))
    assert (meta.n_obs, meta.n_years) == ((1025, 61) if what == 'n_obs_1025' else (65, 65))
    params, _ = compile_params(10.0, wf.GD)
    n = 130
    vals = torch.zeros((meta.n_obs, n), dtype=torch.float64, device=eng.device)
    out = eng.alloc_outputs(meta.n_years, 1, n)
    guard = {f: (7 if t.dtype in (torch.uint8, torch.int16, torch.int32) else 7.5)
             for f, t in out.items()}
    for f, t in out.items():
        t.fill_(guard[f])
    with pytest.raises(LtError) as ei:
        eng.analyze_tile(meta, params, vals, None, out=out)
    assert '(%d)' % vx.LT_ERR_LIMIT in str(ei.value), str(ei.value)
    with pytest.raises(LtError) as ei:
        eng.analyze_tiles(meta, params, [(vals, None)], outs=[out])
    assert '(%d)' % vx.LT_ERR_LIMIT in str(ei.value), str(ei.value)
    for f, t in _host(out).items():
        assert (t == guard[f]).all(), f


def test_seventeen_rules_are_refused():
    assert _abi.LT_MAX_RULES == 16
    rules = wf.wide_rules(16) + [{'name': 'r16', 'val': 17, 'change_type': 'GD'}]
    with pytest.raises(ValueError):
        compile_params(10.0, rules, 'documented')
    assert compile_params(10.0, rules[:16], 'documented')[0].n_rules == 16


# ---- g. the kernels that read an analysis's planes, at 64 years ---------------------------------

@pytest.mark.parametrize('name', ['y64_r16', 'y64_masks_r5'])
def test_vertex_table_and_fit_to_vertex_on_a_64_year_analysis(eng, name):
    g = wf.WideScene(name)
    v, m = _inputs(eng, g.values, g.valid, 'f64')
    a = eng.analyze_tile(g.scene, g.params, v, m, ALL_FIELDS)
    table = _host(eng.vertex_table(g.scene.years, a['val_fit'], a['vertex'], winner=a['winner'],
                                   val_raw=a['val_raw']))
    want = vx.vertex_numpy(g.scene.years, g.ref['val_fit'], g.ref['vertex'],
                           winner=g.ref['winner'], val_raw=g.ref['val_raw'])
    vx.assert_table(table, want, name)
    assert table['n_vertices'].max() > 2
    # fit to vertex of the same series: the analysis's own fitted planes (the reference's)
    ftv = _host(eng.ftv_tile(g.scene, a['winner'], a['spike'], a['vertex'], v))
    fx.check_golden(g, ftv, g.ref['winner'])
