"""Year offsets past 63 on the GPU: scenes whose calendar years have gaps, with spans of 63-255
years (spanfixture.YEAR_LISTS). Every other GPU scene has consecutive years, so none of them reaches
what the kernels do only past offset 63: the wide zero-residual bound and vertex-fit width
(lt_pixel.h zero_bound / kZeroWide, fit_width_factor) in the lazy DP and the certified labels path
(lt_fast.h), uint8_t offsets above 63 in LDS, and the slots of the x-set factor table whose x-set
starts at an offset <= 63 and ends past it (lt_lapack.h xset_key; lsq_lockstep and
lsq_fit_lockstep of the analyze, resolve and fit-to-vertex kernels load them). Those slots were
once left empty (rc -4): the DP priced such starts with e = 0 and the pixels came out with wrong
fits and LT_ST_NUMERIC.

Everything is compared bit for bit, with the reference's own outputs (tests/golden/span_*.npz) and
with the oracle (oracle/lt_oracle.c), which tests/test_span_host.py pins to the reference on these
year lists; the expected status is the oracle's, 0 on all of these inputs.

span63_y33 is the control (every offset <= 63). span64_y33 reaches past 63 only across a 33-year
gap, beyond every gap the table holds: it runs the wide bounds and the factor-on-the-fly path, not
an affected slot (spanfixture._check_lists)."""
import datetime as dt
import os

import numpy as np
import pytest
import torch

import ftvfixture as fx
import golden_io
import spanfixture as sf
import test_gpu_wide as tw
import vertexfixture as vx
import widefixture as wf
from land_trendr_amd import _abi, index_eqn
from land_trendr_amd.engine import Engine, LtError, pack_valid_bits
from land_trendr_amd.scene import build_scene, parse_date
from land_trendr_amd.settings import compile_params

pytestmark = pytest.mark.gpu
P = sf.P
LABELS = tw.LABELS
LINE_COSTS = (10.0, 1.0, 0.5)
THREADS = min(os.cpu_count() or 1, 16)
LISTS = list(sf.YEAR_LISTS)
_cache = {}  # a case's inputs and oracle planes, computed once for every test that uses it


@pytest.fixture(scope='module')
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope='module')
def eng_pre():
    """A context of its own for the precompiled runs of a program: no JIT module in its map."""
    e = Engine(0)
    yield e
    e.close()


def _prog():
    return index_eqn.IndexProgram('B1 - B2', band_dtype='int16')


def _case(key, make):
    """(meta, params, values, valid, the oracle's planes) of make(), cached under key."""
    from oracle import oracle
    if key not in _cache:
        meta, params, vals, valid = make()
        want = oracle.analyze_tile(meta, params, vals, valid, n_threads=THREADS)
        assert (want['status'] == 0).all(), key
        _cache[key] = (meta, params, vals, valid, want)
    return _cache[key]


def _noise(name, lc, n_rules=1):
    return _case(('noise', name, lc, n_rules), lambda: sf.noise_case(name, lc, n_rules=n_rules))


def _full_and_labels(eng, case, how, tag, **kw):
    """test_gpu_wide._full_and_labels, and status 0 everywhere."""
    full = tw._full_and_labels(eng, case, how, tag, **kw)
    assert (full['status'] == 0).all(), (tag, how, int((full['status'] != 0).sum()))
    return full


# ---- a. the reference's own outputs ---------------------------------------------------------------

@pytest.mark.parametrize('how', ['f64', 'f32'])
@pytest.mark.parametrize('name', sf.span_names())
def test_span_golden_scene_bit_exact(eng, name, how):
    g = sf.SpanScene(name)
    valid = None if g.valid.all() else g.valid
    v, m = tw._inputs(eng, g.values, valid, how)  # (asserts the values exact in binary32)
    got = tw._host(eng.analyze_tile(g.scene, g.params, v, m))
    bad = golden_io.compare(g, got)
    assert not bad, '\n'.join(bad[:40])
    assert (got['status'] == 0).all()


# ---- b. noise values on every list against the oracle --------------------------------------------

@pytest.mark.parametrize('how', ['f64', 'f32', 'i16'])
@pytest.mark.parametrize('lc', LINE_COSTS)
@pytest.mark.parametrize('name', LISTS)
def test_precompiled_kernels_match_the_oracle(eng, eng_pre, name, lc, how, tmp_path, monkeypatch):
    """'i16': band pairs through the compiled B1 - B2 program with every JIT compile failing
    (LT_SRC_DIR names an empty directory, the switch of test_gpu_mask32.py), so the tiles run on
    the library's own instances."""
    case = _noise(name, lc)
    if how != 'i16':
        before = eng.jit_stats()['jit_tiles']
        full = _full_and_labels(eng, case, how, (name, lc))
        assert eng.jit_stats()['jit_tiles'] == before
    else:
        monkeypatch.setenv('LT_SRC_DIR', str(tmp_path))  # no kernel headers: no JIT module
        before = eng_pre.jit_stats()
        full = _full_and_labels(eng_pre, case, how, (name, lc),
                                index=eng_pre.compile_index(_prog()))
        st = eng_pre.jit_stats()
        assert st['fallback_tiles'] == before['fallback_tiles'] + 2, (before, st)
        assert st['jit_tiles'] == 0 and 'not found' in st['last_error'], st
    assert full['matched'].any()
    assert (full['n_years'] == (len(sf.YEAR_LISTS[name]) if case[3] is None
                                else case[3].sum(axis=0))).all()


@pytest.mark.parametrize('fields', ['full', 'labels'])
@pytest.mark.parametrize('lc', LINE_COSTS)
@pytest.mark.parametrize('name', LISTS)
def test_jit_kernels_match_the_oracle(eng, name, lc, fields):
    """index= the program: kernels specialised for the launch (lt_jit.h), with the scene's years,
    the line cost and the output planes among the constants: one module, and one compile of 3-5 s,
    per case."""
    meta, params, vals, valid, want = _noise(name, lc)
    v, m = tw._inputs(eng, vals, valid, 'i16')
    names = tuple(want) if fields == 'full' else LABELS
    before = eng.jit_stats()
    got = tw._host(eng.analyze_tile(meta, params, v, m, names, index=eng.compile_index(_prog())))
    after = eng.jit_stats()
    assert after['jit_tiles'] == before['jit_tiles'] + 1, after
    tw._assert_planes(got, want, ('jit', name, lc, fields), names)
    assert (got['status'] == 0).all()


# ---- c. ties: the resolve stage's exact-OPT DP ----------------------------------------------------

@pytest.mark.parametrize('name', ['biennial_y64', 'span255_y30'])
def test_tie_heavy_series_through_the_resolve_kernel(eng, name):
    """Exact rational ties at line cost 1e-4: the analyze kernel defers a large share of the pixels
    to the resolve kernel, whose exact-OPT DP prices every start through lsq_lockstep."""
    meta, params, vals, valid, want = _case(('tie', name), lambda: sf.tie_case(name, 1e-4))
    for how in ('f64', 'i16'):
        v, m = tw._inputs(eng, vals, valid, how)
        kw = dict(lin=eng.compile_index(_prog()).lin) if how == 'i16' else {}
        got = tw._host(eng.analyze_tile(meta, params, v, m, **kw))
        n_def = eng.last_deferred()
        print('%s %s: last_deferred() = %d of 1024' % (name, how, n_def))
        tw._assert_planes(got, want, ('tie', name, how))
        assert (got['status'] == 0).all()
        assert n_def >= 32, n_def


# ---- d. exactly collinear series: the zero-residual shortcut under kZeroWide ----------------------

@pytest.mark.parametrize('lc', [10.0, 1e-4])
@pytest.mark.parametrize('name', ['biennial_y64', 'span255_y64'])
def test_collinear_int16_series_match_the_oracle(eng, name, lc):
    case = _case(('collinear', name, lc), lambda: sf.collinear_case(name, lc))
    want = case[4]
    if lc == 1e-4:  # every kink is a vertex: segments of 3+ collinear points between them
        assert (want['vertex'].sum(axis=0) >= 8).mean() > 0.9
    lin = eng.compile_index(_prog()).lin
    _full_and_labels(eng, case, 'f64', ('collinear', name, lc))
    _full_and_labels(eng, case, 'i16', ('collinear', name, lc), lin=lin)


# ---- e. 16 rules labels-only: the certified labels path at 16 kFitW --------------------------------

@pytest.mark.parametrize('name', ['span255_y64', 'late_dense_y64'])
def test_sixteen_rules_labels_only_match_the_full_launch_and_the_oracle(eng, name):
    case = _noise(name, 10.0, n_rules=16)
    want = case[4]
    assert (want['matched'].sum(axis=1) > 0).sum() >= 8  # most rules label some pixel
    lin = eng.compile_index(_prog()).lin
    _full_and_labels(eng, case, 'f64', ('r16', name))
    _full_and_labels(eng, case, 'i16', ('r16', name), lin=lin)


# ---- f. fit to vertex on a span analysis -----------------------------------------------------------

@pytest.mark.parametrize('name', ['biennial_y64', 'span255_y30'])
def test_fit_to_vertex_on_a_span_analysis(eng, name):
    """lt_ftv_tile (lsq_fit_lockstep on the analysis's segments) against ftvfixture.ftv_numpy, for
    an int16 and a binary64 second band, on the first 321 pixels."""
    n = 321
    meta, params, vals, valid, want = _noise(name, 10.0)
    v, m = tw._inputs(eng, np.ascontiguousarray(vals[:, :n]), valid, 'f64')
    a = eng.analyze_tile(meta, params, v, m, ('winner', 'spike', 'vertex', 'status'))
    planes = tw._host(a)
    for f in ('winner', 'spike', 'vertex'):
        assert (planes[f] == want[f][:, :n]).all(), (name, f)
    rng = np.random.default_rng(64)
    Y = meta.n_years
    for second in (rng.integers(-3000, 3000, (Y, n)).astype(np.int16), rng.normal(300, 200, (Y, n))):
        got = tw._host(eng.ftv_tile(meta, a['winner'], a['spike'], a['vertex'],
                                    torch.from_numpy(second).to(eng.device)))
        ref = fx.ftv_numpy(meta.years, planes['winner'], planes['spike'], planes['vertex'], second)
        assert (ref['status'] == 0).all()
        for f in fx.FTV_FIELDS:
            same = fx.bits_equal(got[f], ref[f])
            assert same.all(), (name, second.dtype, f, int((~same).sum()))
        assert (got['status'] == 0).all(), (name, second.dtype)
    # the same series as the second band gives the analysis's own fitted planes
    got = tw._host(eng.ftv_tile(meta, a['winner'], a['spike'], a['vertex'], v))
    for f in ('val_fit', 'fit_m', 'fit_b', 'right_m', 'right_b'):
        assert wf.bits_equal(got[f], want[f][:, :n]).all(), (name, f)


# ---- g. the span limit ------------------------------------------------------------------------------

@pytest.mark.parametrize('span', [255, 256])
def test_year_span_limit(eng, span):
    """A span of 255 years is accepted, 256 refused with LT_ERR_LIMIT by the analysis and by fit to
    vertex, nothing written."""
    dates = [dt.date(2014 - span, 7, 1), dt.date(2000, 7, 1), dt.date(2014, 7, 1)]
    meta = build_scene(dates, parse_date(sf.TARGET))
    params, _ = compile_params(10.0, sf.GD)
    n = 130
    vals = torch.arange(3 * n, dtype=torch.float64, device=eng.device).reshape(3, n)
    out = eng.alloc_outputs(3, 1, n)
    guard = {f: (7 if t.dtype in (torch.uint8, torch.int16, torch.int32) else 7.5)
             for f, t in out.items()}
    for f, t in out.items():
        t.fill_(guard[f])
    winner = torch.arange(3, dtype=torch.int16, device=eng.device)[:, None].repeat(1, n)
    spike = torch.zeros((3, n), dtype=torch.uint8, device=eng.device)
    vertex = torch.ones((3, n), dtype=torch.uint8, device=eng.device)
    fout = {f: torch.full((3, n), 7.5, dtype=torch.float64, device=eng.device)
            for f in fx.FTV_FIELDS}
    fout['status'] = torch.full((n,), 7, dtype=torch.int32, device=eng.device)
    if span == 256:
        with pytest.raises(LtError) as ei:
            eng.analyze_tile(meta, params, vals, None, out=out)
        assert '(%d)' % vx.LT_ERR_LIMIT in str(ei.value), str(ei.value)
        with pytest.raises(LtError) as ei:
            eng.ftv_tile(meta, winner, spike, vertex, vals, out=fout)
        assert '(%d)' % vx.LT_ERR_LIMIT in str(ei.value), str(ei.value)
        for o, g in ((out, guard), (fout, {f: (7 if f == 'status' else 7.5) for f in fout})):
            for f, t in tw._host(o).items():
                assert (t == g[f]).all(), f
        return
    from oracle import oracle
    got = tw._host(eng.analyze_tile(meta, params, vals, None, out=out))
    want = oracle.analyze_tile(meta, params, vals.cpu().numpy(), None)
    tw._assert_planes(got, want, 'span 255')
    assert (got['status'] == 0).all() and (got['n_years'] == 3).all()
    ftv = tw._host(eng.ftv_tile(meta, winner, spike, vertex, vals, out=fout))
    ref = fx.ftv_numpy(meta.years, *(t.cpu().numpy() for t in (winner, spike, vertex, vals)))
    for f in fx.FTV_FIELDS:
        assert fx.bits_equal(ftv[f], ref[f]).all(), f
    assert (ftv['status'] == 0).all() and (ref['status'] == 0).all()


# ---- h. repeatability -------------------------------------------------------------------------------

def test_two_launches_give_identical_planes(eng):
    meta, params, vals, valid, want = _noise('span255_y64', 1.0)
    v, m = tw._inputs(eng, vals, valid, 'f64')
    first = tw._host(eng.analyze_tile(meta, params, v, m))
    again = tw._host(eng.analyze_tile(meta, params, v, m))
    for f in first:
        assert first[f].tobytes() == again[f].tobytes(), f
    tw._assert_planes(first, want, 'repeat')
