"""The wide sizes without a GPU: 41-64-point least squares, the wide_* golden scenes (49-64 years,
5-16 rules, exactly full 32 / 48 / 64-year instances) and the synthetic cases of
tests/test_gpu_wide.py, through the oracle (oracle/lt_oracle.c) and through the kernels' per-pixel
code compiled for the host (lt_pixel.h, tests/native/lapack_host_check.hip). The goldens are the
reference's own outputs (tests/golden/make_wide_golden.py), so this pins the checker of the GPU
tests at these sizes: a GPU mismatch there is then a kernel's, not the checker's. Bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import golden_io
import test_kernel_host as tk
import widefixture as wf
from land_trendr_amd import _abi
from oracle import oracle

D = ctypes.POINTER(ctypes.c_double)
THREADS = min(os.cpu_count() or 1, 16)


@pytest.fixture(scope='module')
def hc():
    if not os.path.exists(tk.HOSTCHECK):
        pytest.fail('host harness not built: run __graft_entry__.build()')
    L = ctypes.CDLL(tk.HOSTCHECK)
    L.ltx_analyze_tile.argtypes = [ctypes.POINTER(_abi.LtScene), ctypes.POINTER(_abi.LtParams),
                                   ctypes.POINTER(_abi.LtTileIn), ctypes.POINTER(_abi.LtTileOut)]
    L.ltx_lstsq.argtypes = [ctypes.c_int, D, D, ctypes.c_int, D]
    L.ltx_lstsq_xint.argtypes = [ctypes.c_int, D, D, ctypes.c_int, ctypes.c_int, D]
    return L


@pytest.fixture(scope='module')
def lstsq_wide():
    z = dict(np.load(os.path.join(golden_io.GOLDEN, 'lstsq_wide.npz')))
    assert len(z['m']) == 3000 and z['m'].min() == 41 and z['m'].max() == 64
    assert z['x'].max() == 63
    return z


def _cases(z):
    for t in range(len(z['m'])):
        m = int(z['m'][t])
        yield (np.ascontiguousarray(z['x'][t, :m]), np.ascontiguousarray(z['y'][t, :m]),
               (z['slope'][t], z['icpt'][t], z['ssr'][t]))


def _same3(got, want):
    return all(golden_io._bits_equal(a, b) for a, b in zip(got, want))


def test_oracle_lstsq_matches_reference_41_to_64_points(lstsq_wide):
    bad = 0
    for x, y, want in _cases(lstsq_wide):
        rc, s, c, r = oracle.lstsq(x, y)
        assert rc == 0
        bad += not _same3((s, c, r), want)
    assert bad == 0, '%d of 3000 segments differ from the reference' % bad


def test_device_lstsq_matches_reference_41_to_64_points(hc, lstsq_wide):
    """ltx_lstsq (lt_lapack.h's emulation) and ltx_lstsq_xint (the fused integer-x variant, with
    and without the solution / the residual)."""
    bad = bad_x = 0
    for x, y, want in _cases(lstsq_wide):
        o = (ctypes.c_double * 3)()
        rc = hc.ltx_lstsq(len(x), x.ctypes.data_as(D), y.ctypes.data_as(D), 1, ctypes.cast(o, D))
        assert rc == 0
        bad += not _same3(tuple(o), want)
        rc = hc.ltx_lstsq(len(x), x.ctypes.data_as(D), y.ctypes.data_as(D), 0, ctypes.cast(o, D))
        assert rc == 0
        bad += not golden_io._bits_equal(o[2], want[2])
        for sol, ssr in ((1, 1), (1, 0), (0, 1)):
            o = (ctypes.c_double * 3)()
            rc = hc.ltx_lstsq_xint(len(x), x.ctypes.data_as(D), y.ctypes.data_as(D), sol, ssr,
                                   ctypes.cast(o, D))
            assert rc == 0
            if sol:
                bad_x += not _same3(o[:2], want[:2])
            if ssr:
                bad_x += not golden_io._bits_equal(o[2], want[2])
    assert (bad, bad_x) == (0, 0)


def test_wide_fixture_set():
    assert wf.wide_names() == ['y32_r5', 'y48_r1', 'y49_ties_r16', 'y64_masks_r5',
                                      'y64_r16', 'y64_ties_r1']
    assert not set(wf.wide_names()) & set(golden_io.scene_names())
    shape = {}
    for name in wf.wide_names():
        g = wf.WideScene(name)
        assert g.meta['mode'] == 'documented' and not any(g.err)
        yrs = g.meta['years']
        assert yrs == list(range(yrs[0], yrs[0] + len(yrs)))  # consecutive years: x <= 63
        shape[name] = (len(yrs), len(g.rules), g.n_pix)
        if len(g.rules) > 1:  # the rule planes are not trivially empty or full
            n = g.ref['matched'].sum(axis=1)
            assert (n > 0).sum() >= len(g.rules) // 2 and (n < g.n_pix).any(), (name, n)
    assert shape == {'y64_r16': (64, 16, 192), 'y64_masks_r5': (64, 5, 128),
                     'y49_ties_r16': (49, 16, 128), 'y64_ties_r1': (64, 1, 128),
                     'y32_r5': (32, 5, 64), 'y48_r1': (48, 1, 64)}
    g = wf.WideScene('y64_r16')
    strip = lambda r: {k: v for k, v in r.items() if k not in ('name', 'val')}
    for a, b in ((1, 12), (3, 14)):  # the pairs that differ in val (and name) only
        ra, rb = g.meta['rules'][a], g.meta['rules'][b]
        assert strip(ra) == strip(rb) and ra['val'] != rb['val']
        assert (g.ref['matched'][a] == g.ref['matched'][b]).all()


@pytest.mark.parametrize('name', wf.wide_names())
def test_oracle_wide_scene_bit_exact(name):
    g = wf.WideScene(name)
    out = oracle.analyze_tile(g.scene, g.params, g.values, g.valid, n_threads=THREADS)
    bad = golden_io.compare(g, out)
    assert not bad, '\n'.join(bad[:40])


@pytest.mark.parametrize('name', wf.wide_names())
def test_kernel_code_on_host_matches_reference_wide(hc, name):
    g = wf.WideScene(name)
    out = tk.run_host(hc, g.scene, g.params, g.values, g.valid)
    bad = golden_io.compare(g, out)
    assert not bad, '\n'.join(bad[:40])


def _host_vs_oracle(hc, case, tag):
    meta, params, vals, valid = case
    want = oracle.analyze_tile(meta, params, vals, valid, n_threads=THREADS)
    got = tk.run_host(hc, meta, params, vals, valid)
    for f in want:
        same = wf.bits_equal(want[f], got[f])
        assert same.all(), (tag, f, int((~same).sum()))
    return got, want


@pytest.mark.parametrize('years,n_rules', wf.MATRIX)
def test_host_build_matches_oracle_on_the_instance_matrix(hc, years, n_rules):
    got, want = _host_vs_oracle(hc, wf.matrix_case(years, n_rules, 1061), (years, n_rules))
    assert (want['status'] == 0).all()
    assert want['matched'].any()


@pytest.mark.parametrize('n_rules', [1, 16])
def test_host_build_matches_oracle_on_mixed_lengths_at_64_years(hc, n_rules):
    case = wf.mixed_case(n_rules, 1061)
    assert sorted(set(case[3].sum(axis=0))) == list(range(65))  # 0..64 points
    _host_vs_oracle(hc, case, ('mixed', n_rules))


@pytest.mark.parametrize('years', [32, 48, 64])
def test_host_build_matches_oracle_on_values_binary32_cannot_hold(hc, years):
    _host_vs_oracle(hc, wf.wide_values_case(years, 1061), ('wide values', years))


def test_host_build_matches_oracle_at_the_observation_limit(hc):
    case = wf.obs_limit_case()
    assert case[0].n_obs == _abi.LT_MAX_OBS and case[0].n_years == 64
    got, want = _host_vs_oracle(hc, case, 'K=1024')
    assert (want['status'] == 0).all()
    assert want['winner'].max() >= 1008  # observations of the last year are picked


@pytest.mark.parametrize('rules', ['gd_ld', 'r16'])
@pytest.mark.parametrize('lc', [1e-4, 0.5])
@pytest.mark.parametrize('T', [49, 64])
def test_tie_heavy_series_defer_pixels_and_match_oracle(hc, T, lc, rules):
    """The tie-heavy inputs of the GPU resolve tests must defer pixels to the exact DP (a condition
    on the inputs: the resolve kernel is only run by deferred pixels), and the host build must
    agree with the oracle on them. Measured with the 2-rule set: 367 / 163 of 1024 at 49 years
    (line cost 1e-4 / 0.5), 331 / 203 at 64 years."""
    rl = wf.GD_LD if rules == 'gd_ld' else wf.tie_rules16(T)
    got, _ = _host_vs_oracle(hc, wf.tie_case(T, rl, lc), (T, lc, rules))
    print('T=%d lc=%g %s: %d of 1024 pixels deferred' % (T, lc, rules, got['_deferred']))
    assert got['_deferred'] >= 100
