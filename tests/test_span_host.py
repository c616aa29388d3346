"""Year offsets past 63 without a GPU: the span goldens (tests/golden/make_span_golden.py, the
reference's own outputs on scenes whose years have gaps: spans of 63-255 years, and least squares
on x up to 255) through the oracle (oracle/lt_oracle.c) and through the kernels' per-pixel code
compiled for the host (lt_pixel.h, tests/native/lapack_host_check.hip), bit for bit. This pins the
checker of tests/test_gpu_span.py: a GPU mismatch there is then a kernel's, not the checker's.

The host build factors every segment directly and never reads the x-set factor table the GPU
kernels look segments up in (lt_lapack.h xset_key, lt_fast.h lsq_lockstep), so the table has a test
of its own here: every x-set xset_key maps to a slot must be the one the slot is filled from."""
import ctypes
import os

import numpy as np
import pytest

import golden_io
import spanfixture as sf
import test_kernel_host as tk
import widefixture as wf
from land_trendr_amd import _abi
from oracle import oracle

D = ctypes.POINTER(ctypes.c_double)
I = ctypes.POINTER(ctypes.c_int)
THREADS = min(os.cpu_count() or 1, 16)
KXT_SIZE = 64 * 16 + 3 * 64 * 64  # lt_lapack.h kXtSize
XSETCHECK = os.path.join(tk.ROOT, 'tests', 'native', 'build', 'liblt_xsetcheck.so')


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
def xc():
    """The x-set table's maps compiled for the host (tests/native/xset_host_check.hip)."""
    if not os.path.exists(XSETCHECK):
        pytest.fail('host harness not built: run __graft_entry__.build()')
    L = ctypes.CDLL(XSETCHECK)
    L.ltx_xset_key.argtypes = [ctypes.c_int, I]
    L.ltx_xset_of_key.argtypes = [ctypes.c_int, I, I]
    L.ltx_lsq_factor.argtypes = [ctypes.c_int, I, ctypes.c_void_p]
    return L


# ---- the year lists ------------------------------------------------------------------------------

def test_year_lists_reach_what_they_are_for():
    """(spanfixture asserts the same at import: restated where a failure is a test's.)"""
    assert sf.offsets(sf.CONTROL).max() == 63 and not sf.straddling_triples(sf.CONTROL)
    assert sf.offsets('span64_y33').max() == 64
    for name in ('biennial_y64', 'late_dense_y64', 'span255_y30', 'span255_y64'):
        assert sf.straddling_triples(name), name
    assert sf.straddling_run('late_dense_y64') >= 5
    for name in sf.YEAR_LISTS:
        meta = sf.meta_of(name)
        assert meta.n_years == meta.n_obs == len(sf.YEAR_LISTS[name])
    valid = sf.span_mask('late_dense_y64', sf.P)
    assert (valid[0, ::3] == 0).all() and 0.17 < 1 - valid[1:].mean() < 0.23


def test_span_fixture_set():
    names = sorted(sf.YEAR_LISTS) + ['biennial_y64_ties', 'span255_y64_collinear']
    assert sf.span_names() == sorted(names)
    assert not set(sf.span_names()) & (set(golden_io.scene_names()) | set(wf.wide_names()))
    for name in sf.span_names():
        g = sf.SpanScene(name)
        assert g.meta['mode'] == 'documented' and not any(g.err), name
        assert 64 <= g.n_pix <= 192
        ylist = next(n for n in sorted(sf.YEAR_LISTS, key=len, reverse=True) if name.startswith(n))
        assert g.meta['years'] == sf.YEAR_LISTS[ylist]
        assert g.ref['matched'].any() or name.endswith('collinear'), name
        assert os.path.getsize(os.path.join(golden_io.GOLDEN, 'span_%s.npz' % name)) < 1 << 20
    # the collinear scene has zero-residual segments: vertices joined by exact lines
    g = sf.SpanScene('span255_y64_collinear')
    assert (g.ref['vertex'].sum(0) >= 3).mean() > 0.5
    assert (np.abs(g.ref['val_fit'] - g.ref['val_raw']) < 1e-6).mean() > 0.5


# ---- least squares on offsets up to 255 ---------------------------------------------------------

@pytest.fixture(scope='module')
def lstsq_span():
    z = dict(np.load(os.path.join(golden_io.GOLDEN, 'lstsq_span.npz')))
    m = z['m']
    assert len(m) == 3000 and m.min() == 2 and m.max() == 64
    last = z['x'][np.arange(len(m)), m - 1]
    assert (last > 63).all() and last.max() == 255 and (z['x'] == np.round(z['x'])).all()
    gaps_ok = np.array([np.diff(z['x'][t, :m[t]]).max() <= 8 for t in range(len(m))])
    assert ((z['x'][:, 0] >= 48) & (z['x'][:, 0] <= 63) & gaps_ok).sum() >= 1000
    return z


def _cases(z):
    for t in range(len(z['m'])):
        m = int(z['m'][t])
        yield (np.ascontiguousarray(z['x'][t, :m]), np.ascontiguousarray(z['y'][t, :m]),
               (z['slope'][t], z['icpt'][t], z['ssr'][t]))


def _same3(got, want):
    return all(golden_io._bits_equal(a, b) for a, b in zip(got, want))


def test_oracle_lstsq_matches_reference_past_offset_63(lstsq_span):
    bad = 0
    for x, y, want in _cases(lstsq_span):
        rc, s, c, r = oracle.lstsq(x, y)
        assert rc == 0
        bad += not _same3((s, c, r), want)
    assert bad == 0, '%d of 3000 segments differ from the reference' % bad


def test_device_lstsq_matches_reference_past_offset_63(hc, lstsq_span):
    """ltx_lstsq (lt_lapack.h's emulation) and ltx_lstsq_xint (the fused integer-x variant, with
    and without the solution / the residual)."""
    bad = bad_x = 0
    for x, y, want in _cases(lstsq_span):
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


# ---- the x-set factor table ----------------------------------------------------------------------

def _families():
    """Every strictly increasing x-set with m <= 64 and x <= 255 that can have a slot, by family:
    xset_key tells the families apart by m alone and tests each gap against one limit (16 / 8 / 4),
    so gaps are taken to twice the limit, m = 2 gaps to the end, and x0 over the whole range."""
    for x0 in range(256):
        for d in range(1, 256 - x0):
            yield (x0, x0 + d)
        for d1 in range(1, 17):
            for d2 in range(1, 17):
                if x0 + d1 + d2 <= 255:
                    yield (x0, x0 + d1, x0 + d1 + d2)
        for d1 in range(1, 9):
            for d2 in range(1, 9):
                for d3 in range(1, 9):
                    if x0 + d1 + d2 + d3 <= 255:
                        yield (x0, x0 + d1, x0 + d1 + d2, x0 + d1 + d2 + d3)
        for m in range(5, 65):
            if x0 + m - 1 <= 255:
                yield tuple(range(x0, x0 + m))


def test_every_slot_xset_key_returns_is_filled_from_that_x_set(xc):
    """For every x-set xset_key maps to a slot, xset_of_key(slot) (what build_xtable_kernel fills
    the slot from, lt_abi.hip) must succeed and return that x-set, and the lsq_xf factored from it
    must be the one factored from the original, byte for byte: lsq_lockstep loads the slot for any
    key >= 0. Slots of x-sets that start at an offset <= 63 and end past it were left empty (rc -4)
    while xset_key returned them: 3,202 of the 13,312."""
    size = xc.ltx_lsq_xf_size()
    assert size == 136 and xc.ltx_xset_table_size() == KXT_SIZE
    n_sets = n_mapped = 0
    empty, wrong, differs, slots, past63 = set(), [], [], set(), set()
    back = (ctypes.c_int * 64)()
    fa, fb = ctypes.create_string_buffer(size), ctypes.create_string_buffer(size)
    for xs in _families():
        m = len(xs)
        arr = (ctypes.c_int * m)(*xs)
        n_sets += 1
        key = xc.ltx_xset_key(m, arr)
        if key < 0:
            continue
        assert key < KXT_SIZE and key not in slots, (xs, key)  # in range, one x-set per slot
        slots.add(key)
        n_mapped += 1
        if xs[-1] > 63:
            past63.add(key)
        mb = ctypes.c_int()
        if not xc.ltx_xset_of_key(key, ctypes.byref(mb), back):
            empty.add(key)
            continue
        if mb.value != m or tuple(back[:m]) != xs:
            wrong.append((xs, key, tuple(back[:mb.value])))
            continue
        assert xc.ltx_lsq_factor(m, arr, fa) == 0 and xc.ltx_lsq_factor(mb.value, back, fb) == 0
        if fa.raw != fb.raw:
            differs.append((xs, key))
    print('%d x-sets, %d with a slot (%d ending past offset 63), %d empty slots'
          % (n_sets, n_mapped, len(past63), len(empty)))
    assert not empty, '%d slots xset_key returns are empty, first %s' % (len(empty),
                                                                        sorted(empty)[:5])
    assert not wrong and not differs, (wrong[:3], differs[:3])
    # the table's shape: x0 0..63 with every allowed gap, consecutive runs of 5..64 points
    assert n_mapped == 64 * 16 + 64 * 64 + 64 * 64 + 64 * 60
    assert len(past63) == 3202
    # and no other slot is filled: the rest (runs shorter than 5) map to no x-set
    mb = ctypes.c_int()
    filled = {k for k in range(KXT_SIZE) if xc.ltx_xset_of_key(k, ctypes.byref(mb), back)}
    assert filled == slots


# ---- the span scenes ------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sf.span_names())
def test_oracle_span_scene_bit_exact(name):
    g = sf.SpanScene(name)
    out = oracle.analyze_tile(g.scene, g.params, g.values, g.valid, n_threads=THREADS)
    bad = golden_io.compare(g, out)
    assert not bad, '\n'.join(bad[:40])
    assert (out['status'] == 0).all()


@pytest.mark.parametrize('name', sf.span_names())
def test_kernel_code_on_host_matches_reference_span(hc, name):
    g = sf.SpanScene(name)
    out = tk.run_host(hc, g.scene, g.params, g.values, g.valid)
    bad = golden_io.compare(g, out)
    assert not bad, '\n'.join(bad[:40])
    assert (out['status'] == 0).all()


def _host_vs_oracle(hc, case, tag):
    meta, params, vals, valid = case
    want = oracle.analyze_tile(meta, params, vals, valid, n_threads=THREADS)
    got = tk.run_host(hc, meta, params, vals, valid)
    for f in want:
        same = wf.bits_equal(want[f], got[f])
        assert same.all(), (tag, f, int((~same).sum()))
    assert (want['status'] == 0).all(), tag
    return got, want


@pytest.mark.parametrize('name', list(sf.YEAR_LISTS))
def test_host_build_matches_oracle_on_the_gpu_cases(hc, name):
    """The synthetic inputs of tests/test_gpu_span.py: the noise values at the three line costs and
    under 16 rules, and the collinear series."""
    for lc in (10.0, 1.0, 0.5):
        _, want = _host_vs_oracle(hc, sf.noise_case(name, lc), (name, lc))
        assert want['matched'].any()
        # the pixels' own offsets (from their first present year) reach the list's span
        first = np.argmax(want['winner'] >= 0, axis=0)
        last = want['winner'].shape[0] - 1 - np.argmax(want['winner'][::-1] >= 0, axis=0)
        years = np.array(sf.YEAR_LISTS[name])
        assert (years[last] - years[first]).max() == sf.offsets(name)[-1]
    if name in ('span255_y64', 'late_dense_y64'):
        _, want = _host_vs_oracle(hc, sf.noise_case(name, 10.0, n_rules=16), (name, 'r16'))
        assert (want['matched'].sum(axis=1) > 0).sum() >= 8
    if name in ('biennial_y64', 'span255_y64'):
        for lc in (10.0, 1e-4):
            _host_vs_oracle(hc, sf.collinear_case(name, lc), (name, 'collinear', lc))


@pytest.mark.parametrize('name', ['biennial_y64', 'span255_y30'])
def test_tie_heavy_span_series_defer_pixels_and_match_oracle(hc, name):
    """The tie inputs of the GPU resolve test must defer pixels to the exact DP (the resolve kernel
    is only run by deferred pixels), and the host build must agree with the oracle on them."""
    got, _ = _host_vs_oracle(hc, sf.tie_case(name, 1e-4), (name, 'ties'))
    print('%s: %d of 1024 pixels deferred' % (name, got['_deferred']))
    assert got['_deferred'] >= 100
