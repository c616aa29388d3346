"""The change maps on the CPU: the kernels' host twin (tests/native/change_host_check.hip, the
per-pixel code of land_trendr_amd/csrc/lt_change.h) against the independent reference of
changefixture, bit for bit, into guarded buffers with padded strides; the argument checks; the
per-key count; the exports; and LocalJob through a CPU double whose change_maps, label_counts and
sieve are the host twins. No tolerances anywhere."""
import ctypes
import os

import numpy as np
import pytest

import changefixture as cx
import sievefixture as sx
from changefixture import (JOB_MAPS, JOB_MATCHED, JOB_REMOVED, SHAPE, check_change_files,
                           expected_stats, file_bytes, job_reference)
from land_trendr_amd import _abi


@pytest.fixture(scope='module')
def lib():
    return cx.load_host()


@pytest.mark.parametrize('tag', cx.case_tags())
def test_handmade_cases_against_the_reference(lib, tag):
    rules, kw = cx.case(tag)
    want = cx.case_reference(tag)
    for pad in (0, 5):
        cx.assert_maps(cx.run_host(lib, rules, pad=pad, **kw), want, (tag, pad))


def test_the_handmade_cases_hold_what_they_are_for():
    """The cases cannot pass vacuously: every sort has a pixel where two kept segments tie on its
    key and the first is the winner, zero and negative-zero and NaN steps occur, so do pixels
    without a fitted point and pixels whose rmse is zero, and every presence form and both fit
    forms run."""
    tags = cx.case_tags()
    for pres in cx.PRESENCE:
        for fit in ('-fit', '-nofit'):
            assert any(pres + fit in t for t in tags), (pres, fit)
    assert {len(r) for r in cx.rule_sets().values()} >= {1, 2, 3, 5, 8}
    ties = set()
    zero = negzero = nan = False
    for tag in tags:
        if 'sorts' not in tag:
            continue
        rules, kw = cx.case(tag)
        Y, P = kw['val_fit'].shape
        pres = kw['present'] != 0 if 'present' in kw else (
            kw['winner'] >= 0 if 'winner' in kw else np.ones((Y, P), bool))
        want = cx.case_reference(tag)
        for p in range(P):
            _, segs = cx.segments(kw['years'], kw['val_fit'], kw['vertex'], pres, p)
            for s in segs:
                zero |= s[3] == 0 and not np.signbit(s[3])
                negzero |= s[3] == 0 and bool(np.signbit(s[3]))
                nan |= bool(np.isnan(s[3]))
            for m, rule in enumerate(rules):
                col, way = cx._KEY[rule['sort']]
                kept = [s for s in segs if (s[3] > 0 if rule['delta'] == 'loss' else s[3] < 0)]
                if not kept:
                    continue
                top = (max if way > 0 else min)(s[col] for s in kept)
                tied = [s for s in kept if s[col] == top]
                # a tie the outputs can tell apart: taking a later one would show
                if len(tied) > 1 and any(s[:3] != tied[0][:3] for s in tied[1:]):
                    assert (want['onset_year'][m, p], want['duration'][m, p],
                            want['preval'][m, p]) == tied[0][:3], (tag, p, m)
                    ties.add(rule['sort'])
    assert ties == set(cx.SORTS), ties
    assert zero and negzero and nan
    fit = [cx.case_reference(t) for t in tags if t.endswith('-fit') and t.startswith('33x257')]
    assert any((w['n_fit'] == 0).any() for w in fit)
    assert any(np.isposinf(w['dsnr']).any() for w in fit)
    assert any((w['rmse'] == 0).any() for w in fit)


def test_without_the_fit_inputs_val_raw_is_never_read(lib):
    """No val_raw and no spike (NULL: a read would fault): the six map planes come out as with
    them. And with them but no rmse / n_fit / dsnr asked for, the same again."""
    rules, kw = cx.case('33x257-loss-sorts-winner-fit')
    if 'val_raw' not in kw:
        kw = dict(kw, val_raw=cx._planes(33, 257, False)[2], spike=cx._planes(33, 257, False)[4])
    full = cx.run_host(lib, rules, pad=3, **kw)
    six = {f: a for f, a in full.items() if f not in ('dsnr', 'rmse', 'n_fit')}
    bare = {k: v for k, v in kw.items() if k not in ('val_raw', 'spike')}
    cx.assert_maps(cx.run_host(lib, rules, pad=3, **bare), six, 'no inputs')
    cx.assert_maps(cx.run_host(lib, rules, pad=3, fields=tuple(six), **kw), six, 'no outputs')
    one = cx.run_host(lib, rules, pad=3, fields=('matched', 'rmse'), **kw)
    cx.assert_maps(one, {f: full[f] for f in ('matched', 'rmse')}, 'two outputs')


def test_random_field_against_the_reference(lib):
    kw = cx.random_field(4099, 30, seed=3)
    want = cx.reference(rules=cx.EIGHT, **kw)
    assert (want['matched'].sum(axis=1) > 0).all()
    cx.assert_maps(cx.run_host(lib, cx.EIGHT, pad=7, **kw), want, 'random')
    for M in (1, 3):
        got = cx.run_host(lib, cx.EIGHT[:M], pad=1, **kw)
        cx.assert_maps(got, {f: (a if f in cx.PIX_FIELDS else a[:M]) for f, a in want.items()},
                       ('random', M))


def test_argument_checks_write_nothing(lib):
    A, L = cx.LT_ERR_ARG, cx.LT_ERR_LIMIT
    Y, P, M = 6, 70, 3
    years, val_fit, val_raw, vertex, spike, present, winner = cx.handmade(Y, P, seed=1)
    yrs = np.ascontiguousarray(years)
    ins = {'val_fit': val_fit, 'vertex': vertex, 'val_raw': val_raw, 'present': present,
           'winner': winner, 'spike': spike}
    ins = {f: np.ascontiguousarray(a) for f, a in ins.items()}
    bufs = cx.guarded_outputs(M, P, 0, cx.MAP_FIELDS + cx.PIX_FIELDS)
    before = {f: b.copy() for f, b in bufs.items()}
    optr = cx.output_ptrs(bufs, 0)
    good = [{'delta': 'loss'}, {'delta': 'gain', 'year': [1990, 1991]},
            {'delta': 'loss', 'mag': ['>', 1]}]

    def call(n_pix=P, stride=P, ostride=P, n_maps=M, n_years=None, null=None, odrop=(),
             use=('val_fit', 'vertex', 'val_raw', 'present', 'spike'), edit=None, no_year=False):
        cin, cout = cx.structs(yrs, n_pix, stride, {f: ins[f].ctypes.data for f in use}, ostride,
                               {f: a for f, a in optr.items() if f not in odrop})
        if n_years is not None:
            cin.n_years = n_years
        if no_year:
            cin.year = None
        rules = cx.c_rules(good)
        if edit:
            setattr(rules[edit[0]], edit[1], edit[2])
        rc = lib.ltx_change_maps(None if null == 'in' else ctypes.byref(cin), n_maps,
                                 None if null == 'rules' else rules,
                                 None if null == 'out' else ctypes.byref(cout))
        if rc != cx.LT_OK or n_pix == 0:
            for f, b in bufs.items():
                assert cx.same(b, before[f]).all(), f
        return rc
    assert call() == cx.LT_OK
    for f, b in bufs.items():
        b[...] = before[f]
    assert call(null='in') == A and call(null='rules') == A and call(null='out') == A
    assert call(n_pix=-1) == A and call(n_years=-1) == A
    assert call(n_maps=0) == A and call(n_maps=9) == A and call(n_maps=-1) == A
    assert call(use=('vertex', 'val_raw', 'spike')) == A               # no val_fit
    assert call(use=('val_fit', 'val_raw', 'spike')) == A              # no vertex
    assert call(no_year=True) == A
    assert call(stride=P - 1) == A and call(ostride=P - 1) == A
    assert call(use=('val_fit', 'vertex', 'val_raw', 'spike', 'present', 'winner')) == A
    fit_out = ('dsnr', 'rmse', 'n_fit')
    for miss in ('val_raw', 'spike'):
        use = tuple(f for f in ('val_fit', 'vertex', 'val_raw', 'spike') if f != miss)
        assert call(use=use) == A, miss
        for f in fit_out:  # any one of the three outputs asks for both inputs
            assert call(use=use, odrop=tuple(g for g in fit_out if g != f)) == A, (miss, f)
    for field, v in (('delta', 2), ('delta', -1), ('sort', 8), ('sort', -1), ('index_sign', 0),
                     ('index_sign', 2), ('mag_op', _abi.LT_Q_EQ), ('dur_op', _abi.LT_Q_OTHER),
                     ('pre_op', 6), ('mag_op', -1)):
        for m in range(M):
            assert call(edit=(m, field, v)) == A, (m, field, v)
    assert call(edit=(1, 'year_lo', 1992)) == A                        # lo > hi
    assert call(n_years=_abi.LT_MAX_YEARS + 1) == L
    assert call(n_pix=(1 << 28) + 1, stride=1 << 29, ostride=1 << 29) == L
    # nothing to do: LT_OK at once, whatever else is passed
    assert call(n_pix=0) == cx.LT_OK
    assert call(n_pix=0, n_maps=99, use=(), stride=-4, edit=(0, 'sort', 77)) == cx.LT_OK


@pytest.mark.parametrize('P', [0, 1, 255, 256, 257, 70001])
def test_label_counts(lib, P):
    rng = np.random.default_rng(P)
    matched = (rng.random(P) < 0.7).astype(np.uint8) * rng.integers(1, 256, P).astype(np.uint8)
    key = rng.integers(1980, 2020, P).astype(np.int32)
    if P > 3:
        key[:3] = (-2 ** 31, 2 ** 31 - 1, 1979)
        matched[:3] = 1
    for lo, n_bins in ((1985, 1), (1985, 30), (1900, 256), (-2 ** 31, 256), (2 ** 31 - 5, 256)):
        want = cx.counts_reference(matched, key, lo, n_bins)
        assert (cx.host_counts(lib, matched, key, lo, n_bins) == want).all(), (lo, n_bins)
        start = rng.integers(0, 1 << 40, n_bins + 1)
        again = cx.host_counts(lib, matched, key, lo, n_bins, start=start)
        assert (again == cx.counts_reference(matched, key, lo, n_bins, start)).all()
        assert int(want.sum()) == int((matched != 0).sum())
    if P > 3:
        out = cx.counts_reference(matched, key, 1985, 30)
        assert out[30] >= 3  # the three keys planted outside the range land in the last bin


def test_label_counts_argument_checks(lib):
    m, k = np.ones(9, np.uint8), np.full(9, 5, np.int32)
    c = np.full(8, 77, np.uint64)

    def call(mp=m.ctypes.data, kp=k.ctypes.data, n=9, n_bins=4, cp=c.ctypes.data):
        rc = lib.ltx_label_counts(mp, kp, n, 0, n_bins, cp)
        if rc != cx.LT_OK or n == 0:
            assert (c == 77).all()
        return rc
    A = cx.LT_ERR_ARG
    assert call(mp=None) == A and call(kp=None) == A and call(cp=None) == A
    assert call(n=-1) == A and call(n_bins=0) == A and call(n_bins=257) == A
    assert call(n=(1 << 28) + 1) == cx.LT_ERR_LIMIT
    assert call(n=0) == cx.LT_OK and call(n=0, mp=None, n_bins=0) == cx.LT_OK
    assert call() == cx.LT_OK and c[4] == 77 + 9 and (c[:4] == 77).all() and (c[5:] == 77).all()


def test_the_exports_are_declared_and_the_abi_version_stays():
    assert 'lt_change_maps' in _abi.EXPORTS and 'lt_label_counts' in _abi.EXPORTS
    assert _abi.LT_ABI_VERSION == 8
    lib = _abi.load_lib()
    assert lib.lt_abi_version() == 8
    assert hasattr(lib, 'lt_change_maps') and hasattr(lib, 'lt_label_counts')
    hdr = open(os.path.join(cx.ROOT, 'include', 'lt_abi.h')).read()
    assert 'int lt_change_maps(' in hdr and 'int lt_label_counts(' in hdr
    for t in ('lt_change_rule', 'lt_change_in', 'lt_change_out'):
        assert '} %s;' % t in hdr
    assert '#define LT_MAX_CHANGE_MAPS 8' in hdr and _abi.LT_MAX_CHANGE_MAPS == 8
    assert ctypes.sizeof(_abi.LtChangeRule) == 64
    assert ctypes.sizeof(_abi.LtChangeIn) == 80 and ctypes.sizeof(_abi.LtChangeOut) == 80


# ---- LocalJob through the host twins ----

def run_job(root, job, settings, engine, trendline=False, **kw):
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    make_job(root, job, rows=SHAPE[0], cols=SHAPE[1], seed=5, settings=settings)
    j = LocalJob(root, job, on_error='skip', engine=engine, trendline=trendline, **kw)
    return j, j.run()


@pytest.mark.parametrize('mode', ['reference', 'typed'])
def test_job_through_the_host_twins(tmp_path, mode):
    from engine_double import OracleEngine
    from jobfixture import SETTINGS
    root = str(tmp_path)
    _, before = run_job(root, 'before', SETTINGS, OracleEngine(), raster_mode=mode)
    nokey, files0 = run_job(root, 'nokey', SETTINGS, cx.make_twin_engine(), raster_mode=mode)
    assert nokey.change_planes is None and nokey.change_stats is None
    assert file_bytes(files0) == file_bytes(before)   # without the key: what was written before
    plain, _ = run_job(root, 'plain', SETTINGS, cx.make_twin_engine(), trendline=True,
                       raster_mode=mode)
    assert plain._raster_hw == SHAPE
    want, keep = job_reference(plain)
    pl = plain.planes
    # the conditions without which the job tests could pass vacuously
    assert keep.all() and len(keep) == 960
    got_n = {r['name']: int(want['matched'][m].sum()) for m, r in enumerate(JOB_MAPS)}
    assert got_n == JOB_MATCHED
    assert all(n > 0 for n in got_n.values())
    assert all(n < 960 for name, n in got_n.items() if name != 'A')
    n_loss = n_gain = n_zero = 0
    for p in range(960):
        for s in cx.segments(plain.scene.years, pl['val_fit'], pl['vertex'], pl['winner'] >= 0,
                             p)[1]:
            n_loss, n_gain, n_zero = n_loss + (s[3] > 0), n_gain + (s[3] < 0), n_zero + (s[3] == 0)
    assert (n_loss, n_gain, n_zero) == (2564, 2807, 5)

    for trendline in (False, True):
        j, files = run_job(root, 'cm%d' % trendline, dict(SETTINGS, change_maps=JOB_MAPS),
                           cx.make_twin_engine(), trendline=trendline, raster_mode=mode)
        cx.assert_maps({f: t.numpy() for f, t in j.change_planes.items()}, want, 'planes')
        check_change_files(j, files, want, keep, mode)
        assert j.change_stats == expected_stats(want, plain.scene.years)
        assert j.change_s > 0
        rest = {k: v for k, v in files.items() if not k.startswith('change/')}
        if not trendline:  # the other rasters are the job's without the key, byte for byte
            assert file_bytes(rest) == file_bytes(files0)

    # top-level mmu 3: each map loses exactly the patches the sieve's reference finds (and the
    # label rules' rasters theirs, as before); a map's own "mmu": 1 turns its sieve off
    maps = [dict(r, mmu=1) if r['name'] == 'D' else r for r in JOB_MAPS]
    j, files = run_job(root, 'mmu', dict(SETTINGS, change_maps=maps, mmu=3),
                       cx.make_twin_engine(), raster_mode=mode)
    sieved = {f: a.copy() for f, a in want.items()}
    for m, rule in enumerate(JOB_MAPS):
        _, size = sx.reference(want['matched'][m], want['onset_year'][m], SHAPE, 8)
        gone = (size > 0) & (size < 3)
        assert gone.any() and (size >= 3).any(), rule['name']
        assert int(gone.sum()) == JOB_REMOVED[rule['name']]
        if rule['name'] != 'D':
            sieved['matched'][m][gone] = 0
    cx.assert_maps({'matched': j.change_planes['matched'].numpy()},
                   {'matched': sieved['matched']}, 'sieved')
    check_change_files(j, files, sieved, keep, mode)
    assert j.change_stats == expected_stats(sieved, plain.scene.years, before=want)
    assert j.change_stats['D']['removed'] == 0
    assert j.change_stats['A']['removed'] == JOB_REMOVED['A']
