"""The change maps on the MI355X (lt_change_maps, lt_label_counts, lt_change.hip): the hand-made
cases of changefixture through Engine.change_maps into guarded device buffers against the
independent reference, a large random field against the host twin on every element, the argument
checks, the per-key count against numpy, and LocalJob on the HIP engine. No tolerances anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import changefixture as cx
import sievefixture as sx
from changefixture import (JOB_MAPS, JOB_REMOVED, SHAPE, check_change_files, expected_stats,
                           file_bytes, job_reference)
from land_trendr_amd import _abi
from land_trendr_amd.engine import LtError, get_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    return get_engine(0)


@pytest.fixture(scope='module')
def lib():
    return cx.load_host()


def dev(eng, a):
    return torch.from_numpy(np.array(a, order="C")).to(eng.device)


def host(out):
    torch.cuda.synchronize()
    return {f: t.cpu().numpy() for f, t in out.items()}


def run_dev(eng, rules, years, val_fit, vertex, present=None, winner=None, val_raw=None,
            spike=None, pad=0, fields=None, launches=1):
    """Engine.change_maps on planes in rows of P + pad, the outputs in guarded device buffers
    (changefixture.guarded_outputs); checks the guards after each launch, returns the written
    part of each."""
    Y, P = val_fit.shape
    M = len(rules)
    ins = {}
    for f, a, dt in (('val_fit', val_fit, np.float64), ('vertex', vertex, np.uint8),
                     ('val_raw', val_raw, np.float64), ('present', present, np.uint8),
                     ('winner', winner, np.int16), ('spike', spike, np.uint8)):
        if a is not None:
            ins[f] = dev(eng, cx.padded(np.ascontiguousarray(a, dt), pad))[:, :P]
    if fields is None:
        fields = cx.default_fields(val_raw is not None and spike is not None)
    res = []
    for _ in range(launches):
        bufs = {f: dev(eng, b) for f, b in cx.guarded_outputs(M, P, pad, fields).items()}
        out = {f: (b[pad + 1:pad + 1 + P] if f in cx.PIX_FIELDS else b[1:M + 1, :P])
               for f, b in bufs.items()}
        eng.change_maps(years, rules, ins['val_fit'], ins['vertex'], ins.get('present'),
                        ins.get('winner'), ins.get('val_raw'), ins.get('spike'), out=out)
        res.append(cx.check_guards(host(bufs), M, P, pad))
    return res


@pytest.mark.parametrize('shape', ['%dx%d' % s for s in cx.SHAPES])
def test_handmade_cases_against_the_reference(eng, shape):
    tags = [t for t in cx.case_tags() if t.startswith(shape + '-')]
    assert tags
    for tag in tags:
        rules, kw = cx.case(tag)
        first, second = run_dev(eng, rules, pad=7, launches=2, **kw)
        cx.assert_maps(first, cx.case_reference(tag), tag)
        cx.assert_maps(second, first, (tag, 'second launch'))


def test_partial_outputs_and_no_fit_inputs(eng):
    rules, kw = cx.case('33x257-loss-sorts-winner-fit')
    if 'val_raw' not in kw:
        kw = dict(kw, val_raw=cx._planes(33, 257, False)[2], spike=cx._planes(33, 257, False)[4])
    want = cx.reference(rules=rules, **kw)
    six = {f: a for f, a in want.items() if f not in ('dsnr', 'rmse', 'n_fit')}
    bare = {k: v for k, v in kw.items() if k not in ('val_raw', 'spike')}
    cx.assert_maps(run_dev(eng, rules, pad=3, **bare)[0], six, 'no inputs')
    cx.assert_maps(run_dev(eng, rules, pad=3, fields=tuple(six), **kw)[0], six, 'no outputs')
    cx.assert_maps(run_dev(eng, rules, pad=3, fields=('matched', 'rmse'), **kw)[0],
                   {f: want[f] for f in ('matched', 'rmse')}, 'two outputs')
    out = eng.change_maps(kw['years'], rules, dev(eng, kw['val_fit']), dev(eng, kw['vertex']),
                          winner=dev(eng, kw['winner']))
    cx.assert_maps(host(out), six, 'allocated by the engine')


@pytest.fixture(scope='module')
def field(eng):
    kw = cx.random_field(1024 * 1024, 30, seed=11)
    return kw, {f: dev(eng, a) for f, a in kw.items() if f != 'years'}


@pytest.mark.parametrize('M', [8, 1])
def test_a_megapixel_field_against_the_host_twin(eng, lib, field, M):
    kw, ins = field
    rules = cx.EIGHT[:M]
    want = cx.run_host(lib, rules, **kw)
    assert (want['matched'].sum(axis=1) > 0).all() and np.isfinite(want['rmse']).all()
    got = host(eng.change_maps(kw['years'], rules, ins['val_fit'], ins['vertex'],
                               winner=ins['winner'], val_raw=ins['val_raw'], spike=ins['spike']))
    cx.assert_maps(got, want, ('field', M))


def test_argument_errors_launch_nothing(eng):
    Y, P, M = 6, 70, 3
    years, val_fit, val_raw, vertex, spike, present, winner = cx.handmade(Y, P, seed=1)
    yrs = np.ascontiguousarray(years)
    ins = {'val_fit': dev(eng, val_fit), 'vertex': dev(eng, vertex), 'val_raw': dev(eng, val_raw),
           'present': dev(eng, present), 'winner': dev(eng, winner), 'spike': dev(eng, spike)}
    guards = cx.guarded_outputs(M, P, 0, cx.MAP_FIELDS + cx.PIX_FIELDS)
    bufs = {f: dev(eng, b) for f, b in guards.items()}
    optr = {f: b[1:].data_ptr() for f, b in bufs.items()}
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    good = [{'delta': 'loss'}, {'delta': 'gain', 'year': [1990, 1991]},
            {'delta': 'loss', 'mag': ['>', 1]}]

    def call(n_pix=P, stride=P, ostride=P, n_maps=M, n_years=None, null=None, odrop=(),
             use=('val_fit', 'vertex', 'val_raw', 'present', 'spike'), edit=None):
        cin, cout = cx.structs(yrs, n_pix, stride, {f: ins[f].data_ptr() for f in use}, ostride,
                               {f: a for f, a in optr.items() if f not in odrop})
        if n_years is not None:
            cin.n_years = n_years
        rules = cx.c_rules(good)
        if edit:
            setattr(rules[edit[0]], edit[1], edit[2])
        rc = eng.lib.lt_change_maps(eng.ctx, None if null == 'in' else ctypes.byref(cin), n_maps,
                                    None if null == 'rules' else rules,
                                    None if null == 'out' else ctypes.byref(cout), st)
        torch.cuda.synchronize()
        for f, b in bufs.items():  # nothing was launched: every guard value is intact
            assert cx.same(b.cpu().numpy(), guards[f]).all(), f
        return rc
    A, L = cx.LT_ERR_ARG, cx.LT_ERR_LIMIT
    assert call(null='in') == A and call(null='rules') == A and call(null='out') == A
    assert call(n_pix=-1) == A and call(n_years=-1) == A
    assert call(n_maps=0) == A and call(n_maps=9) == A
    assert call(use=('vertex', 'val_raw', 'spike')) == A
    assert call(use=('val_fit', 'val_raw', 'spike')) == A
    assert call(stride=P - 1) == A and call(ostride=P - 1) == A
    assert call(use=('val_fit', 'vertex', 'val_raw', 'spike', 'present', 'winner')) == A
    assert call(use=('val_fit', 'vertex', 'spike')) == A
    assert call(use=('val_fit', 'vertex', 'val_raw')) == A
    assert call(use=('val_fit', 'vertex'), odrop=('rmse', 'n_fit')) == A
    for field, v in (('delta', 2), ('sort', 8), ('index_sign', 0), ('mag_op', _abi.LT_Q_EQ),
                     ('dur_op', 9), ('pre_op', -1)):
        assert call(edit=(M - 1, field, v)) == A, (field, v)
    assert call(edit=(1, 'year_lo', 1992)) == A
    assert call(n_years=_abi.LT_MAX_YEARS + 1) == L
    assert call(n_pix=(1 << 28) + 1, stride=1 << 29, ostride=1 << 29) == L
    assert call(n_pix=0) == cx.LT_OK
    with pytest.raises(LtError):  # the Python layer refuses the same before it calls
        eng.change_maps(years, good, ins['val_fit'], ins['vertex'], ins['present'], ins['winner'])
    with pytest.raises(LtError):
        eng.change_maps(years, [], ins['val_fit'], ins['vertex'])
    with pytest.raises(LtError):
        eng.change_maps(years, [{'delta': 'up'}], ins['val_fit'], ins['vertex'])
    with pytest.raises(LtError):
        eng.change_maps(years, good, ins['val_fit'], ins['vertex'],
                        out={'rmse': torch.empty(P, dtype=torch.float64, device=eng.device)})


@pytest.mark.parametrize('P', [0, 1, 255, 256, 257, 70001])
def test_label_counts_against_numpy(eng, P):
    rng = np.random.default_rng(P)
    matched = (rng.random(P) < 0.7).astype(np.uint8) * rng.integers(1, 256, P).astype(np.uint8)
    key = rng.integers(1980, 2020, P).astype(np.int32)
    if P > 3:
        key[:3] = (-2 ** 31, 2 ** 31 - 1, 1979)
        matched[:3] = 1
    m, k = dev(eng, matched), dev(eng, key)
    for lo, n_bins in ((1985, 1), (1985, 30), (1900, 256), (-2 ** 31, 256), (2 ** 31 - 5, 256)):
        want = cx.counts_reference(matched, key, lo, n_bins)
        got = eng.label_counts(m, k, lo, n_bins)
        assert (got.cpu().numpy() == want).all(), (lo, n_bins)
        start = rng.integers(0, 1 << 40, n_bins + 1)
        out = dev(eng, start.astype(np.int64))
        assert eng.label_counts(m, k, lo, n_bins, out=out) is out
        assert (out.cpu().numpy() == cx.counts_reference(matched, key, lo, n_bins, start)).all()
    for bad in (0, 257, True):
        with pytest.raises(LtError):
            eng.label_counts(m, k, 0, bad)


def test_label_counts_argument_errors_launch_nothing(eng):
    m, k = dev(eng, np.ones(9, np.uint8)), dev(eng, np.full(9, 2, np.int32))
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    c = torch.full((5,), 77, dtype=torch.int64, device=eng.device)
    for args in ((None, k.data_ptr(), 9, 0, 4, c.data_ptr()), (m.data_ptr(), None, 9, 0, 4,
                                                               c.data_ptr()),
                 (m.data_ptr(), k.data_ptr(), 9, 0, 4, None),
                 (m.data_ptr(), k.data_ptr(), -1, 0, 4, c.data_ptr()),
                 (m.data_ptr(), k.data_ptr(), 9, 0, 0, c.data_ptr()),
                 (m.data_ptr(), k.data_ptr(), 9, 0, 257, c.data_ptr())):
        assert eng.lib.lt_label_counts(eng.ctx, *args, st) == cx.LT_ERR_ARG
    assert eng.lib.lt_label_counts(eng.ctx, m.data_ptr(), k.data_ptr(), (1 << 28) + 1, 0, 4,
                                   c.data_ptr(), st) == cx.LT_ERR_LIMIT
    assert eng.lib.lt_label_counts(eng.ctx, None, None, 0, 0, 0, None, st) == cx.LT_OK
    torch.cuda.synchronize()
    assert (c.cpu().numpy() == 77).all()
    assert eng.lib.lt_label_counts(eng.ctx, m.data_ptr(), k.data_ptr(), 9, 0, 4, c.data_ptr(),
                                   st) == cx.LT_OK
    torch.cuda.synchronize()
    assert c.cpu().tolist() == [77, 77, 77 + 9, 77, 77]


# ---- LocalJob on the HIP engine ----

def gpu_job(root, job, settings, **kw):
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    make_job(root, job, rows=SHAPE[0], cols=SHAPE[1], seed=5, settings=settings)
    j = LocalJob(root, job, device=0, tile_pixels=400, on_error='skip', **kw)
    return j, j.run()


@pytest.fixture(scope='module')
def plain(tmp_path_factory):
    """The 24 x 40 job without the key through the CPU double, trendline planes kept: what the
    reference is applied to; and its files with and without the trendline."""
    from jobfixture import SETTINGS, make_job
    from land_trendr_amd.job import LocalJob
    root = str(tmp_path_factory.mktemp('plain'))
    make_job(root, 'plain', rows=SHAPE[0], cols=SHAPE[1], seed=5, settings=SETTINGS)
    j = LocalJob(root, 'plain', on_error='skip', engine=cx.make_twin_engine(), raster_mode='typed')
    j.run()
    return j


def test_job_writes_the_change_rasters(eng, plain, tmp_path):
    from jobfixture import SETTINGS
    root = str(tmp_path)
    want, keep = job_reference(plain)
    settings = dict(SETTINGS, change_maps=JOB_MAPS)
    seen = {}
    for mode, encode in (('reference', 'host'), ('typed', 'device'), ('typed', 'host')):
        for trendline in (False, True):
            job = 'cm_%s_%s_%d' % (mode, encode, trendline)
            j, files = gpu_job(root, job, settings, trendline=trendline, raster_mode=mode,
                               encode=encode)
            if not trendline:
                assert set(j.host_trendline) == {'winner'}  # no binary64 plane left the GPU
            cx.assert_maps(host(j.change_planes), want, job)
            check_change_files(j, files, want, keep, mode)
            assert j.change_stats == expected_stats(want, plain.scene.years)
            data = file_bytes({k: v for k, v in files.items() if k.startswith('change/')})
            # the same bytes with and without the trendline, and from either encoder
            assert seen.setdefault(mode, data) == data, job
            if encode == 'device':
                assert j.encode_stats['device'] >= len(data)


def test_job_with_mmu_sieves_every_map(eng, plain, tmp_path):
    from jobfixture import SETTINGS
    want, keep = job_reference(plain)
    j, files = gpu_job(str(tmp_path), 'mmu', dict(SETTINGS, change_maps=JOB_MAPS, mmu=3),
                       trendline=False, raster_mode='typed')
    sieved = {f: a.copy() for f, a in want.items()}
    for m, rule in enumerate(JOB_MAPS):
        _, size = sx.reference(want['matched'][m], want['onset_year'][m], SHAPE, 8)
        gone = (size > 0) & (size < 3)
        assert gone.any() and (size >= 3).any() and int(gone.sum()) == JOB_REMOVED[rule['name']]
        sieved['matched'][m][gone] = 0
    cx.assert_maps({'matched': host(j.change_planes)['matched']}, {'matched': sieved['matched']},
                   'sieved')
    check_change_files(j, files, sieved, keep, 'typed')
    assert j.change_stats == expected_stats(sieved, plain.scene.years, before=want)


def test_job_without_the_key_writes_what_it_wrote_before(eng, plain, tmp_path):
    """No key: no change plane, no change raster, and the label rasters' bytes are those of the
    job with the key (which the key must not touch) and of the CPU double's run."""
    from jobfixture import SETTINGS
    from land_trendr_amd.geotiff import GeoTiff
    from land_trendr_amd.raster import label_rasters
    root = str(tmp_path)
    j0, files0 = gpu_job(root, 'nokey', SETTINGS, trendline=False, raster_mode='typed')
    assert j0.change_planes is None and j0.change_stats is None
    assert not any(k.startswith('change/') for k in files0)
    j1, files1 = gpu_job(root, 'key', dict(SETTINGS, change_maps=JOB_MAPS[:2]), trendline=False,
                         raster_mode='typed')
    rest = {k: v for k, v in files1.items() if not k.startswith('change/')}
    assert sorted(rest) == sorted(files0) and file_bytes(rest) == file_bytes(files0)
    exp = label_rasters(plain.planes, plain.rules, SHAPE, GeoTiff(j0.rast_fns[0]).dtype.newbyteorder('='),
                        'typed')
    assert sorted(exp) == sorted(files0)
    for k, w in exp.items():
        a = GeoTiff(files0[k][0]).read()[0]
        assert a.dtype == w.dtype and cx.same(a, w).all(), k
