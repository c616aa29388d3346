"""The zonal table without a GPU: the host twin of lt_zonal.h (tests/native/zonal_host_check.hip,
the per-pixel code and the argument checks the kernels run) against the numpy reference of
zonalfixture on every case; the argument checks; the exports; and LocalJob on the 24 x 40 job
through a CPU double whose zonal_stats is the twin."""
import ctypes
import os

import numpy as np
import pytest

import changefixture as cx
import zonalfixture as zx
from land_trendr_amd import _abi


@pytest.fixture(scope='module')
def lib():
    return zx.load_host()


@pytest.mark.parametrize('pattern', zx.PATTERNS)
def test_host_twin_equals_the_reference(lib, pattern):
    n = 0
    for P, Z, B in zx.shapes(pattern):
        c = zx.case(pattern, P, Z, B)
        got = zx.host_table(lib, c)
        what = (pattern, P, Z, B)
        if c['start'] is None and c['times'] == 1:
            zx.check_sparse(got, zx.case_sparse(pattern, P, Z, B), what)
        else:
            assert np.array_equal(got, zx.case_dense(pattern, P, Z, B)), what
        n += int((got[..., 0] != 0).sum()) if c['start'] is None else 1
    assert n > 0 or pattern == 'unmatched'


def test_the_cases_hold_what_they_are_for():
    """The conditions without which the case list could pass vacuously."""
    c = zx.case('lane_cells', 257, 300, 30)
    cells = c['zone'].astype(np.int64) * 31 + (c['key'] - c['key_lo'])
    assert all(len(set(cells[w:w + 64])) == 64 for w in (0, 64, 128))
    c = zx.case('one_cell', 70001, 7, 30)
    t = zx.case_dense('one_cell', 70001, 7, 30)
    assert (t[..., 0] != 0).sum() == 1 and t[6, 29, 0] == 70001
    assert t[6, 29, 1] == 70001 * zx.I32_MAX and t[6, 29, 2] == 70001 * 16 * 10 ** 9
    c = zx.case('edges_lo', 16385, 300, 1)
    t = zx.case_dense('edges_lo', 16385, 300, 1)
    assert t[:, 0, 0].sum() == ((c['key'] == zx.I32_MAX) & (c['matched'] != 0)).sum() > 0
    assert t[:, 1, 0].sum() > 0
    c = zx.case('edges', 16385, 300, 1)
    t = zx.case_dense('edges', 16385, 300, 1)
    assert t[300, :, 0].sum() > 0 and t[0, :, 0].sum() > 0 and t[299, :, 0].sum() > 0
    # the two ties round to even; the clamp holds on both sides; NaN is not counted
    one = lambda v: zx.reference([1], [0], [0], 0, 1, 1, value=[v])[0, 0]   # noqa: E731
    assert list(one(0.03125)[2:]) == [0, 1] and list(one(0.09375)[2:]) == [2, 1]
    assert list(one(-0.09375)[2:]) == [-2, 1] and list(one(np.nan)) == [1, 0, 0, 0]
    assert one(np.inf)[2] == 2 ** 34 and one(-1e300)[2] == -2 ** 34 and one(-0.0)[2] == 0
    assert zx.case('start', 65, 7, 1)['start'] is not None
    assert zx.case('null_val', 70001, 7, 30)['value'] is None
    for P, Z, B in ((64, 300, 30), (70001, 300, 256)):
        assert zx.paths(Z, B) == (2,)
    assert zx.paths(7, 30) == (1, 2) and zx.paths(1, 256) == (1, 2) and zx.paths(300, 1) == (1, 2)


def test_null_planes_leave_their_words(lib):
    for pattern, kept in (('null_dur', [1]), ('null_val', [2, 3]), ('null_both', [1, 2, 3])):
        c = zx.case(pattern, 70001, 7, 30)
        got = zx.host_table(lib, c)
        assert np.array_equal(got[..., kept], c['start'][..., kept])
        assert (got[..., 0] != c['start'][..., 0]).any()


def test_argument_checks(lib):
    c = zx.case('mixed', 65, 7, 30)
    arrs = {f: np.array(a) for f, a in zx.planes(c).items()}
    t = np.full(8 * 31 * 4, 77, np.uint64)

    def call(n=65, n_bins=30, n_zones=7, path=0, **null):
        p = {f: (None if f in null else a.ctypes.data) for f, a in arrs.items()}
        return lib.ltx_zonal_stats(p['matched'], p['zone'], p['key'], p['duration'], p['value'],
                                   n, 1985, n_bins, n_zones, path,
                                   None if 'table' in null else t.ctypes.data)
    A = zx.LT_ERR_ARG
    assert call(matched=1) == A and call(zone=1) == A and call(key=1) == A and call(table=1) == A
    assert call(n=-1) == A and call(n_bins=0) == A and call(n_bins=257) == A
    assert call(n_zones=0) == A and call(n_zones=zx.LT_MAX_ZONES + 1) == A
    assert call(path=-1) == A and call(path=3) == A
    assert call(path=1, n_zones=300) == A        # 301 * 31 cells: not an LDS table
    assert call(n=(1 << 28) + 1) == zx.LT_ERR_LIMIT
    assert call(n=0) == zx.LT_OK and call(n=0, matched=1, table=1, n_bins=0, n_zones=0) == zx.LT_OK
    assert (t == 77).all()                       # nothing was added by any of these
    assert call(duration=1, value=1) == zx.LT_OK and not (t == 77).all()
    assert lib.ltx_zonal_path(0, 7, 30) == 1 and lib.ltx_zonal_path(0, 300, 30) == 2
    assert lib.ltx_zonal_path(0, 32, 30) == 1 and lib.ltx_zonal_path(0, 33, 30) == 2
    assert lib.ltx_zonal_path(2, 7, 30) == 2


def test_the_export_is_declared_and_the_abi_version_stays():
    assert 'lt_zonal_stats' in _abi.EXPORTS
    assert _abi.LT_ABI_VERSION == 8
    lib = _abi.load_lib()
    assert lib.lt_abi_version() == 8 and hasattr(lib, 'lt_zonal_stats')
    hdr = open(os.path.join(zx.ROOT, 'include', 'lt_abi.h')).read()
    assert 'int lt_zonal_stats(' in hdr
    assert '#define LT_MAX_ZONES 65536' in hdr and _abi.LT_MAX_ZONES == 65536
    assert len(lib.lt_zonal_stats.argtypes) == 13
    # the Python copies of lt_zonal.h's kZonalLdsCells are the header's value: the twin chooses
    # the LDS path up to exactly that many cells ((n_zones + 1) * 2 cells with one bin)
    assert _abi.LT_ZONAL_LDS_CELLS == zx.LDS_CELLS and zx.LDS_CELLS % 2 == 0
    twin = zx.load_host()
    assert twin.ltx_zonal_path(0, _abi.LT_ZONAL_LDS_CELLS // 2 - 1, 1) == 1
    assert twin.ltx_zonal_path(0, _abi.LT_ZONAL_LDS_CELLS // 2, 1) == 2


# ---- LocalJob through the host twins ----

def run_job(root, job, settings, engine=None, zones=(), trendline=False, **kw):
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    make_job(root, job, rows=zx.SHAPE[0], cols=zx.SHAPE[1], seed=5, settings=settings)
    for z in zones:
        zx.write_zones(root, job, **z)
    j = LocalJob(root, job, on_error='skip', engine=engine or zx.make_twin_engine(),
                 trendline=trendline, **kw)
    return j, j.run()


def published(j):
    """{name: (matched, onset_year, duration, magnitude)} of the finished job's label rules and
    change maps, as numpy: the planes the rasters were made from."""
    def rows(pl, names):
        return {n: tuple(np.asarray(pl[f][i].cpu().numpy())
                         for f in ('matched', 'onset_year', 'duration', 'magnitude'))
                for i, n in enumerate(names)}
    out = rows(j.dev_planes, [r.name for r in j.rules])
    if j.change_planes is not None:
        out.update(rows(j.change_planes, [o['name'] for o in j._change_opts]))
    return out


def check_tables(j, shift, ignore, names):
    """The finished job's tables and CSV files against the reference applied to its planes."""
    index, zone_ids = zx.expected_zones(shift, ignore)
    years = [int(y) for y in j.scene.years]
    lo, B = min(years), max(years) - min(years) + 1
    Z = len(zone_ids)
    assert sorted(j.zonal_stats) == sorted(names) and sorted(j.zonal_files) == sorted(names)
    pl = published(j)
    tdir = os.path.join(j.root, j.job, 'output', 'tables')
    assert sorted(os.listdir(tdir)) == sorted('zonal-%s.csv' % n for n in names)
    for name in names:
        m, on, du, mg = pl[name]
        want = zx.reference(m, index, on, lo, B, Z, du, mg)
        got = j.zonal_stats[name]
        assert got['table'].dtype == np.int64 and np.array_equal(got['table'], want), name
        assert np.array_equal(got['zone_ids'], zone_ids) and got['zone_ids'].dtype == np.int64
        assert np.array_equal(got['years'], np.arange(lo, lo + B))
        assert got['pixel_area'] == 900.0
        assert np.array_equal(got['pixels'], want[..., 0])
        assert np.array_equal(got['area'], want[..., 0] * 900.0)
        # each table's word-0 total is the plane's matched count
        assert int(want[..., 0].sum()) == int((m != 0).sum()) == int(got['pixels'].sum())
        with open(j.zonal_files[name]) as fh:
            text = fh.read()
        assert text == zx.expected_csv(want, zone_ids, np.arange(lo, lo + B), 900.0), name
        full = got['pixels'] > 0
        assert np.isnan(got['mean_duration'][~full]).all()
        assert np.array_equal(got['mean_duration'][full],
                              want[..., 1][full] / want[..., 0][full])
        valued = want[..., 3] > 0
        assert np.array_equal(got['mean_magnitude'][valued],
                              want[..., 2][valued] / 16.0 / want[..., 3][valued])
    return index, zone_ids


@pytest.mark.parametrize('mode', ['reference', 'typed'])
def test_job_through_the_host_twins(tmp_path, mode):
    from jobfixture import SETTINGS
    root = str(tmp_path)
    both = dict(SETTINGS, change_maps=cx.JOB_MAPS, mmu=3)
    rules = [r['name'] for r in SETTINGS['label_rules']]
    maps = [m['name'] for m in cx.JOB_MAPS]
    nokey, files0 = run_job(root, 'nokey', both, raster_mode=mode)
    assert nokey.zonal_stats is None and nokey.zonal_files is None and nokey.zonal_s == 0.0
    assert not os.path.exists(os.path.join(root, 'nokey', 'output', 'tables'))

    opt = {'zones': 'zones.tif', 'ignore': [zx.ZONE_IGNORED]}
    for trendline in (False, True):
        j, files = run_job(root, 'z%d' % trendline, dict(both, zonal_stats=opt),
                           zones=[{}], trendline=trendline, raster_mode=mode)
        index, zone_ids = check_tables(j, 0, (zx.ZONE_IGNORED,), rules + maps)
        assert j.zonal_s > 0
        # the conditions without which this could pass vacuously: the four quadrants in
        # ascending id order, pixels outside every zone, and every table with a pixel in it
        assert list(zone_ids) == sorted(zx.QUADRANT_IDS) and (index == -1).sum() == 2 * 24 + 48
        assert index[0] == 1 and index[39] == 3 and index[23 * 40] == 2 and index[-1] == 0
        for name in rules + maps:
            t = j.zonal_stats[name]['table']
            assert t[..., 0].sum() > 0, name
            if name in ('gd', 'A'):  # (the widest: the sieve leaves the narrow maps few pixels)
                assert t[-1, :, 0].sum() > 0 and (t[:-1, :, 0].sum(axis=1) > 0).all(), name
        # summed over the zones, a change map's table is its per-year count (lt_label_counts)
        for name in maps:
            t = j.zonal_stats[name]
            by_year = j.change_stats[name]['by_year']
            got = {int(y): int(n) for y, n in zip(t['years'], t['pixels'][:, :-1].sum(axis=0))}
            assert {y: got[y] for y in by_year} == by_year, name
            assert sum(got.values()) + int(t['pixels'][:, -1].sum()) == sum(by_year.values())
            assert sum(by_year.values()) == (cx.JOB_MATCHED[name] - cx.JOB_REMOVED[name])
        if not trendline:  # the key writes no raster and changes none
            assert cx.file_bytes(files) == cx.file_bytes(files0)

    # a raster shifted by 5 pixels (grid points fall off it), nothing ignored, the short form,
    # labels only by "of", int32 ids
    j, files = run_job(root, 'shift', dict(both, zonal_stats={'zones': 'z5.tif', 'of': ['labels']}),
                       zones=[dict(name='z5.tif', shift=5, dtype=np.int32)], raster_mode=mode)
    index, zone_ids = check_tables(j, 5, (), rules)
    assert list(zone_ids) == sorted(zx.QUADRANT_IDS + (zx.ZONE_IGNORED,))
    # (pt2val's truncation: the pixel centred half a step before the raster reads its first row)
    grid = index.reshape(zx.SHAPE)
    assert (grid[:4] == -1).all() and (grid[:, :4] == -1).all() and (grid[4:, 4:18] >= 0).all()
    assert cx.file_bytes(files) == cx.file_bytes(files0)
    j, _ = run_job(root, 'short', dict(SETTINGS, zonal_stats='zones.tif'), zones=[{}],
                   raster_mode=mode)
    check_tables(j, 0, (), rules)
    j, _ = run_job(root, 'maps', dict(both, zonal_stats=dict(opt, of=['change_maps'])),
                   zones=[{}], raster_mode=mode)
    check_tables(j, 0, (zx.ZONE_IGNORED,), maps)


def test_zone_rasters_the_job_refuses(tmp_path):
    from engine_double import OracleEngine
    from jobfixture import SETTINGS
    root = str(tmp_path)
    z = dict(SETTINGS, zonal_stats='zones.tif')
    with pytest.raises(ValueError, match='integer zone ids'):
        run_job(root, 'float', z, zones=[dict(dtype=np.float32)])
    with pytest.raises(ValueError, match='no zone raster'):
        run_job(root, 'missing', z)
    with pytest.raises(ValueError, match='band 2'):
        run_job(root, 'band', dict(SETTINGS, zonal_stats={'zones': 'zones.tif', 'band': 2}),
                zones=[{}])
    many = (np.arange(960, dtype=np.int32).reshape(zx.SHAPE) * 100)
    j, _ = run_job(root, 'many', z, zones=[dict(image=many, dtype=np.int32, nodata=None)])
    assert len(j.zonal_stats['gd']['zone_ids']) == 960
    with pytest.raises(RuntimeError, match='zonal_stats needs the HIP engine'):
        run_job(root, 'noengine', z, engine=OracleEngine(), zones=[{}])
    # an absolute path is taken as it is
    path = zx.write_zones(root, 'elsewhere', name='abs.tif')
    j, _ = run_job(root, 'abs', dict(SETTINGS, zonal_stats={'zones': path}))
    assert list(j.zonal_stats['gd']['zone_ids']) == sorted(zx.QUADRANT_IDS + (zx.ZONE_IGNORED,))


def test_more_zone_ids_than_the_limit_are_refused(tmp_path, monkeypatch):
    from jobfixture import SETTINGS
    root = str(tmp_path)
    monkeypatch.setattr(_abi, 'LT_MAX_ZONES', 4)
    with pytest.raises(ValueError, match='more than LT_MAX_ZONES'):
        run_job(root, 'five', dict(SETTINGS, zonal_stats='zones.tif'), zones=[{}])
    j, _ = run_job(root, 'four', dict(SETTINGS, zonal_stats={'zones': 'zones.tif',
                                                             'ignore': [zx.ZONE_IGNORED]}),
                   zones=[{}])
    assert len(j.zonal_stats['gd']['zone_ids']) == 4


def test_world_size_two_is_refused_at_construction(tmp_path, monkeypatch):
    from jobfixture import SETTINGS, make_job
    from land_trendr_amd.job import LocalJob
    root = str(tmp_path)
    make_job(root, 'z', rows=3, cols=3, settings=dict(SETTINGS, zonal_stats='zones.tif'))
    make_job(root, 'bad', rows=3, cols=3, settings=dict(SETTINGS, zonal_stats=7))
    make_job(root, 'plain', rows=3, cols=3, settings=SETTINGS)
    with pytest.raises(ValueError, match='zonal_stats'):
        LocalJob(root, 'bad', engine=zx.make_twin_engine())
    LocalJob(root, 'z', engine=zx.make_twin_engine())
    monkeypatch.setattr(LocalJob, '_dist', staticmethod(lambda: (object(), 2, 0)))
    with pytest.raises(ValueError, match='zonal_stats is supported on one rank only'):
        LocalJob(root, 'z', engine=zx.make_twin_engine())
    LocalJob(root, 'plain', engine=zx.make_twin_engine())  # without the key: no objection
