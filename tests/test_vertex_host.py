"""The vertex table on the CPU: the kernel's per-pixel code compiled for the host
(tests/native/vertex_host_check.hip over land_trendr_amd/csrc/lt_vertex.h) against the reference's
own vertex points and Disturbance lists (tests/golden/vertex_table.npz) and a numpy restatement,
bit for bit; the settings key, the ABI, and LocalJob through a CPU engine double whose
vertex_table is that host code. No tolerances anywhere."""
import json
import os

import numpy as np
import pytest

import golden_io
import vertexfixture as vx
from land_trendr_amd import _abi
from land_trendr_amd.utils import disturbances_from_vertices


@pytest.fixture(scope='module')
def lib():
    return vx.load_host()


@pytest.fixture(scope='module')
def fixture():
    return vx.load_fixture()


def golden_table(lib, g, pix, V=None, pad=0):
    r = g.ref
    return vx.run_host(lib, g.scene.years, r['val_fit'][:, pix], r['vertex'][:, pix],
                       winner=r['winner'][:, pix], val_raw=r['val_raw'][:, pix], V=V, pad=pad)


def test_the_fixture_covers_every_accepted_pixel_and_both_ends(fixture):
    n_pix = n_seg = 0
    lo, hi = 1 << 30, 0
    for name in golden_io.scene_names():
        g, fz = golden_io.GoldenScene(name), fixture[name]
        assert list(fz['pix']) == [p for p in range(g.n_pix) if g.err[p] in vx.OK_ERR], name
        seg = np.diff(fz['doff'])
        assert (np.diff(fz['voff']) == seg + 1).all(), name
        n_pix += len(seg)
        n_seg += int(seg.sum())
        lo, hi = min(lo, int(seg.min())), max(hi, int(seg.max()))
    assert (n_pix, n_seg) == (2875, 34163)
    assert lo == 1 and hi >= 20  # pixels with exactly one segment and with at least twenty


@pytest.mark.parametrize('name', golden_io.scene_names())
def test_golden_planes_give_the_reference_vertices_and_disturbances(lib, fixture, name):
    g, fz = golden_io.GoldenScene(name), fixture[name]
    Y = g.scene.n_years
    want, want_dis = vx.fixture_table(fz, Y)
    got = golden_table(lib, g, fz['pix'], pad=3)
    vx.assert_table(got, want, name)
    dis = disturbances_from_vertices(got)
    vx.assert_table(dis, want_dis, name + ' disturbances')


@pytest.mark.parametrize('V', [2, 5])
def test_a_cap_keeps_the_full_count_and_the_first_slots(lib, fixture, V):
    for name in ('c1', 'c5', 'edge'):
        g, fz = golden_io.GoldenScene(name), fixture[name]
        full = golden_table(lib, g, fz['pix'])
        got = golden_table(lib, g, fz['pix'], V=V, pad=5)
        assert (got['n_vertices'] == full['n_vertices']).all(), name
        assert name == 'edge' or (full['n_vertices'] > V).any(), name  # (edge: 2 to 5 vertices)
        for f in vx.PLANES:
            assert vx.same(got[f], full[f][:V]).all(), (name, f)
        # the capped table yields the first V - 1 segments
        dis, dfull = disturbances_from_vertices(got), disturbances_from_vertices(full)
        assert (dis['n_segments'] == np.minimum(dfull['n_segments'], V - 1)).all()
        for f in ('onset_year', 'duration', 'initial_val', 'magnitude'):
            assert vx.same(dis[f], dfull[f][:V - 1]).all(), (name, f)


@pytest.mark.parametrize('Y,P', vx.HAND_SHAPES)
def test_handmade_planes_against_the_numpy_restatement(lib, Y, P):
    for tag, kw in vx.handmade_cases(Y, P, seed=100 + Y):
        want = vx.vertex_numpy(**kw)
        got = vx.run_host(lib, pad=7, **kw)
        vx.assert_table(got, want, (Y, P, tag))
        if tag == 'present' and P >= 5:
            n = want['n_vertices']
            assert n[0] == Y and n[1] == 1 and n[2] == 0  # every year, no flag, no point
            assert want['vertex_year'][0, 3] == kw['years'][Y // 2]  # a late first year
        if tag == 'neither':
            assert (want['n_vertices'] >= 1).all()
    # NaN payloads and -0.0 travel by bits (vx.same would take any NaN for any NaN)
    years, val_fit, val_raw, vertex, present, winner = vx.handmade(Y, P, seed=100 + Y)
    got = vx.run_host(lib, years, val_fit, np.ones_like(vertex), val_raw=val_raw, pad=7)
    assert (got['n_vertices'] == Y).all()
    assert (got['vertex_fit'].view(np.uint64) == val_fit.view(np.uint64)).all()
    assert (got['vertex_raw'].view(np.uint64) == val_raw.view(np.uint64)).all()
    if Y * P > 100:
        assert np.isnan(val_fit).any() and (val_fit.view(np.uint64) == 1 << 63).any()


def test_argument_checks_write_nothing(lib):
    years, val_fit, val_raw, vertex, present, winner = vx.handmade(6, 9, seed=1)
    ok = dict(years=years, val_fit=val_fit, vertex=vertex, val_raw=val_raw, present=present)
    A, L = vx.LT_ERR_ARG, vx.LT_ERR_LIMIT

    def untouched(expect, V=6, **kw):
        got = vx.run_host(lib, expect=expect, V=V, **dict(ok, **kw))
        for f, a in got.items():
            assert (a == vx.GUARD[f]).all(), (kw, f)
    untouched(A, winner=winner)                      # both present and winner
    untouched(A, V=0)
    untouched(A, V=_abi.LT_MAX_YEARS + 1)
    import ctypes
    yrs = np.ascontiguousarray(years)
    keep = [np.ascontiguousarray(a) for a in (val_fit, vertex)]
    bufs = vx.guarded_outputs(6, 9, 0)
    optr = {f: (b[1:].ctypes.data) for f, b in bufs.items()}

    def call(n_pix=9, stride=9, ostride=9, V=6, drop=(), odrop=(), n_years=None, null=None):
        ptr = {'val_fit': keep[0].ctypes.data, 'vertex': keep[1].ctypes.data}
        vin, vout = vx.structs(yrs, n_pix, stride, {k: v for k, v in ptr.items() if k not in drop},
                               ostride, V, {k: v for k, v in optr.items()
                                            if k not in odrop})
        if n_years is not None:
            vin.n_years = n_years
        rc = lib.ltx_vertex_table(None if null == 'in' else ctypes.byref(vin),
                                  None if null == 'out' else ctypes.byref(vout))
        for f, b in bufs.items():
            assert (b == vx.GUARD[f]).all(), f
        return rc
    assert call(null='in') == A and call(null='out') == A
    assert call(drop=('val_fit',), odrop=('vertex_raw',)) == A
    assert call(drop=('vertex',), odrop=('vertex_raw',)) == A
    assert call(stride=8, odrop=('vertex_raw',)) == A
    assert call(ostride=8, odrop=('vertex_raw',)) == A
    assert call() == A                               # vertex_raw without val_raw
    assert call(n_years=_abi.LT_MAX_YEARS + 1, odrop=('vertex_raw',)) == L
    assert call(n_pix=0, stride=0, ostride=0) == vx.LT_OK


def test_settings_key_is_validated():
    from land_trendr_amd.settings import check_vertex_table, load_settings, vertex_cap
    base = {'index_eqn': 'B1', 'line_cost': 10, 'target_date': '2014-07-01'}
    assert vertex_cap(base, 30) is None
    assert vertex_cap(dict(base, vertex_table=True), 30) == 30
    assert vertex_cap(dict(base, vertex_table=3), 30) == 3
    assert vertex_cap(dict(base, vertex_table=64), 30) == 30
    for good in (True, 2, 64):
        assert load_settings(json.dumps(dict(base, vertex_table=good)))['vertex_table'] == good
    for bad in (False, 1, 65, 0, -3, 2.0, '3', None, [3], {}):
        with pytest.raises(ValueError):
            check_vertex_table(dict(base, vertex_table=bad))
        with pytest.raises(ValueError):
            load_settings(dict(base, vertex_table=bad))


def test_the_export_is_declared_and_the_abi_version_stays():
    assert 'lt_vertex_table' in _abi.EXPORTS
    assert _abi.LT_ABI_VERSION == 8
    lib = _abi.load_lib()
    assert lib.lt_abi_version() == 8
    assert hasattr(lib, 'lt_vertex_table')
    hdr = open(os.path.join(vx.ROOT, 'include', 'lt_abi.h')).read()
    assert 'int lt_vertex_table(' in hdr and '} lt_vertex_in;' in hdr and '} lt_vertex_out;' in hdr


# ---- LocalJob through the CPU double ----

def run_job(root, job, settings, **kw):
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    if not os.path.exists(os.path.join(root, job)):
        make_job(root, job, settings=settings)
    j = LocalJob(root, job, tile_pixels=40, on_error='skip', engine=vx.VertexOracleEngine(), **kw)
    return j, j.run()


def file_bytes(files, prefix):
    out = {}
    for k, (path,) in files.items():
        if k.startswith(prefix):
            with open(path, 'rb') as fh:
                out[k] = fh.read()
    return out


def job_table(j, val_fit=None, val_raw=None):
    """The host computation from the job's planes: the numpy restatement on the trendline planes
    (the rejected pixels' winners are -1 there: no vertex)."""
    from land_trendr_amd.settings import vertex_cap
    pl = j.planes
    V = vertex_cap(j.settings, j.scene.n_years)
    return vx.vertex_numpy(j.scene.years, pl['val_fit'] if val_fit is None else val_fit,
                           pl['vertex'], winner=pl['winner'],
                           val_raw=pl['val_raw'] if val_raw is None else val_raw, V=V)


def check_rasters(j, files, table, mode, prefix='vertices/'):
    from land_trendr_amd.geotiff import GeoTiff
    ok = (j.planes['status'] & ~_abi.LT_ST_EMPTY) == 0
    want = vx.expected_vertex_rasters(j, table, ok, mode, prefix)
    got = {k: v for k, v in files.items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want) and want, (sorted(got), sorted(want))
    for k, w in want.items():
        a = GeoTiff(got[k][0]).read()[0]
        assert a.dtype == w.dtype and vx.same(a, w).all(), k
    return want


@pytest.mark.parametrize('cap', [True, 3])
@pytest.mark.parametrize('mode', ['reference', 'typed'])
def test_job_writes_the_vertex_rasters(tmp_path, cap, mode):
    from jobfixture import SETTINGS
    root = str(tmp_path)
    plain, plain_files = run_job(root, 'plain', SETTINGS, raster_mode=mode)
    j, files = run_job(root, 'vt', dict(SETTINGS, vertex_table=cap), raster_mode=mode)
    # every other key is what the job without vertex_table writes, byte for byte
    rest = {k: v for k, v in files.items() if not k.startswith('vertices/')}
    assert sorted(rest) == sorted(plain_files)
    assert file_bytes(rest, '') == file_bytes(plain_files, '')
    table = job_table(j)
    n = table['n_vertices']
    assert (n >= 2).any() and (n > 3).any()
    got = {f: t.numpy() for f, t in j.vertex_planes.items()}
    vx.assert_table(got, table, 'job planes')
    want = check_rasters(j, files, table, mode)
    top = min(int(n.max()), 3 if cap == 3 else j.scene.n_years)
    assert sorted(want) == sorted(
        ['vertices/n_vertices'] + ['vertices/%02d-%s' % (k, a) for k in range(1, top + 1)
                                   for a in ('year', 'val_fit', 'val_raw')])
    # labels only: the same vertices/ files byte for byte, and no trendline plane on the host
    first = file_bytes(files, 'vertices/')
    j2, files2 = run_job(root, 'vt', None, raster_mode=mode, trendline=False)
    assert set(j2.host_trendline) == {'winner'}
    assert not any(k.startswith('trendline/') for k in files2)
    assert file_bytes(files2, 'vertices/') == first and len(first) == len(want)


def test_on_error_skip_leaves_a_rejected_pixel_out(tmp_path):
    """A rule with pre_threshold makes the reference raise AttributeError for every pixel that has
    a segment (pre_threshold_mode 'reference'): under on_error='skip' those pixels emit nothing,
    although their planes hold two or more vertices."""
    from jobfixture import SETTINGS
    rules = SETTINGS['label_rules'] + [{'name': 'pt', 'val': 5, 'change_type': 'GD',
                                        'pre_threshold': ['>', 0]}]
    j, files = run_job(str(tmp_path), 'rej', dict(SETTINGS, label_rules=rules, vertex_table=True))
    bad = (j.planes['status'] & _abi.LT_ST_PRE_THRESHOLD_ATTR) != 0
    assert bad.sum() > 50
    assert not any(k.startswith('vertices/') for k in files)
    assert (j.vertex_planes['n_vertices'].numpy()[bad] == 0).all()
    # the same stack without that rule: those pixels have vertices
    j2, files2 = run_job(str(tmp_path), 'acc', dict(SETTINGS, vertex_table=True))
    assert (j2.vertex_planes['n_vertices'].numpy()[bad] >= 2).all()
    assert 'vertices/n_vertices' in files2


def test_job_with_ftv_eqns_and_vertex_table(tmp_path):
    import ftvfixture
    from jobfixture import SETTINGS
    root = str(tmp_path)
    eqns = {'b2': 'B2', 'sum': 'B1 + B2'}
    j, files = run_job(root, 'both', dict(SETTINGS, vertex_table=True, ftv_eqns=eqns),
                       raster_mode='typed')
    check_rasters(j, files, job_table(j), 'typed')
    b = j.stack['bands']
    second = {'b2': b[:, 1], 'sum': (b[:, 0] + b[:, 1]).astype(b.dtype)}
    pl = j.planes
    for name, vals in second.items():
        f = ftvfixture.ftv_numpy(j.scene.years, pl['winner'], pl['spike'], pl['vertex'], vals)
        table = job_table(j, f['val_fit'], f['val_raw'])
        check_rasters(j, files, table, 'typed', 'ftv/%s/vertices/' % name)
    assert j._ftv_vertex is None


def test_world_size_two_is_refused(tmp_path, monkeypatch):
    from jobfixture import SETTINGS, make_job
    from land_trendr_amd.job import LocalJob
    root = str(tmp_path)
    make_job(root, 'vt', settings=dict(SETTINGS, vertex_table=True))
    monkeypatch.setattr(LocalJob, '_dist', staticmethod(lambda: (object(), 2, 0)))
    with pytest.raises(ValueError, match='one rank'):
        LocalJob(root, 'vt', engine=vx.VertexOracleEngine())
    make_job(root, 'badkey', settings=dict(SETTINGS, vertex_table=1))
    monkeypatch.undo()
    with pytest.raises(ValueError, match='vertex_table'):
        LocalJob(root, 'badkey', engine=vx.VertexOracleEngine())
