"""The vertex table on the MI355X (lt_vertex_table, lt_vertex.hip): each pixel's vertices compacted
from the planes a real analysis wrote, bit for bit against the reference's own vertex points
(tests/golden/vertex_table.npz), against the host twin on hand-made planes with padded strides and
guard values, the argument checks, and LocalJob. No tolerances anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import golden_io
import vertexfixture as vx
from land_trendr_amd import _abi
from land_trendr_amd.engine import LtError, get_engine
from land_trendr_amd.utils import disturbances_from_vertices

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    return get_engine(0)


@pytest.fixture(scope='module')
def lib():
    return vx.load_host()


@pytest.fixture(scope='module')
def fixture():
    return vx.load_fixture()


def dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def host(out):
    torch.cuda.synchronize()
    return {f: t.cpu().numpy() for f, t in out.items()}


@pytest.mark.parametrize('name', golden_io.scene_names())
def test_analysis_then_vertex_table_gives_the_reference_vertices(eng, fixture, name):
    g, fz = golden_io.GoldenScene(name), fixture[name]
    fields = ('winner', 'val_fit', 'val_raw', 'vertex', 'status')
    a = eng.analyze_tile(g.scene, g.params, dev(eng, g.values), dev(eng, g.valid), fields)
    args = (g.scene.years, a['val_fit'], a['vertex'])
    kw = dict(winner=a['winner'], val_raw=a['val_raw'])
    t1 = eng.vertex_table(*args, **kw)
    t2 = eng.vertex_table(*args, **kw)
    got, again = host(t1), host(t2)
    want, want_dis = vx.fixture_table(fz, g.scene.n_years)
    pix = fz['pix']
    vx.assert_table({f: v[..., pix] for f, v in got.items()}, want, name)
    dis = disturbances_from_vertices({f: t[..., dev(eng, pix.astype(np.int64))]
                                      for f, t in t1.items()})
    vx.assert_table(dis, want_dis, name + ' disturbances')
    for f in got:  # a second launch differs in no element (floats by their bits)
        a1, a2 = got[f], again[f]
        if a1.dtype.kind == 'f':
            a1, a2 = a1.view(np.uint64), a2.view(np.uint64)
        assert (a1 == a2).all(), (name, f)


def run_dev(eng, years, val_fit, vertex, present=None, winner=None, val_raw=None, V=None, pad=0):
    """Engine.vertex_table on planes in rows of P + pad, the outputs in guarded device buffers
    (vertexfixture.guarded_outputs); checks the guards, returns the written part."""
    Y, P = val_fit.shape
    V = Y if V is None else V
    ins = {}
    for f, a, dt in (('val_fit', val_fit, np.float64), ('vertex', vertex, np.uint8),
                     ('val_raw', val_raw, np.float64), ('present', present, np.uint8),
                     ('winner', winner, np.int16)):
        if a is not None:
            ins[f] = dev(eng, vx.padded(np.ascontiguousarray(a, dt), pad, 0)[0])[:, :P]
    bufs = {f: dev(eng, b) for f, b in
            vx.guarded_outputs(V, P, pad, raw=val_raw is not None).items()}
    out = {f: (b[pad + 1:pad + 1 + P] if f == 'n_vertices' else b[1:V + 1, :P])
           for f, b in bufs.items()}
    eng.vertex_table(years, ins['val_fit'], ins['vertex'], ins.get('present'), ins.get('winner'),
                     ins.get('val_raw'), V, out=out)
    return vx.check_guards(host(bufs), V, P, pad)


@pytest.mark.parametrize('Y,P', vx.HAND_SHAPES + ((30, 63), (30, 64), (5, 4099)))
def test_handmade_planes_against_the_host_twin(eng, lib, Y, P):
    for tag, kw in vx.handmade_cases(Y, P, seed=100 + Y):
        for V in sorted({1, min(2, Y), kw.get('V', Y), Y}):
            kv = dict(kw, V=V)
            want = vx.run_host(lib, pad=7, **kv)
            got = run_dev(eng, pad=7, **kv)
            vx.assert_table(got, want, (Y, P, tag, V))
            for f in ('vertex_fit', 'vertex_raw'):  # NaN payloads and -0.0: the same bits
                if f in got:
                    assert (got[f].view(np.uint64) == want[f].view(np.uint64)).all(), (tag, V, f)
            if P <= 130:
                vx.assert_table(got, vx.vertex_numpy(**kv), (Y, P, tag, V, 'numpy'))


def test_argument_errors_launch_nothing(eng):
    Y, P, V = 6, 70, 6
    years, val_fit, val_raw, vertex, present, winner = vx.handmade(Y, P, seed=1)
    yrs = np.ascontiguousarray(years)
    ins = {'val_fit': dev(eng, val_fit), 'vertex': dev(eng, vertex), 'val_raw': dev(eng, val_raw),
           'present': dev(eng, present), 'winner': dev(eng, winner)}
    bufs = {f: dev(eng, b) for f, b in vx.guarded_outputs(V, P, 0).items()}
    optr = {f: b[1:].data_ptr() for f, b in bufs.items()}
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)

    def call(n_pix=P, stride=P, ostride=P, V=V, use=('val_fit', 'vertex', 'val_raw', 'present'),
             odrop=(), n_years=None, null=None):
        vin, vout = vx.structs(yrs, n_pix, stride, {f: ins[f].data_ptr() for f in use}, ostride,
                               V, {f: a for f, a in optr.items() if f not in odrop})
        if n_years is not None:
            vin.n_years = n_years
        rc = eng.lib.lt_vertex_table(eng.ctx, None if null == 'in' else ctypes.byref(vin),
                                     None if null == 'out' else ctypes.byref(vout), st)
        torch.cuda.synchronize()
        for f, b in bufs.items():  # nothing was launched: every guard value is intact
            assert (b.cpu().numpy() == vx.GUARD[f]).all(), f
        return rc
    A, L = vx.LT_ERR_ARG, vx.LT_ERR_LIMIT
    assert call(null='in') == A and call(null='out') == A
    assert call(use=('vertex', 'val_raw')) == A                      # no val_fit
    assert call(use=('val_fit', 'val_raw')) == A                     # no vertex
    assert call(stride=P - 1) == A and call(ostride=P - 1) == A
    assert call(use=('val_fit', 'vertex', 'val_raw', 'present', 'winner')) == A
    assert call(use=('val_fit', 'vertex')) == A                      # vertex_raw without val_raw
    assert call(V=0) == A and call(V=_abi.LT_MAX_YEARS + 1) == A
    assert call(n_years=_abi.LT_MAX_YEARS + 1) == L
    assert call(n_pix=0) == vx.LT_OK
    with pytest.raises(LtError):  # the Python layer refuses the same before it calls
        eng.vertex_table(years, ins['val_fit'], ins['vertex'], ins['present'], ins['winner'])


def test_analysis_reducer_batch_adds_the_vertex_tables(eng):
    """settings['vertex_table'] in the batched reducer: the analysis's table and, per FTV equation,
    that equation's; only the fields asked for come back; absent key: no table."""
    from jobfixture import SETTINGS
    from land_trendr_amd.engine import LABELS, TRENDLINE
    from land_trendr_amd.synth import make_scene
    from land_trendr_amd.utils import analysis_reducer_batch
    sc = make_scene(333, n_years=14, k_min=1, k_max=2, mask_prob=0.15, seed=8, with_bands=True)
    bands, valid = sc.bands.to(eng.device), sc.valid.to(eng.device)
    full = analysis_reducer_batch(sc.dates, None, valid, dict(SETTINGS, ftv_eqns={'b2': 'B2'}),
                                  TRENDLINE + ('status',), bands=bands)
    years = full['_scene'].years
    assert 'vertex_table' not in full and 'vertex_table' not in full['ftv']['b2']
    want = {f: t.cpu().numpy() for f, t in full.items() if f in TRENDLINE}
    wftv = {f: t.cpu().numpy() for f, t in full['ftv']['b2'].items()}
    for cap, V in ((True, len(years)), (4, 4)):
        settings = dict(SETTINGS, vertex_table=cap, ftv_eqns={'b2': 'B2'})
        out = analysis_reducer_batch(sc.dates, None, valid, settings, TRENDLINE + ('status',),
                                     bands=bands)
        vx.assert_table(host(out['vertex_table']), vx.vertex_numpy(
            years, want['val_fit'], want['vertex'], winner=want['winner'],
            val_raw=want['val_raw'], V=V), ('analysis', cap))
        vx.assert_table(host(out['ftv']['b2']['vertex_table']), vx.vertex_numpy(
            years, wftv['val_fit'], want['vertex'], winner=want['winner'],
            val_raw=wftv['val_raw'], V=V), ('ftv', cap))
        # labels only: the table all the same, and no plane that was not asked for
        lab = analysis_reducer_batch(sc.dates, None, valid, settings, bands=bands)
        assert set(lab) == set(LABELS) | {'status', 'vertex_table', '_scene', '_rules'}
        vx.assert_table(host(lab['vertex_table']), host(out['vertex_table']), ('labels', cap))


# ---- LocalJob on the HIP engine ----

def gpu_job(root, job, settings, **kw):
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    make_job(root, job, settings=settings)
    j = LocalJob(root, job, device=0, tile_pixels=40, on_error='skip', **kw)
    return j, j.run()


def host_job(root, job, settings):
    """The same stack through the CPU double with the trendline planes: the host computation."""
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    make_job(root, job, settings=settings)
    j = LocalJob(root, job, tile_pixels=40, on_error='skip', raster_mode='typed',
                 engine=vx.VertexOracleEngine())
    j.run()
    return j


def check_files(j, files, table, ok, mode, prefix):
    from land_trendr_amd.geotiff import GeoTiff
    want = vx.expected_vertex_rasters(j, table, ok, mode, prefix)
    got = {k: v for k, v in files.items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want) and want
    for k, w in want.items():
        a = GeoTiff(got[k][0]).read()[0]
        assert a.dtype == w.dtype and vx.same(a, w).all(), k
    return want


def test_labels_only_job_writes_the_vertex_rasters(eng, tmp_path):
    from jobfixture import SETTINGS
    from land_trendr_amd.settings import vertex_cap
    root = str(tmp_path)
    settings = dict(SETTINGS, vertex_table=True)
    h = host_job(root, 'host', settings)
    pl = h.planes
    ok = (pl['status'] & ~_abi.LT_ST_EMPTY) == 0
    table = vx.vertex_numpy(h.scene.years, pl['val_fit'], pl['vertex'], winner=pl['winner'],
                            val_raw=pl['val_raw'], V=vertex_cap(settings, h.scene.n_years))
    seen = {}
    for mode, encode in (('reference', 'host'), ('typed', 'device')):
        for trendline in (False, True):
            job = 'gpu_%s_%d' % (mode, trendline)
            j, files = gpu_job(root, job, settings, trendline=trendline, raster_mode=mode,
                               encode=encode)
            if not trendline:
                assert set(j.host_trendline) == {'winner'}  # no binary64 plane left the GPU
                assert not any(k.startswith('trendline/') for k in files)
            vx.assert_table(host(j.vertex_planes), table, job)
            want = check_files(j, files, table, ok, mode, 'vertices/')
            data = {}
            for k in want:
                with open(files[k][0], 'rb') as fh:
                    data[k] = fh.read()
            # the labels-only job's files are the trendline job's, byte for byte
            assert seen.setdefault(mode, data) == data, job


def test_job_with_ftv_eqns_and_vertex_table(eng, tmp_path):
    import ftvfixture
    from jobfixture import SETTINGS
    root = str(tmp_path)
    eqns = {'b2': 'B2', 'sum': 'B1 + B2'}
    settings = dict(SETTINGS, vertex_table=3, ftv_eqns=eqns)
    h = host_job(root, 'host', dict(SETTINGS, vertex_table=3))
    pl = h.planes
    ok = (pl['status'] & ~_abi.LT_ST_EMPTY) == 0
    j, files = gpu_job(root, 'gpu', settings, raster_mode='typed')
    table = vx.vertex_numpy(h.scene.years, pl['val_fit'], pl['vertex'], winner=pl['winner'],
                            val_raw=pl['val_raw'], V=3)
    check_files(j, files, table, ok, 'typed', 'vertices/')
    b = j.stack['bands']
    for name, vals in (('b2', b[:, 1]), ('sum', (b[:, 0] + b[:, 1]).astype(b.dtype))):
        f = ftvfixture.ftv_numpy(h.scene.years, pl['winner'], pl['spike'], pl['vertex'], vals)
        t = vx.vertex_numpy(h.scene.years, f['val_fit'], pl['vertex'], winner=pl['winner'],
                            val_raw=f['val_raw'], V=3)
        check_files(j, files, t, ok, 'typed', 'ftv/%s/vertices/' % name)
    assert j._ftv_vertex is None
