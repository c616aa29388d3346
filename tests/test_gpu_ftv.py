"""Fit to vertex on the MI355X (lt_ftv_tile, lt_ftv.hip): the analysis's spikes and vertices
applied to another series, bit for bit against the reference goldens, the reference's own
vertices2eqns / eqns2fitted_points on second series (tests/golden/ftv_second.npz) and the numpy
restatement over the oracle's lstsq (tests/ftvfixture.py). No tolerances anywhere."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ftvfixture as fx
import golden_io
from land_trendr_amd import _abi
from land_trendr_amd.engine import FTV_FIELDS, get_engine, label_tile
from land_trendr_amd.scene import build_scene, parse_date
from land_trendr_amd.settings import compile_params
from land_trendr_amd.synth import make_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    return get_engine(0)


@pytest.fixture(scope='module')
def fixture():
    return fx.load_fixture()


def dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def run(eng, scene, winner, spike, vertex, vals, fields=FTV_FIELDS):
    out = eng.ftv_tile(scene, dev(eng, winner.astype(np.int16)), dev(eng, spike.astype(np.uint8)),
                       dev(eng, vertex.astype(np.uint8)), dev(eng, vals), fields)
    torch.cuda.synchronize()
    return {f: t.cpu().numpy() for f, t in out.items()}


def assert_planes(out, want, tag, fields=FTV_FIELDS):
    for f in fields:
        m = ~fx.bits_equal(out[f], want[f])
        assert not m.any(), (tag, f, int(m.sum()), np.argwhere(m)[:5].tolist())
    assert (out['status'] == want['status']).all(), tag


@pytest.mark.parametrize('name', golden_io.scene_names())
def test_identity_on_the_golden_scenes(eng, name):
    """The golden flags and the golden values give the golden planes back; label_tile on the
    fitted values gives the golden labels; a second run gives the same bits."""
    g = golden_io.GoldenScene(name)
    winner = fx.rejected_winners(g)
    d = [dev(eng, a) for a in (winner, g.ref['spike'], g.ref['vertex'], g.values)]
    t1 = eng.ftv_tile(g.scene, *d)
    t2 = eng.ftv_tile(g.scene, *d)
    torch.cuda.synchronize()
    out = {f: t.cpu().numpy() for f, t in t1.items()}
    fx.check_golden(g, out, winner)
    for f, t in t2.items():
        a, b = out[f], t.cpu().numpy()
        assert (fx.bits_equal(a, b) if a.dtype.kind == 'f' else a == b).all(), (name, f)
    lab = label_tile(eng, g.scene.years, g.params, t1['val_fit'], d[2], dev(
        eng, (winner >= 0).astype(np.uint8)))
    torch.cuda.synchronize()
    ok = np.array([e == '' for e in g.err])
    R = len(g.rules)
    for f in ('matched', 'class_val', 'onset_year', 'duration', 'magnitude'):
        got, ref = lab[f].cpu().numpy()[:R], g.ref[f]
        m = (~fx.bits_equal(got, ref) if f == 'magnitude' else got != ref) & ok[None, :]
        assert not m.any(), (name, f, int(m.sum()))


@pytest.mark.parametrize('name', fx.FIXTURE_SCENES)
@pytest.mark.parametrize('integer', [True, False])
def test_second_series_equals_the_reference(eng, fixture, name, integer):
    """obs_index int16 for the integer kinds, obs_val for the float kind."""
    g = golden_io.GoldenScene(name)
    winner, spike, vertex, vals, want = fx.fixture_inputs(g, fixture[name], integer)
    assert vals.dtype == (np.int16 if integer else np.float64)
    out = run(eng, g.scene, winner, spike, vertex, vals)
    fx.check_fixture(out, winner, vals, want, (name, integer))


@pytest.fixture(scope='module')
def analysed(eng):
    """make_scene(4099, 30 years) analysed once; a few pixels forced fully masked / to one year."""
    sc = make_scene(4099, n_years=30, k_min=1, k_max=3, mask_prob=0.2, seed=42)
    meta = build_scene(sc.dates, parse_date('2014-07-01'))
    params, _ = compile_params(10, [{'name': 'gd', 'val': 1, 'change_type': 'GD'}])
    valid = sc.valid.clone()
    valid[:, [0, 77, 4098]] = 0
    valid[:, [5, 64, 4097]] = 0
    valid[3, [5, 64, 4097]] = 1
    out = eng.analyze_tile(meta, params, sc.values.to(eng.device), valid.to(eng.device),
                           ('winner', 'spike', 'vertex', 'status'))
    torch.cuda.synchronize()
    return meta, out


def test_after_a_real_analysis_with_strides_and_guards(eng, analysed):
    meta, a = analysed
    Y, P, K = meta.n_years, 4099, meta.n_obs
    st = a['status'].cpu().numpy()
    assert (st & _abi.LT_ST_EMPTY).sum() >= 3 and (st & _abi.LT_ST_SINGLE_YEAR).sum() >= 3
    rng = np.random.default_rng(99)
    second = rng.integers(-32768, 32768, (K, P)).astype(np.int16)
    IS, VS, OS = P + 61, P + 13, P + 29  # row strides of the flag planes, the values, the outputs

    def padded(t, stride, fill):
        buf = torch.full((t.shape[0] + 1, stride), fill, dtype=t.dtype, device=eng.device)
        buf[:t.shape[0], :P] = t
        return buf

    w, s, v = (padded(a[f], IS, 9) for f in ('winner', 'spike', 'vertex'))
    vals = padded(dev(eng, second), VS, 1234)
    # the outputs in one buffer, side by side with a neighbouring guard row after each plane
    outbuf = torch.full((len(FTV_FIELDS), Y + 1, OS), -7.25, dtype=torch.float64,
                        device=eng.device)
    stbuf = torch.full((P + 64,), -3, dtype=torch.int32, device=eng.device)
    out = {f: outbuf[i, :Y, :P] for i, f in enumerate(FTV_FIELDS)}
    out['status'] = stbuf[:P]
    eng.ftv_tile(meta, w[:Y, :P], s[:Y, :P], v[:Y, :P], vals[:K, :P], out=out)
    torch.cuda.synchronize()
    host = outbuf.cpu().numpy()
    assert (host[:, :, P:] == -7.25).all() and (host[:, Y, :] == -7.25).all()
    assert (stbuf[P:].cpu().numpy() == -3).all()
    for t, fill in ((w, 9), (s, 9), (v, 9), (vals, 1234)):
        h = t.cpu().numpy()
        assert (h[:, P:] == fill).all() and (h[-1] == fill).all()
    got = {f: host[i, :Y, :P] for i, f in enumerate(FTV_FIELDS)}
    got['status'] = stbuf[:P].cpu().numpy()
    want = fx.ftv_numpy(meta.years, a['winner'].cpu().numpy(), a['spike'].cpu().numpy(),
                        a['vertex'].cpu().numpy(), second)
    assert_planes(got, want, 'analysed')
    rej = (st & (_abi.LT_ST_EMPTY | _abi.LT_ST_SINGLE_YEAR)) != 0
    assert (got['status'][rej] == st[rej]).all() and (got['status'][~rej] == 0).all()


def test_long_and_gapped_segments_in_one_wave(eng):
    """Y = 40, 130 pixels: lanes whose only vertices are the first and the last point (0, 1 or 3
    spikes, 0-4 absent years and more: m from 5 to 38 with gaps, so the x-set table misses and the
    general lsq_apply runs) beside lanes with a vertex every year and lanes that start late."""
    Y, P = 40, 130
    scene = fx.yearly_scene(Y)
    winner, spike, vertex = fx.handmade(Y, P, Y, seed=40 * 1000 + P)
    ms = [int(((winner[:, p] >= 0) & (spike[:, p] == 0)).sum()) for p in range(0, P, 4)]
    assert min(ms) <= 9 and max(ms) >= 36 and len(set(ms)) > 6, ms
    assert len({int(np.argmax(winner[:, p] >= 0)) for p in range(P)}) > 3
    rng = np.random.default_rng(40)
    for vals in (rng.integers(-3000, 3000, (Y, P)).astype(np.int16),
                 rng.normal(300, 200, (Y, P))):
        out = run(eng, scene, winner, spike, vertex, vals)
        assert_planes(out, fx.ftv_numpy(scene.years, winner, spike, vertex, vals), vals.dtype)


@pytest.mark.parametrize('P', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('Y', [2, 21])
def test_edges(eng, P, Y):
    scene = fx.yearly_scene(Y)
    winner, spike, vertex = fx.handmade(Y, P, Y, seed=Y * 1000 + P)
    rng = np.random.default_rng(P)
    cases = {'zero': np.zeros((Y, P), np.int16),
             'extremes': rng.choice(np.array([32767, -32768, -32767], np.int16), (Y, P)),
             'zero f64': np.zeros((Y, P))}
    for tag, vals in cases.items():
        out = run(eng, scene, winner, spike, vertex, vals)
        assert_planes(out, fx.ftv_numpy(scene.years, winner, spike, vertex, vals), (tag, P, Y))


def test_val_fit_alone_leaves_the_other_buffers_untouched(eng):
    Y, P = 12, 200
    scene = fx.yearly_scene(Y)
    winner, spike, vertex = fx.handmade(Y, P, Y, seed=12)
    vals = np.random.default_rng(12).integers(-900, 900, (Y, P)).astype(np.int16)
    full = run(eng, scene, winner, spike, vertex, vals)
    d = [dev(eng, a) for a in (winner, spike, vertex, vals)]
    # sentinel-filled buffers of the other fields' shapes around the one requested plane
    buf = torch.full((len(FTV_FIELDS), Y, P), 3.5, dtype=torch.float64, device=eng.device)
    k = FTV_FIELDS.index('val_fit')
    stat = torch.full((P,), -5, dtype=torch.int32, device=eng.device)
    out = eng.ftv_tile(scene, *d, out={'val_fit': buf[k]})
    torch.cuda.synchronize()
    assert set(out) == {'val_fit'}
    host = buf.cpu().numpy()
    assert fx.bits_equal(host[k], full['val_fit']).all()
    assert (np.delete(host, k, axis=0) == 3.5).all() and (stat.cpu().numpy() == -5).all()
    one = eng.ftv_tile(scene, *d, fields=('val_fit',))
    torch.cuda.synchronize()
    assert set(one) == {'val_fit', 'status'}
    assert fx.bits_equal(one['val_fit'].cpu().numpy(), full['val_fit']).all()


def _structs(eng, scene, Y, P, K):
    """Valid lt_ftv_tile arguments over guard-surrounded buffers, for the argument checks."""
    t = dict(winner=torch.zeros((Y, P), dtype=torch.int16, device=eng.device),
             spike=torch.zeros((Y, P), dtype=torch.uint8, device=eng.device),
             vertex=torch.zeros((Y, P), dtype=torch.uint8, device=eng.device),
             vals=torch.zeros((K, P), dtype=torch.int16, device=eng.device),
             fvals=torch.zeros((K, P), dtype=torch.float64, device=eng.device),
             out=torch.full((Y, P), 2.5, dtype=torch.float64, device=eng.device),
             status=torch.full((P,), -9, dtype=torch.int32, device=eng.device))
    fin = _abi.LtFtvIn()
    fin.n_pix, fin.stride, fin.obs_stride = P, P, P
    fin.winner = ctypes.cast(t['winner'].data_ptr(), _abi.c_i16p)
    fin.spike = ctypes.cast(t['spike'].data_ptr(), _abi.c_u8p)
    fin.vertex = ctypes.cast(t['vertex'].data_ptr(), _abi.c_u8p)
    fin.obs_index = t['vals'].data_ptr()
    fin.index_type = _abi.LT_T_I16
    tout = _abi.LtTileOut()
    tout.stride = P
    tout.val_fit = ctypes.cast(t['out'].data_ptr(), _abi.c_f64p)
    tout.status = ctypes.cast(t['status'].data_ptr(), _abi.c_i32p)
    return t, fin, tout


def test_argument_errors_launch_nothing(eng):
    Y, P = 6, 70
    scene = fx.yearly_scene(Y)
    t, fin, tout = _structs(eng, scene, Y, P, Y)
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    lib, ctx = eng.lib, eng.ctx

    def call(sc=scene.to_c(), fin=fin, tout=tout, null=None):
        args = [ctypes.byref(sc), ctypes.byref(fin), ctypes.byref(tout)]
        if null is not None:
            args[null] = None
        rc = lib.lt_ftv_tile(ctx, *args, st)
        return rc, lib.lt_last_error(ctx).decode()

    def variant(struct, **kw):
        c = type(struct)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(struct), ctypes.sizeof(struct))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    f64 = ctypes.cast(t['fvals'].data_ptr(), _abi.c_f64p)
    arg_cases = [dict(null=0), dict(null=1), dict(null=2),
                 dict(fin=variant(fin, winner=None)), dict(fin=variant(fin, spike=None)),
                 dict(fin=variant(fin, vertex=None)),
                 dict(fin=variant(fin, stride=P - 1)), dict(fin=variant(fin, obs_stride=P - 1)),
                 dict(tout=variant(tout, stride=P - 1)),
                 dict(fin=variant(fin, obs_val=f64)),                  # both
                 dict(fin=variant(fin, obs_index=None)),               # neither
                 dict(fin=variant(fin, index_type=_abi.LT_T_BOOL)),
                 dict(fin=variant(fin, index_type=-1)), dict(fin=variant(fin, n_pix=-1))]
    for kw in arg_cases:
        rc, msg = call(**kw)
        assert rc == -1 and msg, (kw.keys(), rc, msg)
    # LT_ERR_LIMIT as lt_analyze_tile gives it for the scene
    yrs = (ctypes.c_int32 * 70)(*range(1900, 1970))
    sc = scene.to_c()
    big = [variant(sc, n_years=65, year=ctypes.cast(yrs, _abi.c_i32p)),
           variant(sc, n_obs=_abi.LT_MAX_OBS + 1)]
    far = (ctypes.c_int32 * Y)(*[1900, 1901, 1902, 1903, 1904, 2156])
    big.append(variant(sc, year=ctypes.cast(far, _abi.c_i32p)))
    for s in big:
        rc, msg = call(sc=s)
        assert rc == -4 and msg, (rc, msg)
    assert call(fin=variant(fin, n_pix=0, winner=None))[0] == 0   # LT_OK at once
    torch.cuda.synchronize()
    assert (t['out'].cpu().numpy() == 2.5).all() and (t['status'].cpu().numpy() == -9).all()
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert (t['status'].cpu().numpy() != -9).all()


def test_malformed_flags_set_numeric_and_stay_in_bounds(eng):
    Y, P, K = 9, 131, 9
    scene = fx.yearly_scene(Y)
    winner = np.tile(np.arange(Y, dtype=np.int16)[:, None], (1, P))
    spike = np.zeros((Y, P), np.uint8)
    vertex = np.zeros((Y, P), np.uint8)          # no vertex at all with T = 9
    winner[:, 1::2] = K                          # not an observation: every year absent
    winner[4, 4] = 32767
    winner[2, 6] = -32768
    spike[:, 8] = 1                              # every point a spike
    vertex[:, 10] = 1
    spike[:, 10] = 1                             # vertices only on spikes
    vals = torch.full((K + 1, P + 32), 77, dtype=torch.int16, device=eng.device)
    outbuf = torch.full((len(FTV_FIELDS), Y + 1, P + 32), -1.5, dtype=torch.float64,
                        device=eng.device)
    status = torch.full((P + 32,), -2, dtype=torch.int32, device=eng.device)
    out = {f: outbuf[i, :Y, :P] for i, f in enumerate(FTV_FIELDS)}
    out['status'] = status[:P]
    eng.ftv_tile(scene, dev(eng, winner), dev(eng, spike), dev(eng, vertex), vals[:K, :P], out=out)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert (st[:P] & _abi.LT_ST_NUMERIC).all() and (st[P:] == -2).all()
    host = outbuf.cpu().numpy()
    assert (host[:, :, P:] == -1.5).all() and (host[:, Y, :] == -1.5).all()
    assert (vals.cpu().numpy() == 77).all()
    assert np.isnan(host[0, :Y, 1]).all()        # treated as absent: val_raw NaN


def test_engine_checks_its_tensors(eng):
    from land_trendr_amd.engine import LtError
    Y, P = 5, 10
    scene = fx.yearly_scene(Y)
    w, s, v = (dev(eng, a) for a in fx.handmade(Y, P, Y, seed=1))
    vals = torch.zeros((Y, P), dtype=torch.int16, device=eng.device)
    for bad in (dict(winner=w.to(torch.int32)), dict(spike=s[:, :5]), dict(values=vals[:4]),
                dict(values=vals.cpu()), dict(fields=('spike',)),
                dict(out={'val_fit': torch.zeros((Y, P), device=eng.device)})):
        kw = dict(winner=w, spike=s, vertex=v, values=vals)
        kw.update(bad)
        with pytest.raises(LtError):
            eng.ftv_tile(scene, **kw)


# ---- LocalJob with settings.json ftv_eqns ----

JOB_SETTINGS = {'index_eqn': 'B1 - B2', 'line_cost': 10, 'target_date': '2014-07-01',
                'label_rules': [{'name': 'gd', 'val': 3, 'change_type': 'GD'}]}
FTV_EQNS = {'b3': 'B3', 'sum': 'B1 + B3'}


def make_ftv_job(root, job, settings):
    """A 24 x 20 raster, 6 dates in 4 years, 3 int16 bands, a cloud mask per date (jobfixture's
    naming and geotransform); pixel (0, 0) is valid on one date only, pixel (0, 1) on none."""
    from jobfixture import GT
    from land_trendr_amd.raster import write_geotiff
    rows, cols = 24, 20
    rng = np.random.default_rng(2405)
    rdir = os.path.join(root, job, 'input', 'rasters')
    os.makedirs(rdir, exist_ok=True)
    with open(os.path.join(root, job, 'input', 'settings.json'), 'w') as f:
        json.dump(settings, f)
    for k, (year, doy) in enumerate([(2001, 170), (2001, 200), (2002, 185), (2003, 150),
                                     (2003, 230), (2004, 190)]):
        stem = 'LT5045029_%d_%03d_20120124_104859' % (year, doy)
        img = rng.integers(-3000, 3000, (3, rows, cols)).astype(np.int16)
        write_geotiff(os.path.join(rdir, stem + '_ledaps.tif'), img, geotransform=GT, nodata=None)
        m = (rng.random((rows, cols)) < 0.85).astype(np.uint8)
        m[0, 0] = 1 if k == 2 else 0
        m[0, 1] = 0
        write_geotiff(os.path.join(rdir, stem + '_cloudmask.tif'), m, geotransform=GT,
                      nodata=None)


def expected_ftv_rasters(j, name, planes, winner, ok, mode):
    """The reference's data2raster over the keys 'ftv/<name>/<winner date>-<attr>' a reducer would
    emit for every present year of every pixel the analysis accepts (jobfixture's
    literal_output_rasters, for the FTV keys and for both raster modes)."""
    from land_trendr_amd import ingest, raster
    from land_trendr_amd.geotiff import GeoTiff
    tmpl = GeoTiff(j.rast_fns[0])
    gt = tmpl.geotransform()
    hdt = raster.holder_dtype(tmpl.dtype.newbyteorder('=')) if mode == 'reference' else np.float64
    holders = {}
    for p, w in enumerate(j.grid_wkts()):
        if not ok[p]:
            continue
        x, y = ingest.get_pix_offsets_for_point(gt, *ingest.parse_point_wkt(w))
        for slot in range(winner.shape[0]):
            o = int(winner[slot, p])
            if o < 0:
                continue
            d = j.scene.dates[o].strftime('%Y-%m-%d')
            for attr, f in zip(raster.FTV_ATTRS, FTV_FIELDS):
                key = 'ftv/%s/%s-%s' % (name, d, attr)
                h = holders.get(key)
                if h is None:
                    h = holders[key] = np.full((tmpl.height, tmpl.width), raster.NODATA, hdt)
                h[y, x] = float(planes[f][slot, p])
    if mode == 'reference':
        return {k: raster.gdal_to_byte(h) for k, h in holders.items()}
    return holders


def file_bytes(files):
    out = {}
    for k, (path,) in files.items():
        with open(path, 'rb') as fh:
            out[k] = fh.read()
    return out


@pytest.mark.parametrize('mode,encode', [('reference', 'host'), ('typed', 'device')])
def test_job_writes_the_ftv_rasters(eng, tmp_path, mode, encode):
    from land_trendr_amd.geotiff import GeoTiff
    from land_trendr_amd.job import LocalJob
    from oracle import oracle
    root = str(tmp_path)
    make_ftv_job(root, 'plain', JOB_SETTINGS)
    make_ftv_job(root, 'ftv', dict(JOB_SETTINGS, ftv_eqns=FTV_EQNS))
    kw = dict(tile_pixels=200, raster_mode=mode, on_error='skip', encode=encode)
    plain = LocalJob(root, 'plain', **kw).run()
    j = LocalJob(root, 'ftv', **kw)
    files = j.run()
    # without ftv_eqns: the same file set and bytes as the other keys of the job with them
    rest = {k: v for k, v in files.items() if not k.startswith('ftv/')}
    assert sorted(rest) == sorted(plain) and len(rest) < len(files)
    assert file_bytes(rest) == file_bytes(plain)
    assert not any(k.startswith('ftv/') for k in plain)
    # the host computation: the oracle's analysis of the job's own stack, then the numpy
    # restatement on each equation's values at the oracle's winners
    st = j.stack
    assert list(st['band_numbers']) == [1, 2, 3]
    b = st['bands'].astype(np.int16)
    params, _ = compile_params(JOB_SETTINGS['line_cost'], JOB_SETTINGS['label_rules'])
    exp = oracle.analyze_tile(j.scene, params, (b[:, 0] - b[:, 1]).astype(np.float64),
                              st['valid'])
    ok = exp['status'] == 0
    assert (~ok).sum() >= 2 and ok.sum() > 400
    second = {'b3': b[:, 2], 'sum': (b[:, 0] + b[:, 2]).astype(np.int16)}
    want = {}
    for name, vals in second.items():
        planes = fx.ftv_numpy(j.scene.years, exp['winner'], exp['spike'], exp['vertex'], vals)
        want.update(expected_ftv_rasters(j, name, planes, exp['winner'], ok, mode))
    got = {k: v for k, v in files.items() if k.startswith('ftv/')}
    assert sorted(got) == sorted(want) and len(want) == 2 * 6 * 6
    for k, w in want.items():
        a = GeoTiff(got[k][0]).read()[0]
        assert a.dtype == w.dtype and fx.bits_equal(a, w).all() if mode == 'typed' else \
            np.array_equal(a, w), k
    assert set(j.ftv_s) == set(FTV_EQNS)


def test_analysis_reducer_batch_adds_the_ftv_planes(eng):
    """settings['ftv_eqns'] in the batched reducer: each equation evaluated as index_eqn would be
    and fitted at the vertices the analysis of index_eqn found; absent key: no 'ftv' entry."""
    from land_trendr_amd.engine import TRENDLINE
    from land_trendr_amd.utils import analysis_reducer_batch
    sc = make_scene(333, n_years=14, k_min=1, k_max=2, mask_prob=0.15, seed=8, with_bands=True)
    rng = np.random.default_rng(8)
    b3 = torch.from_numpy(rng.integers(-2000, 2000, (sc.n_obs, 1, 333)).astype(np.int16))
    bands = torch.cat([sc.bands, b3], dim=1).to(eng.device)
    settings = dict(JOB_SETTINGS, ftv_eqns=FTV_EQNS)
    fields = TRENDLINE + ('status',)
    out = analysis_reducer_batch(sc.dates, None, sc.valid.to(eng.device), settings, fields,
                                 bands=bands)
    torch.cuda.synchronize()
    assert set(out['ftv']) == set(FTV_EQNS)
    hb = bands.cpu().numpy()
    flags = [out[f].cpu().numpy() for f in ('winner', 'spike', 'vertex')]
    second = {'b3': hb[:, 2], 'sum': (hb[:, 0] + hb[:, 2]).astype(np.int16)}
    for name, vals in second.items():
        got = {f: t.cpu().numpy() for f, t in out['ftv'][name].items()}
        assert_planes(got, fx.ftv_numpy(out['_scene'].years, *flags, vals), name)
    # the index itself fitted at its own vertices is the analysis's trendline
    again = eng.ftv_tile(out['_scene'], out['winner'], out['spike'], out['vertex'],
                         (bands[:, 0] - bands[:, 1]).contiguous())
    torch.cuda.synchronize()
    okp = (out['status'] == 0).cpu().numpy()
    for f in FTV_FIELDS:
        same = fx.bits_equal(again[f].cpu().numpy(), out[f].cpu().numpy())
        assert same[:, okp].all(), f
    plain = analysis_reducer_batch(sc.dates, None, sc.valid.to(eng.device), JOB_SETTINGS, fields,
                                   bands=bands[:, :2].contiguous())
    assert 'ftv' not in plain
    labels_only = analysis_reducer_batch(sc.dates, None, sc.valid.to(eng.device), settings,
                                         bands=bands)
    assert 'ftv' not in labels_only   # the trendline planes were not requested
