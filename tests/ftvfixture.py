"""Shared pieces of the fit-to-vertex tests (tests/test_ftv_host.py, tests/test_gpu_ftv.py): a
numpy restatement of lt_ftv_tile's definition over the oracle's emulated lstsq, the host twin's
loader, the committed reference fixture, and hand-made flag planes."""
import ctypes
import os

import numpy as np

import golden_io
from land_trendr_amd import _abi
from land_trendr_amd.index_eqn import DTYPES
from land_trendr_amd.scene import build_scene, parse_date
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTVCHECK = os.path.join(ROOT, 'tests', 'native', 'build', 'liblt_ftvcheck.so')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'ftv_second.npz')
FTV_FIELDS = _abi.FTV_FIELDS
FIT_FIELDS = FTV_FIELDS[1:]  # every field but val_raw
FIXTURE_SCENES = ('c1', 'c3', 'edge', 'ties2')
OK_ERR = ('', 'label:AttributeError')


def bits_equal(a, b):
    """Bitwise float equality, any NaN equal to any NaN."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def ftv_numpy(years, winner, spike, vertex, values):
    """lt_ftv_tile's definition, pixel by pixel: vertices2eqns + eqns2fitted_points as
    oracle/lt_oracle.c restates them, the least squares through oracle.lstsq. winner / spike /
    vertex [Y, P], values [K, P] (any real dtype). The first present point must be a vertex (after
    an analysis it is). Returns the six planes ([Y, P] float64, NaN where undefined) + 'status'."""
    years = np.asarray(years, np.int64)
    Y, P = winner.shape
    K = values.shape[0]
    out = {f: np.full((Y, P), np.nan) for f in FTV_FIELDS}
    status = np.zeros(P, np.int32)
    for p in range(P):
        ys = [y for y in range(Y) if 0 <= winner[y, p] < K]
        raw = np.array([float(values[winner[y, p], p]) for y in ys], np.float64)
        for y, v in zip(ys, raw):
            out['val_raw'][y, p] = v
        T = len(ys)
        if T < 2:
            status[p] |= _abi.LT_ST_EMPTY if T == 0 else _abi.LT_ST_SINGLE_YEAR
            continue
        x = (years[ys] - years[ys[0]]).astype(np.float64)
        sp = [bool(spike[y, p]) for y in ys]
        ns = [t for t in range(T) if not sp[t]]          # the fitting series
        vt = [t for t in ns if vertex[ys[t], p]]         # its vertices
        eq = {}
        for q in range(len(vt) - 1):
            pts = [t for t in ns if vt[q] <= t <= vt[q + 1]]
            rc, m, b, _ = oracle.lstsq(x[pts], raw[pts])
            if rc < 0:
                status[p] |= _abi.LT_ST_NUMERIC
            eq[vt[q]] = (np.float64(m), np.float64(b))
        eq[vt[-1]] = eq[vt[-2]]
        right, cur = [], None
        for t in range(T):
            if t in eq:
                cur = eq[t]
            right.append(cur)
        for t, y in enumerate(ys):
            rm, rb = right[t]
            fm, fb = rm, rb
            fv = (rm * x[t]) + rb
            if t > 0 and not (right[t - 1][0] == rm and right[t - 1][1] == rb):
                lm, lb = right[t - 1]
                fl = (lm * x[t]) + lb
                rawv = np.nan if sp[t] else raw[t]
                if abs(fl - rawv) <= abs(fv - rawv):
                    fv, fm, fb = fl, lm, lb
            for f, v in zip(FIT_FIELDS, (fv, fm, fb, rm, rb)):
                out[f][y, p] = v
    out['status'] = status
    return out


def load_host():
    """The host twin (tests/native/ftv_host_check.hip), built by __graft_entry__.build()."""
    if not os.path.exists(FTVCHECK):
        raise RuntimeError('host twin not built: run __graft_entry__.build()')
    L = ctypes.CDLL(FTVCHECK)
    L.ltx_ftv_tile.argtypes = [ctypes.POINTER(_abi.LtScene), ctypes.POINTER(_abi.LtFtvIn),
                               ctypes.POINTER(_abi.LtTileOut)]
    return L


def run_host(lib, scene, winner, spike, vertex, values, fields=FTV_FIELDS):
    """ltx_ftv_tile on numpy planes: values float64 (obs_val) or an index raster (obs_index)."""
    winner = np.ascontiguousarray(winner, np.int16)
    spike = np.ascontiguousarray(spike, np.uint8)
    vertex = np.ascontiguousarray(vertex, np.uint8)
    values = np.ascontiguousarray(values)
    Y, P = winner.shape
    out = {f: np.full((Y, P), 7.5) for f in fields}
    out['status'] = np.full(P, -1, np.int32)
    fin = _abi.LtFtvIn()
    fin.n_pix, fin.stride, fin.obs_stride = P, P, P
    fin.winner = winner.ctypes.data_as(_abi.c_i16p)
    fin.spike = spike.ctypes.data_as(_abi.c_u8p)
    fin.vertex = vertex.ctypes.data_as(_abi.c_u8p)
    if values.dtype == np.float64:
        fin.obs_val = values.ctypes.data_as(_abi.c_f64p)
    else:
        fin.obs_index = values.ctypes.data
        fin.index_type = DTYPES[values.dtype]
    tout = _abi.LtTileOut()
    tout.stride = P
    for f, a in out.items():
        setattr(tout, f, a.ctypes.data_as(type(getattr(tout, f))))
    sc = scene.to_c()
    rc = lib.ltx_ftv_tile(ctypes.byref(sc), ctypes.byref(fin), ctypes.byref(tout))
    assert rc == 0, rc
    return out


def load_fixture():
    """tests/golden/ftv_second.npz (made by tests/golden/make_ftv_golden.py from the reference's
    own vertices2eqns / eqns2fitted_points): {scene: dict(pix, kind, second, <five planes>)}."""
    z = np.load(FIXTURE)
    return {s: {k[len(s) + 1:]: z[k] for k in z.files if k.startswith(s + '_')}
            for s in FIXTURE_SCENES}


def rejected_winners(g):
    """The winner plane a golden scene implies for the pixels the reference rejected (the goldens
    record no point for them): per year slot the first valid observation of the year, -1 if none.
    Which of a year's observations wins does not matter for what FTV does with such a pixel."""
    years = np.asarray(g.scene.years)
    obs_year = np.array([int(d[:4]) for d in g.meta['dates']])
    w = g.ref['winner'].copy()
    for p in range(g.n_pix):
        if g.err[p] in ('', 'label:AttributeError'):
            continue
        for y, yr in enumerate(years):
            ks = [k for k in np.nonzero(obs_year == yr)[0] if g.valid[k, p]]
            w[y, p] = ks[0] if ks else -1
    return w


def handmade(Y, P, K, seed, first_late=True):
    """Hand-made planes of one scene of Y yearly slots and K >= Y observations (obs y is year y's
    winner unless noted) for P pixels, cycling through lane kinds:
      0  only the first and the last point are vertices, 0 / 1 / 3 spikes and 0-4 absent years: one
         long segment, m from 5 up with gaps (the x-set table misses, the general lsq_apply);
      1  a vertex every year (2-point segments);
      2  random vertices, spikes and absences;
      3  as 2 with the first present year late.
    Returns winner int16, spike uint8, vertex uint8 [Y, P]."""
    rng = np.random.default_rng(seed)
    winner = np.tile(np.arange(Y, dtype=np.int16)[:, None], (1, P))
    if K > Y:  # some winners among the extra observations
        pick = rng.random((Y, P)) < 0.3
        winner[pick] = rng.integers(Y, K, int(pick.sum())).astype(np.int16)
    spike = np.zeros((Y, P), np.uint8)
    vertex = np.zeros((Y, P), np.uint8)
    for p in range(P):
        kind = p % 4
        lo = 0
        if kind == 3 and first_late and Y > 6:
            lo = int(rng.integers(1, Y // 2))
            winner[:lo, p] = -1
        inner = np.arange(lo + 1, Y - 1)
        if kind == 0:
            n_abs = int(rng.integers(0, 5)) if len(inner) > 8 else 0
            if p % 8 == 4 and len(inner) > 12:  # many absent years: m from 5 up, x with gaps
                n_abs = len(inner) - int(rng.integers(3, min(31, len(inner))))
            absent = rng.choice(inner, min(n_abs, len(inner)), replace=False)
            winner[absent, p] = -1
            rest = np.setdiff1d(inner, absent)
            n_sp = (0, 1, 3)[(p // 4) % 3]
            if len(rest) > n_sp + 3:
                spike[rng.choice(rest, n_sp, replace=False), p] = 1
        elif kind == 1:
            pass
        elif len(inner):
            winner[inner[rng.random(len(inner)) < 0.15], p] = -1
            spike[inner[rng.random(len(inner)) < 0.15], p] = 1
            spike[winner[:, p] < 0, p] = 0
        pres = np.nonzero(winner[:, p] >= 0)[0]
        good = [y for y in pres if not spike[y, p]]
        if kind == 1:
            vertex[good, p] = 1
        elif kind >= 2:
            for y in good:
                vertex[y, p] = rng.random() < 0.35
        vertex[good[0], p] = vertex[good[-1], p] = 1
    return winner, spike, vertex



def check_golden(g, out, winner):
    """The six planes against a golden scene: bit for bit on present years of accepted pixels, NaN
    on absent years; rejected pixels carry the status bit of what the reference raised (the Feb-29
    rejection is the analysis's alone: FTV sees no dates, so such a pixel with two or more years
    is not looked at)."""
    ok = np.array([e in OK_ERR for e in g.err])
    present = winner >= 0
    for f in FTV_FIELDS:
        same = bits_equal(out[f], g.ref[f])
        m = ~same & present & ok[None, :]
        assert not m.any(), (g.name, f, int(m.sum()), np.argwhere(m)[:5].tolist())
        assert np.isnan(out[f][~present]).all(), (g.name, f)
    assert (out['status'][ok] == 0).all(), g.name
    for p in np.nonzero(~ok)[0]:
        T = int(present[:, p].sum())
        exp = golden_io.expected_status(g.err[p])
        if T < 2:
            assert out['status'][p] & exp, (g.name, p, g.err[p], int(out['status'][p]))
            for f in FIT_FIELDS:
                assert np.isnan(out[f][:, p]).all(), (g.name, f, p)
        else:
            assert exp & _abi.LT_ST_FEB29, (g.name, p, g.err[p])


def fixture_inputs(g, fz, integer):
    """The planes and second series of a fixture scene's pixels of the integer (True) or the float
    (False) kinds, and the expected planes."""
    sel = np.nonzero((fz['kind'] != 3) == integer)[0]
    pix = fz['pix'][sel]
    second = fz['second'][:, sel]
    vals = second.astype(np.int16) if integer else second
    assert (vals == second).all()
    want = {f: fz[f][:, sel] for f in FIT_FIELDS}
    return (g.ref['winner'][:, pix], g.ref['spike'][:, pix], g.ref['vertex'][:, pix], vals, want)


def check_fixture(out, winner, vals, want, tag):
    present = winner >= 0
    for f in FIT_FIELDS:
        m = ~bits_equal(out[f], want[f])
        assert not m.any(), (tag, f, int(m.sum()), np.argwhere(m)[:5].tolist())
    raw = np.where(present, np.take_along_axis(vals.astype(np.float64),
                                               np.maximum(winner, 0).astype(np.int64), 0), np.nan)
    assert bits_equal(out['val_raw'], raw).all(), tag
    assert (out['status'] == 0).all(), tag


def yearly_scene(Y, K=None, y0=1984):
    dates = ['%d-07-01' % (y0 + y) for y in range(Y)]
    dates += ['%d-07-%02d' % (y0 + (k * 7) % Y, 2 + k % 20) for k in range((K or Y) - Y)]
    return build_scene(dates, parse_date('2014-07-01'))
