"""Shared pieces of the vertex-table tests (tests/test_vertex_host.py, tests/test_gpu_vertex.py):
the host twin's loader, a numpy restatement of lt_vertex_table's definition, the committed
reference fixture (tests/golden/vertex_table.npz), hand-made planes with guard values, a CPU engine
double with a vertex_table for the job tests, and the job's expected rasters."""
import ctypes
import os

import numpy as np
import torch

import golden_io
from engine_double import OracleEngine
from land_trendr_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERTEXCHECK = os.path.join(ROOT, 'tests', 'native', 'build', 'liblt_vertexcheck.so')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'vertex_table.npz')
OK_ERR = ('', 'label:AttributeError')
NODATA = _abi.LT_NODATA
LT_OK, LT_ERR_ARG, LT_ERR_LIMIT = 0, -1, -4  # include/lt_abi.h
PLANES = ('vertex_year', 'vertex_fit', 'vertex_raw')
GUARD = {'n_vertices': -7, 'vertex_year': -7, 'vertex_fit': 7.5, 'vertex_raw': 7.5}
HAND_SHAPES = ((2, 1), (26, 19), (33, 65), (64, 130))


def same(a, b):
    """Element-wise equality: bit for bit (any NaN equal to any NaN) for floats."""
    a, b = np.asarray(a), np.asarray(b)
    return golden_io._bits_equal(a, b) if a.dtype.kind == 'f' else a == b


def vertex_numpy(years, val_fit, vertex, present=None, winner=None, val_raw=None, V=None):
    """lt_vertex_table's definition in numpy: the slots that hold a point in year order, the first
    of them vertex 0, every later flagged one the next; LT_NODATA from a pixel's count on."""
    Y, P = val_fit.shape
    V = Y if V is None else V
    pres = present != 0 if present is not None else (
        winner >= 0 if winner is not None else np.ones((Y, P), bool))
    out = {'n_vertices': np.zeros(P, np.int32), 'vertex_year': np.full((V, P), NODATA, np.int32),
           'vertex_fit': np.full((V, P), float(NODATA))}
    if val_raw is not None:
        out['vertex_raw'] = np.full((V, P), float(NODATA))
    for p in range(P):
        ys = np.flatnonzero(pres[:, p])
        ys = [y for i, y in enumerate(ys) if i == 0 or vertex[y, p]]
        out['n_vertices'][p] = len(ys)
        for j, y in enumerate(ys[:V]):
            out['vertex_year'][j, p] = years[y]
            out['vertex_fit'][j, p] = val_fit[y, p]
            if val_raw is not None:
                out['vertex_raw'][j, p] = val_raw[y, p]
    return out


def load_host():
    """The host twin (tests/native/vertex_host_check.hip), built by __graft_entry__.build()."""
    if not os.path.exists(VERTEXCHECK):
        raise RuntimeError('host twin not built: run __graft_entry__.build()')
    L = ctypes.CDLL(VERTEXCHECK)
    L.ltx_vertex_table.argtypes = [ctypes.POINTER(_abi.LtVertexIn), ctypes.POINTER(_abi.LtVertexOut)]
    return L


def structs(years, n_pix, stride, ptr, ostride, V, optr):
    """The two ABI structs over raw addresses: ptr / optr map a field name to an address (absent
    or None: NULL). `years` must stay alive while the structs are used."""
    vin, vout = _abi.LtVertexIn(), _abi.LtVertexOut()
    vin.n_pix, vin.stride, vin.n_years = n_pix, stride, len(years)
    vin.year = years.ctypes.data_as(_abi.c_i32p)
    for f in ('val_fit', 'vertex', 'val_raw', 'present', 'winner'):
        if ptr.get(f):
            setattr(vin, f, ctypes.cast(ptr[f], type(getattr(vin, f))))
    vout.stride, vout.max_vertices = ostride, V
    for f in ('n_vertices',) + PLANES:
        if optr.get(f):
            setattr(vout, f, ctypes.cast(optr[f], type(getattr(vout, f))))
    return vin, vout


def padded(a, pad, guard):
    """`a` ([rows, P]) in rows of P + pad elements, the padding holding `guard`: (buffer, view)."""
    buf = np.full((a.shape[0], a.shape[1] + pad), guard, a.dtype)
    buf[:, :a.shape[1]] = a
    return buf, buf[:, :a.shape[1]]


def guarded_outputs(V, P, pad, raw=True, extra_rows=2):
    """Output buffers with a guard row before, `extra_rows` after row V - 1 and `pad` guard
    elements after every row: {field: full buffer}. Row j of a plane is buffer row j + 1."""
    out = {'n_vertices': np.full(P + 2 * pad + 2, GUARD['n_vertices'], np.int32)}
    for f in PLANES[:3 if raw else 2]:
        out[f] = np.full((V + 1 + extra_rows, P + pad), GUARD[f],
                         np.int32 if f == 'vertex_year' else np.float64)
    return out


def run_host(lib, years, val_fit, vertex, present=None, winner=None, val_raw=None, V=None, pad=0,
             expect=0):
    """ltx_vertex_table on numpy planes, the inputs in rows of P + pad, the outputs in guarded
    buffers; checks the guards and the rows >= V, returns the written part {field: array}."""
    years = np.ascontiguousarray(years, np.int32)
    Y, P = val_fit.shape
    V = Y if V is None else V
    keep, ptr = [], {}
    for f, a, dt in (('val_fit', val_fit, np.float64), ('vertex', vertex, np.uint8),
                     ('val_raw', val_raw, np.float64), ('present', present, np.uint8),
                     ('winner', winner, np.int16)):
        if a is not None:
            buf, _ = padded(np.ascontiguousarray(a, dt), pad, 0)
            keep.append(buf)
            ptr[f] = buf.ctypes.data
    bufs = guarded_outputs(V, P, pad, raw=val_raw is not None)
    optr = {f: (b[pad + 1:].ctypes.data if f == 'n_vertices' else b[1:].ctypes.data)
            for f, b in bufs.items()}
    vin, vout = structs(years, P, P + pad, ptr, P + pad, V, optr)
    rc = lib.ltx_vertex_table(ctypes.byref(vin), ctypes.byref(vout))
    assert rc == expect, rc
    return check_guards(bufs, V, P, pad)


def check_guards(bufs, V, P, pad):
    """The guard values of guarded_outputs buffers are intact; returns the written part."""
    out = {}
    for f, b in bufs.items():
        g = GUARD[f]
        if f == 'n_vertices':
            assert (b[:pad + 1] == g).all() and (b[pad + 1 + P:] == g).all(), f
            out[f] = b[pad + 1:pad + 1 + P].copy()
            continue
        assert (b[0] == g).all() and (b[V + 1:] == g).all(), (f, 'rows outside [0, V)')
        assert (b[:, P:] == g).all(), (f, 'padding')
        out[f] = b[1:V + 1, :P].copy()
    return out


def assert_table(got, want, tag):
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for f, w in want.items():
        m = ~same(got[f], w)
        assert not m.any(), (tag, f, int(m.sum()), np.argwhere(m)[:5].tolist())


def load_fixture():
    """tests/golden/vertex_table.npz (made by tests/golden/make_vertex_golden.py from the
    reference's own Trendline points and parse_disturbances): {scene: {name: array}}."""
    z = np.load(FIXTURE)
    return {s: {k[len(s) + 1:]: z[k] for k in z.files if k.startswith(s + '_')}
            for s in golden_io.scene_names()}


def fixture_table(fz, Y):
    """A fixture scene's ragged vertex lists as dense planes [Y, n] (LT_NODATA from a pixel's
    count on) and the reference's disturbance lists likewise [Y - 1, n]."""
    n = len(fz['pix'])
    nv = np.diff(fz['voff']).astype(np.int32)
    tab = {'n_vertices': nv, 'vertex_year': np.full((Y, n), NODATA, np.int32),
           'vertex_fit': np.full((Y, n), float(NODATA)),
           'vertex_raw': np.full((Y, n), float(NODATA))}
    nd = np.diff(fz['doff']).astype(np.int32)
    dis = {'n_segments': nd, 'onset_year': np.full((Y - 1, n), NODATA, np.int32),
           'duration': np.full((Y - 1, n), NODATA, np.int32),
           'initial_val': np.full((Y - 1, n), float(NODATA)),
           'magnitude': np.full((Y - 1, n), float(NODATA))}
    for i in range(n):
        a, b = fz['voff'][i], fz['voff'][i + 1]
        tab['vertex_year'][:b - a, i] = fz['vyear'][a:b]
        tab['vertex_fit'][:b - a, i] = fz['vfit'][a:b]
        tab['vertex_raw'][:b - a, i] = fz['vraw'][a:b]
        a, b = fz['doff'][i], fz['doff'][i + 1]
        dis['onset_year'][:b - a, i] = fz['donset'][a:b]
        dis['duration'][:b - a, i] = fz['dduration'][a:b]
        dis['initial_val'][:b - a, i] = fz['dinitial'][a:b]
        dis['magnitude'][:b - a, i] = fz['dmagnitude'][a:b]
    return tab, dis


def handmade(Y, P, seed):
    """Hand-made planes for P pixels of Y yearly slots, cycling through pixel kinds:
      0  a vertex in every year, every slot a point (n = Y);
      1  no flag at all (n = 1, the first point);
      2  no point at all (n = 0), flags set all the same;
      3  the first point late (slot Y // 2 if there is one), its flag clear, random flags after;
      4  random points and flags.
    val_fit / val_raw carry NaNs with payloads, -0.0 and infinities by bits. Returns years,
    val_fit, val_raw, vertex, present (uint8), winner (int16; >= 0 where present)."""
    rng = np.random.default_rng(seed)
    years = (1984 + np.arange(Y) + (np.arange(Y) > Y // 3)).astype(np.int32)  # one gap year
    special = np.array([0x7ff8000000000000, 0x7ff8000000000123, 0xfff0000000000001,
                        0x8000000000000000, 0x7ff0000000000000, 0x0000000000000001], np.uint64)

    def values():
        v = rng.normal(0.0, 1000.0, (Y, P))
        pick = rng.random((Y, P)) < 0.2
        v.view(np.uint64)[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
        return v
    val_fit, val_raw = values(), values()
    vertex = (rng.random((Y, P)) < 0.4).astype(np.uint8)
    present = (rng.random((Y, P)) < 0.8).astype(np.uint8)
    for p in range(P):
        kind = p % 5
        if kind == 0:
            vertex[:, p], present[:, p] = 1, 1
        elif kind == 1:
            vertex[:, p] = 0
        elif kind == 2:
            vertex[:, p], present[:, p] = 1, 0
        elif kind == 3:
            lo = Y // 2
            present[:lo, p], present[lo, p], vertex[lo, p] = 0, 1, 0
    winner = np.where(present != 0, rng.integers(0, 300, (Y, P)), -1).astype(np.int16)
    return years, val_fit, val_raw, vertex, present, winner


def handmade_cases(Y, P, seed):
    """(tag, keyword arguments of vertex_numpy / run_host) over handmade(): presence given as
    `present`, as `winner` and not at all; with and without val_raw; V = Y and, where there is
    room, a cap."""
    years, val_fit, val_raw, vertex, present, winner = handmade(Y, P, seed)
    base = dict(years=years, val_fit=val_fit, vertex=vertex)
    yield 'present', dict(base, present=present, val_raw=val_raw)
    yield 'winner', dict(base, winner=winner, val_raw=val_raw)
    yield 'neither', dict(base, val_raw=val_raw)
    yield 'no raw', dict(base, winner=winner)
    if Y > 2:
        yield 'capped', dict(base, present=present, val_raw=val_raw, V=max(1, Y // 3))


class VertexOracleEngine(OracleEngine):
    """The CPU engine double with the two methods the vertex-table job needs, both over the host
    twins (host tensors in, host tensors out): vertex_table, and ftv_tile for ftv_eqns."""

    def vertex_table(self, years, val_fit, vertex, present=None, winner=None, val_raw=None,
                     max_vertices=None, out=None, stream=None):
        Y, P = val_fit.shape
        V = Y if max_vertices is None else int(max_vertices)
        ptr = {f: t.data_ptr() for f, t in (('val_fit', val_fit), ('vertex', vertex),
                                            ('val_raw', val_raw), ('present', present),
                                            ('winner', winner)) if t is not None}
        strides = {t.stride(0) for t in (val_fit, vertex, val_raw, present, winner)
                   if t is not None and Y > 1}
        assert len(strides) <= 1, 'the input planes must share one row stride'
        if out is None:
            out = {'n_vertices': torch.empty(P, dtype=torch.int32),
                   'vertex_year': torch.empty((V, P), dtype=torch.int32),
                   'vertex_fit': torch.empty((V, P), dtype=torch.float64)}
            if val_raw is not None:
                out['vertex_raw'] = torch.empty((V, P), dtype=torch.float64)
        ostrides = {t.stride(0) for f, t in out.items() if f != 'n_vertices' and t.shape[0] > 1}
        assert len(ostrides) <= 1, 'the output planes must share one row stride'
        yrs = np.ascontiguousarray(years, np.int32)
        vin, vout = structs(yrs, P, strides.pop() if strides else max(P, 1), ptr,
                            ostrides.pop() if ostrides else max(P, 1), V,
                            {f: t.data_ptr() for f, t in out.items()})
        rc = load_host().ltx_vertex_table(ctypes.byref(vin), ctypes.byref(vout))
        assert rc == 0, rc
        return out

    def ftv_tile(self, scene, winner, spike, vertex, values, fields=_abi.FTV_FIELDS, out=None,
                 stream=None):
        import ftvfixture
        got = ftvfixture.run_host(ftvfixture.load_host(), scene, winner.numpy(), spike.numpy(),
                                  vertex.numpy(), values.numpy(),
                                  [f for f in (out or fields) if f != 'status'])
        if out is None:
            return {f: torch.from_numpy(a) for f, a in got.items()}
        for f, t in out.items():
            t.copy_(torch.from_numpy(got[f]))
        return out


def expected_vertex_rasters(j, table, ok, mode, prefix='vertices/'):
    """The rasters a reducer would emit from a vertex table (host arrays, the job's pixel order),
    placed like data2raster places values (jobfixture.literal_output_rasters): for every pixel with
    ok[p] and two or more vertices, 'n_vertices' and, per vertex kk it has (up to the table's
    rows), '<kk>-year', '<kk>-val_fit', '<kk>-val_raw'."""
    from land_trendr_amd import ingest, raster
    from land_trendr_amd.geotiff import GeoTiff
    tmpl = GeoTiff(j.rast_fns[0])
    gt = tmpl.geotransform()
    hdt = raster.holder_dtype(tmpl.dtype.newbyteorder('='))
    typed = {'n_vertices': np.int32, 'year': np.int32, 'val_fit': np.float64,
             'val_raw': np.float64}
    holders = {}
    V = table['vertex_year'].shape[0]
    for p, w in enumerate(j.grid_wkts()):
        n = int(table['n_vertices'][p])
        if not ok[p] or n < 2:
            continue
        x, y = ingest.get_pix_offsets_for_point(gt, *ingest.parse_point_wkt(w))
        emit = [('n_vertices', 'n_vertices', n)]
        for k in range(min(n, V)):
            emit += [('%02d-%s' % (k + 1, a), a, table[f][k, p])
                     for a, f in (('year', 'vertex_year'), ('val_fit', 'vertex_fit'),
                                  ('val_raw', 'vertex_raw'))]
        for key, a, v in emit:
            h = holders.get(prefix + key)
            if h is None:
                h = holders[prefix + key] = np.full(
                    (tmpl.height, tmpl.width), raster.NODATA,
                    hdt if mode == 'reference' else typed[a])
            h[y, x] = float(v)
    if mode == 'reference':
        return {k: raster.gdal_to_byte(h) for k, h in holders.items()}
    return holders
