"""Shared pieces of the change-map tests (tests/test_change_host.py, test_change_core_sanitized.py,
test_gpu_change.py): an independent reference of lt_change_maps and lt_label_counts in plain
Python / numpy scalars that walks the planes by the definitions of include/lt_abi.h (not derived
from land_trendr_amd/csrc/lt_change.h), the hand-made cases, the host twin's loader
(tests/native/build/liblt_changecheck.so), guarded buffers, and a CPU engine double with
change_maps / label_counts / sieve over the host twins for the job tests."""
import ctypes
import functools
import os

import numpy as np
import torch

import golden_io
from land_trendr_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANGECHECK = os.path.join(ROOT, 'tests', 'native', 'build', 'liblt_changecheck.so')
NODATA = _abi.LT_NODATA
LT_OK, LT_ERR_ARG, LT_ERR_LIMIT = 0, -1, -4  # include/lt_abi.h
MAP_FIELDS = tuple(f for f, _ in _abi.CHANGE_MAP_FIELDS)
PIX_FIELDS = tuple(f for f, _ in _abi.CHANGE_PIX_FIELDS)
DTYPE = {f: np.dtype(d) for f, d in _abi.CHANGE_MAP_FIELDS + _abi.CHANGE_PIX_FIELDS}
GUARD = {'matched': 0xA5, 'onset_year': -7, 'duration': -7, 'magnitude': 7.5, 'preval': 7.5,
         'rate': 7.5, 'dsnr': 7.5, 'rmse': 7.5, 'n_fit': -7}
SORTS = ('greatest', 'least', 'newest', 'oldest', 'longest', 'shortest', 'steepest', 'gentlest')


def same(a, b):
    """Element-wise equality: bit for bit (any NaN equal to any NaN) for floats."""
    a, b = np.asarray(a), np.asarray(b)
    return golden_io._bits_equal(a, b) if a.dtype.kind == 'f' else a == b


def assert_maps(got, want, tag):
    assert sorted(got) == sorted(want), (tag, sorted(got), sorted(want))
    for f, w in want.items():
        assert got[f].dtype == w.dtype and got[f].shape == w.shape, (tag, f)
        m = ~same(got[f], w)
        assert not m.any(), (tag, f, int(m.sum()), np.argwhere(m)[:5].tolist())


# ---- the reference ----

def _cmp(flt, a):
    """A filter [op, v] on the operand a: true iff it is unset or the comparison holds."""
    if flt is None:
        return True
    op, v = flt[0], np.float64(flt[1])
    return bool({'>': a > v, '<': a < v, '>=': a >= v, '<=': a <= v}[op])


def segments(years, val_fit, vertex, pres, p):
    """The pixel's points (slots) and its segments as (onset_year, duration, preval, d,
    magnitude, rate): the slots that hold a point in year order, the first the first left vertex,
    every later flagged one closing a segment and opening the next."""
    pts = [y for y in range(val_fit.shape[0]) if pres[y, p]]
    verts = [y for i, y in enumerate(pts) if i == 0 or vertex[y, p] != 0]
    segs = []
    with np.errstate(all='ignore'):
        for a, b in zip(verts[:-1], verts[1:]):
            fl, fr = np.float64(val_fit[a, p]), np.float64(val_fit[b, p])
            d = fl - fr
            mag = np.abs(d)
            dur = int(years[b]) - int(years[a])
            rate = mag / np.float64(dur)
            segs.append((int(years[a]), dur, fl, d, mag, rate))
    return pts, segs


_KEY = {'greatest': (4, 1), 'least': (4, -1), 'newest': (0, 1), 'oldest': (0, -1),
        'longest': (1, 1), 'shortest': (1, -1), 'steepest': (5, 1), 'gentlest': (5, -1)}


def reference(years, rules, val_fit, vertex, present=None, winner=None, val_raw=None, spike=None):
    """lt_change_maps by its definition, one pixel and one map at a time. rules: dicts in the
    settings' form ('delta', and optionally 'sort', 'index_sign', 'year', 'mag', 'dur',
    'preval'). Returns the planes Engine.change_maps returns (dsnr / rmse / n_fit only with both
    val_raw and spike)."""
    Y, P = val_fit.shape
    M = len(rules)
    fit = val_raw is not None and spike is not None
    pres = present != 0 if present is not None else (
        winner >= 0 if winner is not None else np.ones((Y, P), bool))
    out = {f: (np.zeros((M, P), np.uint8) if f == 'matched' else
               np.full((M, P), NODATA, DTYPE[f])) for f in MAP_FIELDS if f != 'dsnr' or fit}
    if fit:
        out['rmse'] = np.full(P, float(NODATA))
        out['n_fit'] = np.zeros(P, np.int32)
    for p in range(P):
        pts, segs = segments(years, val_fit, vertex, pres, p)
        rmse, n = None, 0
        if fit:
            acc = np.float64(0.0)
            with np.errstate(all='ignore'):
                for y in pts:
                    if spike[y, p] == 0:
                        r = np.float64(val_raw[y, p]) - np.float64(val_fit[y, p])
                        acc = acc + r * r
                        n += 1
                if n:
                    rmse = np.sqrt(np.float64(acc) / n)
                    out['rmse'][p] = rmse
            out['n_fit'][p] = n
        for m, rule in enumerate(rules):
            col, way = _KEY[rule.get('sort', 'greatest')]
            best = None
            for seg in segs:
                onset, dur, fl, d, mag, rate = seg
                sd = d if rule.get('index_sign', 1) == 1 else -d
                if not (sd > 0 if rule['delta'] == 'loss' else sd < 0):
                    continue
                yr = rule.get('year')
                if yr is not None and not yr[0] <= onset <= yr[1]:
                    continue
                if not (_cmp(rule.get('mag'), mag) and _cmp(rule.get('dur'), np.float64(dur)) and
                        _cmp(rule.get('preval'), fl)):
                    continue
                if best is None or (seg[col] > best[col] if way > 0 else seg[col] < best[col]):
                    best = seg
            if best is None:
                continue
            onset, dur, fl, d, mag, rate = best
            out['matched'][m, p] = 1
            out['onset_year'][m, p], out['duration'][m, p] = onset, dur
            out['magnitude'][m, p], out['preval'][m, p], out['rate'][m, p] = mag, fl, rate
            if fit and n:
                with np.errstate(all='ignore'):
                    out['dsnr'][m, p] = mag / rmse
    return out


def counts_reference(matched, key, key_lo, n_bins, start=None):
    """lt_label_counts by its definition (numpy), added onto `start`."""
    c = np.zeros(n_bins + 1, np.int64) if start is None else np.array(start, np.int64)
    k = np.asarray(key).astype(np.int64)[np.asarray(matched) != 0] - int(key_lo)
    inside = (k >= 0) & (k < n_bins)
    c[:n_bins] += np.bincount(k[inside], minlength=n_bins)
    c[n_bins] += int((~inside).sum())
    return c


# ---- the hand-made cases ----

N_KINDS = 14


def handmade(Y, P, seed, dup_years=False):
    """Hand-made planes for P pixels of Y yearly slots, cycling through pixel kinds:
      0  a vertex in every year, every slot a point;
      1  no flag at all (one vertex: no segment);      2  no point at all, flags set all the same;
      3  the first point late (slot Y // 2), its flag clear, random flags after;
      4  random points and flags, continuous values;   5  exactly one point;
      6  exactly two points (the second flagged for every other such pixel);
      7  every point a spike (n_fit == 0);             8  val_raw == val_fit (rmse 0, dsnr +inf);
      9  a zigzag of equal steps, every slot a vertex (equal keys in every sort but the years');
     10  flat runs: d == +0.0, and -0.0 - +0.0 == -0.0;
     11  a NaN val_fit at some vertex;                 12 / 13 random points, values on a grid of 25
         (magnitudes and prevals that meet the filters' boundary values exactly).
    Years have one gap; with dup_years every year appears twice (equal onset years, zero
    durations). Returns years, val_fit, val_raw, vertex, spike, present (uint8), winner (int16)."""
    rng = np.random.default_rng([seed, Y, P])
    if dup_years:
        years = (1984 + np.arange(Y) // 2).astype(np.int32)
    else:
        years = (1984 + np.arange(Y) + (np.arange(Y) > Y // 3)).astype(np.int32)
    val_fit = rng.normal(300.0, 400.0, (Y, P))
    val_raw = val_fit + rng.normal(0.0, 30.0, (Y, P))
    vertex = (rng.random((Y, P)) < 0.45).astype(np.uint8) * rng.integers(1, 256, (Y, P)).astype(
        np.uint8)
    present = (rng.random((Y, P)) < 0.8).astype(np.uint8)
    spike = (rng.random((Y, P)) < 0.15).astype(np.uint8)
    for p in range(P):
        kind = p % N_KINDS
        if kind == 0:
            vertex[:, p], present[:, p] = 1, 1
        elif kind == 1:
            vertex[:, p] = 0
        elif kind == 2:
            vertex[:, p], present[:, p] = 1, 0
        elif kind == 3:
            lo = Y // 2
            present[:lo, p], present[lo, p], vertex[lo, p] = 0, 1, 0
        elif kind == 5:
            present[:, p] = 0
            present[rng.integers(0, Y), p] = 1
        elif kind == 6:
            present[:, p] = 0
            pick = rng.choice(Y, size=min(2, Y), replace=False)
            present[pick, p] = 1
            vertex[:, p] = (p // N_KINDS) % 2
        elif kind == 7:
            spike[:, p] = 1
        elif kind == 8:
            val_raw[:, p] = val_fit[:, p]
        elif kind == 9:
            vertex[:, p], present[:, p] = 1, 1
            val_fit[:, p] = np.where(np.arange(Y) % 2 == 0, 100.0, 50.0)
        elif kind == 10:
            vertex[:, p], present[:, p] = 1, 1
            val_fit[:, p] = np.repeat(rng.integers(0, 3, (Y + 1) // 2) * 25.0, 2)[:Y]
            if Y >= 2:
                val_fit[0, p], val_fit[1, p] = -0.0, 0.0
        elif kind == 11:
            vertex[:, p] |= (rng.random(Y) < 0.5).astype(np.uint8)
            val_fit[rng.integers(0, Y), p] = np.nan
        elif kind in (12, 13):
            val_fit[:, p] = rng.integers(-4, 9, Y) * 25.0
            val_raw[:, p] = val_fit[:, p] + rng.integers(-2, 3, Y) * 5.0
            vertex[:, p] |= (rng.random(Y) < 0.5).astype(np.uint8)
    winner = np.where(present != 0, rng.integers(0, 300, (Y, P)), -1).astype(np.int16)
    return years, val_fit, val_raw, vertex, spike, present, winner


def rule_sets():
    """{tag: list of rule dicts}: every sort in both directions, index_sign -1, each filter alone
    at its boundary value with all four ops, one-year windows, every filter at once; lists of
    1, 2, 3, 5 and 8 maps (every kernel instance, and a non-power of two inside one)."""
    sets = {
        'loss-sorts': [{'delta': 'loss', 'sort': s} for s in SORTS],
        'gain-sorts': [{'delta': 'gain', 'sort': s} for s in SORTS],
        'one': [{'delta': 'loss'}],
        'two': [{'delta': 'gain', 'sort': 'newest'}, {'delta': 'loss', 'index_sign': -1}],
        'three-sign': [{'delta': 'loss', 'index_sign': -1, 'sort': 'steepest'},
                       {'delta': 'gain', 'index_sign': -1, 'sort': 'oldest'},
                       {'delta': 'gain', 'index_sign': 1, 'sort': 'shortest'}],
        'mag-ops': [{'delta': 'loss', 'mag': [op, 50]} for op in ('>', '<', '>=', '<=')] +
                   [{'delta': 'gain', 'sort': 'least', 'mag': [op, 50.0]}
                    for op in ('>', '<', '>=', '<=')],
        'dur-ops': [{'delta': 'loss', 'sort': 'newest', 'dur': [op, 2]}
                    for op in ('>', '<', '>=', '<=')] + [{'delta': 'gain', 'dur': ['>=', 1]}],
        'pre-ops': [{'delta': 'loss', 'sort': 'oldest', 'preval': [op, 100]}
                    for op in ('>', '<', '>=', '<=')] +
                   [{'delta': 'gain', 'sort': 'longest', 'preval': ['<', 0]}],
        'year-windows': [{'delta': 'loss', 'year': [1984, 1984]},
                         {'delta': 'gain', 'year': [1990, 1990], 'sort': 'gentlest'},
                         {'delta': 'loss', 'year': [1986, 1999], 'sort': 'newest'},
                         {'delta': 'gain', 'year': [-5, 1985]},
                         {'delta': 'loss', 'year': [2200, 2300]}],
        'all-filters': [{'delta': 'loss', 'sort': 'steepest', 'year': [1985, 2005],
                         'mag': ['>=', 25], 'dur': ['<=', 3], 'preval': ['>', -50.0]},
                        {'delta': 'gain', 'sort': 'least', 'index_sign': -1, 'year': [1984, 2040],
                         'mag': ['<', 400.5], 'dur': ['>=', 1], 'preval': ['<=', 700]},
                        {'delta': 'loss', 'mag': ['>', float('nan')]}],
    }
    return sets


SHAPES = ((1, 1), (2, 63), (3, 64), (12, 65), (33, 257), (64, 64), (12, 257), (1, 65), (2, 1))
PRESENCE = ('present', 'winner', 'neither')


@functools.lru_cache(maxsize=None)
def _planes(Y, P, dup):
    arrs = handmade(Y, P, 7, dup_years=dup)
    for a in arrs:
        a.setflags(write=False)
    return arrs


def case_tags():
    """Every hand-made case: each shape with each rule set once, the presence form and whether
    the fit inputs are given cycling so that every combination occurs; plus doubled years (equal
    onset years) under the sorts."""
    tags, i = [], 0
    for Y, P in SHAPES:
        for rs in rule_sets():
            tags.append('%dx%d-%s-%s-%s' % (Y, P, rs, PRESENCE[i % 3], 'fit' if i % 4 else 'nofit'))
            i += 1
    for Y, P in ((12, 65), (33, 64)):
        for rs in ('loss-sorts', 'gain-sorts'):
            tags.append('%dx%d-%s-neither-fit-dup' % (Y, P, rs))
    return tags


def case(tag):
    """(rules, keyword arguments of reference / run_host) of a hand-made case."""
    parts = tag.split('-')
    dup = parts[-1] == 'dup'
    if dup:
        parts = parts[:-1]
    shape, rs, pres, fit = parts[0], '-'.join(parts[1:-2]), parts[-2], parts[-1]
    Y, P = (int(v) for v in shape.split('x'))
    years, val_fit, val_raw, vertex, spike, present, winner = _planes(Y, P, dup)
    kw = dict(years=years, val_fit=val_fit, vertex=vertex)
    if pres == 'present':
        kw['present'] = present
    elif pres == 'winner':
        kw['winner'] = winner
    if fit == 'fit':
        kw.update(val_raw=val_raw, spike=spike)
    return rule_sets()[rs], kw


@functools.lru_cache(maxsize=None)
def case_reference(tag):
    """The reference's planes of a case, computed once and shared (read-only arrays)."""
    rules, kw = case(tag)
    out = reference(rules=rules, **kw)
    for a in out.values():
        a.setflags(write=False)
    return out


def random_field(P, Y, seed):
    """A random field with about Y / 2 vertices a pixel, as an analysis would leave it."""
    rng = np.random.default_rng(seed)
    years = (1985 + np.arange(Y)).astype(np.int32)
    val_fit = rng.normal(500.0, 300.0, (Y, P))
    val_raw = val_fit + rng.normal(0.0, 25.0, (Y, P))
    vertex = (rng.random((Y, P)) < 0.5).astype(np.uint8)
    spike = (rng.random((Y, P)) < 0.1).astype(np.uint8)
    winner = np.where(rng.random((Y, P)) < 0.9, rng.integers(0, 60, (Y, P)), -1).astype(np.int16)
    return dict(years=years, val_fit=val_fit, vertex=vertex, winner=winner, val_raw=val_raw,
                spike=spike)


EIGHT = [{'delta': 'loss'}, {'delta': 'gain', 'sort': 'newest', 'mag': ['>', 130]},
         {'delta': 'loss', 'sort': 'steepest', 'dur': ['>', 1], 'preval': ['>=', 600]},
         {'delta': 'loss', 'mag': ['>', 480]}, {'delta': 'gain', 'sort': 'longest', 'dur': ['<', 4]},
         {'delta': 'loss', 'sort': 'oldest', 'year': [1990, 1999]},
         {'delta': 'gain', 'sort': 'least', 'mag': ['<=', 260.0]},
         {'delta': 'loss', 'sort': 'shortest', 'index_sign': -1, 'preval': ['<', 400]}]


# ---- the 24 x 40 job ----

JOB_MAPS = [
    {'name': 'A', 'delta': 'loss', 'sort': 'greatest'},
    {'name': 'B', 'delta': 'gain', 'sort': 'newest', 'mag': ['>', 130], 'year': [1988, 1994]},
    {'name': 'C', 'delta': 'loss', 'sort': 'steepest', 'dur': ['>', 1], 'preval': ['>=', 600]},
    {'name': 'D', 'delta': 'loss', 'sort': 'greatest', 'mag': ['>', 480]},
    {'name': 'E', 'delta': 'gain', 'sort': 'longest', 'dur': ['<', 4]},
    {'name': 'F', 'delta': 'loss', 'sort': 'oldest', 'year': [1990, 1990]},
    {'name': 'G', 'delta': 'gain', 'sort': 'least', 'mag': ['<=', 26.0]},
    {'name': 'H', 'delta': 'loss', 'sort': 'shortest', 'preval': ['<', 0]}]
# what the reference gives on the 24 x 40, seed 5, 12-year job: pixels matched per map, and with
# mmu 3 (8-connectivity by onset year) the pixels removed
JOB_MATCHED = {'A': 960, 'B': 250, 'C': 691, 'D': 474, 'E': 955, 'F': 125, 'G': 517, 'H': 92}
JOB_REMOVED = {'A': 466, 'B': 215, 'C': 413, 'D': 385, 'E': 540, 'F': 75, 'G': 422, 'H': 89}
SHAPE = (24, 40)


def file_bytes(files):
    out = {}
    for k, (path,) in files.items():
        with open(path, 'rb') as fh:
            out[k] = fh.read()
    return out


def job_reference(plain):
    """The reference's change maps of the 24 x 40 job from the trendline planes of a run without
    the key, the dropped pixels' matches cleared; and the mask of the pixels kept."""
    pl = plain.planes
    want = reference(plain.scene.years, JOB_MAPS, pl['val_fit'], pl['vertex'],
                        winner=pl['winner'], val_raw=pl['val_raw'], spike=pl['spike'])
    keep = pl['status'] == 0
    want = {f: a.copy() for f, a in want.items()}
    want['matched'][:, ~keep] = 0
    return want, keep


def expected_stats(want, years, before=None):
    stats = {}
    for m, rule in enumerate(JOB_MAPS):
        on = want['onset_year'][m][want['matched'][m] != 0]
        n0 = int((before if before is not None else want)['matched'][m].astype(bool).sum())
        stats[rule['name']] = {'matched': n0, 'removed': n0 - len(on),
                               'by_year': {int(y): int((on == y).sum()) for y in years}}
    return stats


def check_change_files(j, files, want, keep, mode):
    from land_trendr_amd.geotiff import GeoTiff
    from land_trendr_amd.raster import CHANGE_ATTRS, change_rasters
    tmpl = GeoTiff(j.rast_fns[0])
    exp = change_rasters(want, JOB_MAPS, SHAPE, tmpl.dtype.newbyteorder('='), mode, keep=keep)
    got = {k: v for k, v in files.items() if k.startswith('change/')}
    assert sorted(got) == sorted(exp)
    assert len(exp) == len(JOB_MAPS) * len(CHANGE_ATTRS) + 1 and 'change/rmse' in exp
    for k, w in exp.items():
        a = GeoTiff(got[k][0]).read()[0]
        assert a.dtype == w.dtype and same(a, w).all(), k
    if mode == 'typed':
        assert exp['change/A-onset_year'].dtype == np.int32
        assert exp['change/A-dsnr'].dtype == np.float64


# ---- the host twin ----

def load_host():
    """The host twin (tests/native/change_host_check.hip), built by __graft_entry__.build()."""
    if not os.path.exists(CHANGECHECK):
        raise RuntimeError('host twin not built: run __graft_entry__.build()')
    L = ctypes.CDLL(CHANGECHECK)
    L.ltx_change_maps.argtypes = [ctypes.POINTER(_abi.LtChangeIn), ctypes.c_int,
                                  ctypes.POINTER(_abi.LtChangeRule),
                                  ctypes.POINTER(_abi.LtChangeOut)]
    L.ltx_label_counts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                   ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]
    return L


def c_rules(rules):
    return (_abi.LtChangeRule * max(len(rules), 1))(*[
        r if isinstance(r, _abi.LtChangeRule) else _abi.change_rule(r) for r in rules])


def structs(years, n_pix, stride, ptr, ostride, optr):
    """The two ABI structs over raw addresses: ptr / optr map a field name to an address (absent
    or None: NULL). `years` must stay alive while the structs are used."""
    cin, cout = _abi.LtChangeIn(), _abi.LtChangeOut()
    cin.n_pix, cin.stride, cin.n_years = n_pix, stride, len(years)
    cin.year = years.ctypes.data_as(_abi.c_i32p)
    for f in ('val_fit', 'vertex', 'val_raw', 'present', 'winner', 'spike'):
        if ptr.get(f):
            setattr(cin, f, ctypes.cast(ptr[f], type(getattr(cin, f))))
    cout.stride = ostride
    for f in MAP_FIELDS + PIX_FIELDS:
        if optr.get(f):
            setattr(cout, f, ctypes.cast(optr[f], type(getattr(cout, f))))
    return cin, cout


def padded(a, pad, guard=0):
    """`a` ([rows, P]) in rows of P + pad elements, the padding holding `guard`."""
    buf = np.full((a.shape[0], a.shape[1] + pad), guard, a.dtype)
    buf[:, :a.shape[1]] = a
    return buf


def guarded_outputs(M, P, pad, fields, extra_rows=2):
    """Output buffers with a guard row before, `extra_rows` after row M - 1 and `pad` guard
    elements after every row ([P] planes: pad + 1 guard elements before and after):
    {field: full buffer}. Row m of a map plane is buffer row m + 1."""
    out = {}
    for f in fields:
        if f in PIX_FIELDS:
            out[f] = np.full(P + 2 * pad + 2, GUARD[f], DTYPE[f])
        else:
            out[f] = np.full((M + 1 + extra_rows, P + pad), GUARD[f], DTYPE[f])
    return out


def output_ptrs(bufs, pad):
    return {f: (b[pad + 1:].ctypes.data if f in PIX_FIELDS else b[1:].ctypes.data)
            for f, b in bufs.items()}


def check_guards(bufs, M, P, pad):
    """The guard values of guarded_outputs buffers are intact; returns the written part."""
    out = {}
    for f, b in bufs.items():
        g = GUARD[f]
        if f in PIX_FIELDS:
            assert (b[:pad + 1] == g).all() and (b[pad + 1 + P:] == g).all(), f
            out[f] = b[pad + 1:pad + 1 + P].copy()
            continue
        assert (b[0] == g).all() and (b[M + 1:] == g).all(), (f, 'rows outside [0, M)')
        assert (b[:, P:] == g).all(), (f, 'padding')
        out[f] = b[1:M + 1, :P].copy()
    return out


def default_fields(fit):
    return tuple(f for f in MAP_FIELDS + PIX_FIELDS if fit or f not in ('dsnr', 'rmse', 'n_fit'))


def run_host(lib, rules, years, val_fit, vertex, present=None, winner=None, val_raw=None,
             spike=None, pad=0, fields=None, expect=0):
    """ltx_change_maps on numpy planes, the inputs in rows of P + pad, the outputs in guarded
    buffers; checks the guards and the rows >= M, returns the written part {field: array}."""
    years = np.ascontiguousarray(years, np.int32)
    Y, P = val_fit.shape
    M = len(rules)
    keep, ptr = [], {}
    for f, a, dt in (('val_fit', val_fit, np.float64), ('vertex', vertex, np.uint8),
                     ('val_raw', val_raw, np.float64), ('present', present, np.uint8),
                     ('winner', winner, np.int16), ('spike', spike, np.uint8)):
        if a is not None:
            buf = padded(np.ascontiguousarray(a, dt), pad)
            keep.append(buf)
            ptr[f] = buf.ctypes.data
    if fields is None:
        fields = default_fields(val_raw is not None and spike is not None)
    bufs = guarded_outputs(M, P, pad, fields)
    cin, cout = structs(years, P, P + pad, ptr, P + pad, output_ptrs(bufs, pad))
    rc = lib.ltx_change_maps(ctypes.byref(cin), M, c_rules(rules), ctypes.byref(cout))
    assert rc == expect, rc
    return check_guards(bufs, M, P, pad)


def host_counts(lib, matched, key, key_lo, n_bins, start=None, expect=0):
    """ltx_label_counts on numpy arrays into a guarded count buffer -> int64 [n_bins + 1]."""
    m = np.ascontiguousarray(matched, np.uint8)
    k = np.ascontiguousarray(key, np.int32)
    c = np.full(n_bins + 1 + 4, 0x5555, np.uint64)
    c[2:n_bins + 3] = 0 if start is None else np.asarray(start, np.uint64)
    rc = lib.ltx_label_counts(m.ctypes.data, k.ctypes.data, m.size, key_lo, n_bins,
                              c[2:].ctypes.data)
    assert rc == expect, rc
    assert (c[:2] == 0x5555).all() and (c[n_bins + 3:] == 0x5555).all()
    return c[2:n_bins + 3].astype(np.int64)


def make_twin_engine():
    """The CPU engine double (engine_double.OracleEngine) with change_maps and label_counts over
    the host twin and the sieve of sievefixture's twin engine: host tensors in and out, the
    signatures of Engine's methods. For the job's CPU tests only (the product has no CPU path)."""
    import sievefixture

    class ChangeTwinEngine(type(sievefixture.make_twin_engine())):
        def change_maps(self, years, rules, val_fit, vertex, present=None, winner=None,
                        val_raw=None, spike=None, out=None, stream=None):
            Y, P = val_fit.shape
            M = len(rules)
            planes = {'val_fit': val_fit, 'vertex': vertex, 'val_raw': val_raw,
                      'present': present, 'winner': winner, 'spike': spike}
            ptr = {f: t.data_ptr() for f, t in planes.items() if t is not None}
            strides = {t.stride(0) for t in planes.values() if t is not None and Y > 1}
            assert len(strides) <= 1, 'the input planes must share one row stride'
            fit = val_raw is not None and spike is not None
            if out is None:
                out = {f: torch.empty((P,) if f in PIX_FIELDS else (M, P),
                                      dtype=getattr(torch, DTYPE[f].name))
                       for f in default_fields(fit)}
            ostrides = {t.stride(0) for f, t in out.items()
                        if f not in PIX_FIELDS and t.shape[0] > 1}
            assert len(ostrides) <= 1, 'the output planes must share one row stride'
            yrs = np.ascontiguousarray(years, np.int32)
            cin, cout = structs(yrs, P, strides.pop() if strides else max(P, 1), ptr,
                                ostrides.pop() if ostrides else max(P, 1),
                                {f: t.data_ptr() for f, t in out.items()})
            rc = load_host().ltx_change_maps(ctypes.byref(cin), M, c_rules(rules),
                                             ctypes.byref(cout))
            assert rc == 0, rc
            return out

        def label_counts(self, matched, key, key_lo, n_bins, out=None):
            if out is None:
                out = torch.zeros(n_bins + 1, dtype=torch.int64)
            assert out.dtype == torch.int64 and out.numel() == n_bins + 1 and out.stride(0) == 1
            P = matched.numel()
            assert key.numel() == P and (P <= 1 or (matched.stride(0) == 1 and key.stride(0) == 1))
            rc = load_host().ltx_label_counts(matched.data_ptr(), key.data_ptr(), P, key_lo,
                                              n_bins, out.data_ptr())
            assert rc == 0, rc
            return out
    return ChangeTwinEngine()
