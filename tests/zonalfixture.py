"""Shared by the zonal table's CPU and GPU tests (test_zonal_host.py, test_zonal_settings.py,
test_zonal_core_sanitized.py, test_gpu_zonal.py): an independent reference of lt_zonal_stats in
plain numpy, written from the definition in include/lt_abi.h and not from lt_zonal.h; the case
list; the loader of the host twin (tests/native/zonal_host_check.hip); the zone rasters of the
24 x 40 job; and a CPU engine double with a zonal_stats over the host twin for the job tests."""
import ctypes
import functools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZONALCHECK = os.path.join(ROOT, 'tests', 'native', 'build', 'liblt_zonalcheck.so')
LT_OK, LT_ERR_ARG, LT_ERR_LIMIT = 0, -1, -4
LT_MAX_ZONES = 65536
LDS_CELLS = 1024          # path 1 takes (n_zones + 1) * (n_bins + 1) up to this
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


# ---- the reference ----

def reference_sparse(matched, zone, key, key_lo, n_bins, n_zones, duration=None, value=None):
    """lt_zonal_stats by its definition, as (cells, words): the flat indices row * (n_bins + 1) +
    column of the cells some matched pixel falls in, ascending, and their four addends, int64
    [len(cells), 4] (np.add.at on an int64 table; int64 adds wrap as two's complement does)."""
    m = np.asarray(matched) != 0
    z = np.asarray(zone).astype(np.int64)[m]
    row = np.where((z >= 0) & (z < n_zones), z, n_zones)
    k = np.asarray(key).astype(np.int64)[m] - int(key_lo)
    col = np.where((k >= 0) & (k < n_bins), k, n_bins)
    cells, inv = np.unique(row * (n_bins + 1) + col, return_inverse=True)
    words = np.zeros((len(cells), 4), np.int64)
    np.add.at(words[:, 0], inv, 1)
    if duration is not None:
        np.add.at(words[:, 1], inv, np.asarray(duration).astype(np.int64)[m])
    if value is not None:
        v = np.asarray(value, np.float64)[m]
        ok = ~np.isnan(v)
        q = np.rint(np.clip(v[ok], -2 ** 30, 2 ** 30) * 16).astype(np.int64)
        np.add.at(words[:, 2], inv[ok], q)
        np.add.at(words[:, 3], inv[ok], 1)
    return cells, words


def dense(sparse, n_zones, n_bins, start=None, times=1):
    """The table [n_zones + 1, n_bins + 1, 4] a call leaves that starts from `start` (zeros when
    None), the call made `times` times; sums modulo 2^64."""
    cells, words = sparse
    t = (np.zeros((n_zones + 1) * (n_bins + 1) * 4, np.uint64) if start is None
         else np.array(start, np.int64).reshape(-1).view(np.uint64).copy())
    t = t.reshape(-1, 4)
    with np.errstate(over='ignore'):
        for _ in range(times):
            t[cells] += words.view(np.uint64)
    return t.view(np.int64).reshape(n_zones + 1, n_bins + 1, 4)


def reference(matched, zone, key, key_lo, n_bins, n_zones, duration=None, value=None, start=None):
    return dense(reference_sparse(matched, zone, key, key_lo, n_bins, n_zones, duration, value),
                 n_zones, n_bins, start)


# ---- the cases ----

N_PIX = (0, 1, 63, 64, 65, 257, 16383, 16385, 70001)
N_ZONES = (1, 2, 7, 300, 65536)
N_BINS = (1, 30, 256)
# the rounding ties 0.03125 * 16 = 0.5 -> 0 and 0.09375 * 16 = 1.5 -> 2 (half to even), the clamp
# on both sides, what does not fit an int64 before the clamp, both zeros, both infinities, NaN
VALUES = (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300, -1e300, 0.03125, 0.09375, -0.03125,
          -0.09375, -5.5, 1073741824.0, -1073741824.0, 1073741825.0, 1073741823.96875, 2.0 ** 62,
          -523.21875, 7.0)
PATTERNS = ('mixed', 'one_cell', 'lane_cells', 'runs', 'unmatched', 'edges', 'edges_lo', 'values',
            'null_dur', 'null_val', 'null_both', 'start')
# every pattern but 'mixed' (the whole grid) runs on these: each n_pix, each n_zones and each
# n_bins at least once, tables on both sides of the LDS path's limit
SOME = ((0, 7, 30), (1, 1, 1), (63, 2, 256), (64, 300, 30), (65, 7, 1), (257, 65536, 30),
        (16383, 2, 30), (16385, 300, 1), (70001, 7, 30), (70001, 300, 256), (16385, 65536, 256))


def shapes(pattern):
    if pattern == 'mixed':
        return tuple((P, Z, B) for P in N_PIX for Z in N_ZONES for B in N_BINS)
    return SOME


def paths(n_zones, n_bins):
    """The paths lt_zonal_stats can be forced onto for this table."""
    return (1, 2) if (n_zones + 1) * (n_bins + 1) <= LDS_CELLS else (2,)


@functools.lru_cache(maxsize=None)
def case(pattern, P, Z, B):
    """One case: the keyword arguments of reference() (arrays read-only), 'start' included (None:
    a zeroed table) and 'times' (the calls made into the one table)."""
    rng = np.random.default_rng([PATTERNS.index(pattern), P, Z, B])
    lo = 1985
    c = dict(key_lo=lo, n_bins=B, n_zones=Z, start=None, times=1)
    matched = ((rng.random(P) < 0.7) * rng.integers(1, 256, P)).astype(np.uint8)
    zone = rng.integers(-2, Z + 2, P).astype(np.int32)
    key = rng.integers(lo - 2, lo + B + 2, P).astype(np.int32)
    duration = rng.integers(-5, 40, P).astype(np.int32)
    value = rng.normal(0.0, 500.0, P)
    value[rng.random(P) < 0.05] = np.nan
    cells = (Z + 1) * (B + 1)
    if pattern == 'one_cell':   # the most contention: every pixel in one cell, large addends
        matched[:] = 1
        zone[:], key[:] = Z - 1, lo + B - 1
        duration[:], value[:] = I32_MAX, 1e9
    elif pattern == 'lane_cells':  # 64 rounds: a cell of its own for every lane of a wave
        lane = np.arange(P) % 64
        matched[:] = 1
        zone[:] = lane % (Z + 1)
        key[:] = lo + (lane // (Z + 1)) % (B + 1)
    elif pattern == 'runs':     # zone runs of 1, 3, 64 and 100 across wave and block boundaries
        runs = np.resize(np.array([1, 3, 64, 100, 100, 64, 3, 1, 64, 64]), P + 1)
        idx = np.repeat(np.arange(P + 1), runs)[:P]
        zone[:] = idx % Z
        key[:] = lo + idx % B
        matched[:] = (rng.random(P) < 0.95)
    elif pattern == 'unmatched':
        matched[:] = 0
    elif pattern == 'edges':
        zone[:] = rng.choice([-1, I32_MIN, Z, I32_MAX, 0, Z - 1], P)
        key[:] = rng.choice([lo - 1, lo + B, I32_MIN, I32_MAX, lo, lo + B - 1], P)
        duration[:] = rng.choice([I32_MIN, I32_MAX, -1, 0], P)
    elif pattern == 'edges_lo':  # key - key_lo needs 64 bits: INT32_MIN - INT32_MAX
        c['key_lo'] = I32_MAX
        key[:] = rng.choice([I32_MIN, I32_MAX, 0, -1], P)
    elif pattern == 'values':
        matched[:] = 1
        value[:] = np.resize(np.array(VALUES), P)
        zone[:] = (np.arange(P) // len(VALUES)) % Z   # (every value meets every other in a cell)
        duration[:] = -rng.integers(1, 2 ** 31, P)
    if pattern in ('null_dur', 'null_both'):
        duration = None
    if pattern in ('null_val', 'null_both'):
        value = None
    if pattern in ('start', 'null_dur', 'null_val', 'null_both') and cells <= 1 << 16:
        c['start'] = rng.integers(-2 ** 63, 2 ** 63, (Z + 1, B + 1, 4), dtype=np.int64)
    if pattern == 'start':
        c['times'] = 2
    c.update(matched=matched, zone=zone, key=key, duration=duration, value=value)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def planes(c):
    return {f: c[f] for f in ('matched', 'zone', 'key', 'duration', 'value')}


@functools.lru_cache(maxsize=None)
def case_sparse(pattern, P, Z, B):
    """The reference's (cells, words) of a case, computed once and shared (read-only)."""
    c = case(pattern, P, Z, B)
    cells, words = reference_sparse(c['matched'], c['zone'], c['key'], c['key_lo'], B, Z,
                                    c['duration'], c['value'])
    cells.setflags(write=False)
    words.setflags(write=False)
    return cells, words


def case_dense(pattern, P, Z, B):
    c = case(pattern, P, Z, B)
    return dense(case_sparse(pattern, P, Z, B), Z, B, c['start'], c['times'])


def check_sparse(table, sparse, what):
    """A numpy table that started from zero holds exactly the reference's cells and words."""
    cells, words = sparse
    flat = table.reshape(-1, 4)
    assert np.array_equal(np.flatnonzero((flat != 0).any(axis=1)), cells), what
    assert np.array_equal(flat[cells], words), what


# ---- the host twin ----

def load_host():
    """The host twin (tests/native/zonal_host_check.hip), built by __graft_entry__.build()."""
    if not os.path.exists(ZONALCHECK):
        raise RuntimeError('host twin not built: run __graft_entry__.build()')
    L = ctypes.CDLL(ZONALCHECK)
    vp = ctypes.c_void_p
    L.ltx_zonal_stats.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int64, ctypes.c_int32,
                                  ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp]
    L.ltx_zonal_path.argtypes = [ctypes.c_int32] * 3
    return L


GUARD = 0x5555555555555555


def host_table(lib, c, path=0, expect=LT_OK):
    """ltx_zonal_stats on a case's arrays (copies of exactly n_pix elements), c['times'] times into
    one guarded table that starts from c['start'] -> int64 [n_zones + 1, n_bins + 1, 4]."""
    Z, B = c['n_zones'], c['n_bins']
    n = (Z + 1) * (B + 1) * 4
    buf = np.zeros(n + 16, np.uint64)   # (untouched pages of a large table are never written)
    buf[:8] = buf[8 + n:] = GUARD
    if c['start'] is not None:
        buf[8:8 + n] = c['start'].reshape(-1).view(np.uint64)
    arrs = {f: (None if a is None else np.array(a)) for f, a in planes(c).items()}
    ptr = {f: (None if a is None else a.ctypes.data) for f, a in arrs.items()}
    for _ in range(c['times']):
        rc = lib.ltx_zonal_stats(ptr['matched'], ptr['zone'], ptr['key'], ptr['duration'],
                                 ptr['value'], len(c['matched']), c['key_lo'], B, Z, path,
                                 buf[8:].ctypes.data)
        assert rc == expect, rc
    assert (buf[:8] == GUARD).all() and (buf[8 + n:] == GUARD).all()
    return buf[8:8 + n].view(np.int64).reshape(Z + 1, B + 1, 4)


# ---- the 24 x 40 job ----

SHAPE = (24, 40)
ZONE_NODATA = 255
ZONE_IGNORED = 9
QUADRANT_IDS = (11, 40, 23, 7)   # top-left, top-right, bottom-left, bottom-right: not ascending


def zone_image():
    """The job's zone raster: four quadrant ids, a strip of the GDAL_NODATA value down columns
    18-19, and a block of an id the settings ignore."""
    H, W = SHAPE
    z = np.empty(SHAPE, np.uint8)
    z[:H // 2, :W // 2], z[:H // 2, W // 2:] = QUADRANT_IDS[0], QUADRANT_IDS[1]
    z[H // 2:, :W // 2], z[H // 2:, W // 2:] = QUADRANT_IDS[2], QUADRANT_IDS[3]
    z[:, 18:20] = ZONE_NODATA
    z[3:9, 25:33] = ZONE_IGNORED
    return z


def write_zones(root, job, name='zones.tif', shift=0, dtype=np.uint8, image=None, nodata=ZONE_NODATA):
    """The zone raster into <root>/<job>/input/<name>, on the job's grid moved `shift` pixels
    right and down (so the grid's first `shift` rows and columns fall off it)."""
    from jobfixture import GT
    from land_trendr_amd.raster import write_geotiff
    img = zone_image() if image is None else image
    gt = (GT[0] + shift * GT[1], GT[1], 0.0, GT[3] + shift * GT[5], 0.0, GT[5])
    path = os.path.join(root, job, 'input', name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    write_geotiff(path, np.ascontiguousarray(img.astype(dtype)), geotransform=gt, nodata=nodata)
    return path


def expected_zones(shift=0, ignore=(ZONE_IGNORED,)):
    """(zone index of every pixel of the job's raster order int32 [960], zone ids ascending) by
    the definition: a grid point is its pixel's centre, so pixel (r, c) lies r + 0.5 - shift rows
    and c + 0.5 - shift columns into the zone raster, truncated towards zero as pt2val truncates
    (the pixel half a step before the raster reads its first row or column); a negative offset is
    off the raster. Off the raster, nodata and ignored ids -> -1; the other ids dense in ascending
    order."""
    H, W = SHAPE
    img = zone_image().astype(np.int64)
    ids = np.full(SHAPE, -1, np.int64)
    on = np.zeros(SHAPE, bool)
    for r in range(H):
        for c in range(W):
            zr, zc = int(r + 0.5 - shift), int(c + 0.5 - shift)   # int() truncates towards zero
            if r + 0.5 - shift > -1 and c + 0.5 - shift > -1 and zr < H and zc < W:
                ids[r, c], on[r, c] = img[zr, zc], True
    on &= (ids != ZONE_NODATA) & ~np.isin(ids, list(ignore))
    zone_ids = np.unique(ids[on])
    index = np.full(SHAPE, -1, np.int32)
    index[on] = np.searchsorted(zone_ids, ids[on])
    return index.reshape(-1), zone_ids


def expected_csv(table, zone_ids, years, pixel_area):
    """The CSV text of one table, from the definition: one line per cell with a pixel."""
    lines = ['zone,year,pixels,area,mean_magnitude,mean_duration']
    Z, B = len(zone_ids), len(years)
    for r in range(Z + 1):
        for c in range(B + 1):
            n, dur, q, nv = (int(v) for v in table[r, c])
            if n == 0:
                continue
            lines.append(','.join([
                str(int(zone_ids[r])) if r < Z else 'outside',
                str(int(years[c])) if c < B else 'other', str(n), repr(float(n * pixel_area)),
                repr(q / 16.0 / nv) if nv else '', repr(dur / n)]))
    return '\n'.join(lines) + '\n'


def make_twin_engine():
    """The CPU engine double of changefixture (change_maps, label_counts, sieve over their host
    twins) with a zonal_stats over this one's: host tensors in and out, Engine.zonal_stats'
    signature. For the job's CPU tests only (the product has no CPU path)."""
    import torch

    import changefixture

    class ZonalTwinEngine(type(changefixture.make_twin_engine())):
        def zonal_stats(self, matched, zone, key, key_lo, n_bins, n_zones, duration=None,
                        value=None, out=None, _path=0):
            shape = (n_zones + 1, n_bins + 1, 4)
            if out is None:
                out = torch.zeros(shape, dtype=torch.int64)
            assert out.dtype == torch.int64 and tuple(out.shape) == shape and out.is_contiguous()
            P = matched.numel()
            want = {'matched': torch.uint8, 'zone': torch.int32, 'key': torch.int32,
                    'duration': torch.int32, 'value': torch.float64}
            for f, t in (('matched', matched), ('zone', zone), ('key', key),
                         ('duration', duration), ('value', value)):
                assert t is None or (t.dtype == want[f] and t.numel() == P and
                                     (P <= 1 or t.stride(0) == 1)), f
            rc = load_host().ltx_zonal_stats(
                matched.data_ptr(), zone.data_ptr(), key.data_ptr(),
                None if duration is None else duration.data_ptr(),
                None if value is None else value.data_ptr(), P, key_lo, n_bins, n_zones, _path,
                out.data_ptr())
            assert rc == 0, rc
            return out
    return ZonalTwinEngine()
