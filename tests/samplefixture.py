"""The corpus of the grid sampling tests (tests/test_sample_host.py, tests/test_gpu_sample.py): a
raster-order grid of 37 x 53 points, sources of other extents placed by their geotransforms, the
numpy path ingest_stack takes today (grid_offsets, np.take, zero where pt2val raises, the mask
rule) as the reference, and the host build of the sampling core (liblt_io.so lt_grid_sample) run
inside canaries."""
import numpy as np

from land_trendr_amd import ingest, tiffcodec

GT = (500000.0, 30.0, 0.0, 4200000.0, 0.0, -30.0)
H, W = 37, 53
P = H * W
CANARY = 0xA5
PAD = 24  # canary bytes before and after (a multiple of every sample size)

# (rows, cols, dy, dx): a source whose pixel (y, x) lies dy rows / dx columns off grid point (y, x)
SRC_A = (29, 61, -5, 3)      # rows wrap (r < 5) and fall off (r >= 34); the last row is hit
SRC_SMALL = (11, 17, -13, -20)  # smaller than the grid: off on both sides, wraps, last row / column
SRC_MASK = (40, 50, 2, -4)   # a mask with an extent of its own
SOURCES = {'a': SRC_A, 'small': SRC_SMALL}
DTYPES = ('uint8', 'int16', 'uint32', 'float64')
INT_DTYPES = ('uint8', 'int16', 'int32', 'int64')
SELS = ([0], [1, 0], [2, 4])
RANGES = ((0, P), (17, 18), (60, 191), (100, 100))  # whole, one pixel, mid-row to mid-row, n = 0


def axes():
    """(x of each grid column, y of each grid row): the template's pixel centres."""
    return (GT[0] + (np.arange(W) + 0.5) * GT[1], GT[3] + (np.arange(H) + 0.5) * GT[5])


def lnglat():
    xv, yv = axes()
    return np.tile(xv, H), np.repeat(yv, W)


def source_gt(dy, dx):
    return (GT[0] - dx * GT[1], GT[1], 0.0, GT[3] - dy * GT[5], 0.0, GT[5])


def make_src(seed, dtype, spec, bands=6, zeros=0.0):
    rows, cols = spec[:2]
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        a = rng.standard_normal((bands, rows, cols)).astype(dt)
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, (bands, rows, cols), dtype=dt, endpoint=True)
    if zeros:
        a[rng.random(a.shape) < zeros] = 0
    return a, source_gt(*spec[2:])


def offsets(src, gt):
    return ingest.axis_offsets(gt, src.shape[1:], *axes())


def numpy_bands(src, gt, p0, p1, sel):
    """ingest_stack's host path: (planes [len(sel), n], valid [n])."""
    lng, lat = lnglat()
    idx, ok = ingest.grid_offsets(gt, src.shape[1:], lng[p0:p1], lat[p0:p1])
    out = np.take(src.reshape(src.shape[0], -1)[sel], idx, axis=-1)
    out[:, ~ok] = 0
    return out, ok.astype(np.uint8)


def numpy_mask(valid, mask, mgt, p0, p1):
    """v &= ~(mok & (mval == 0)) on a copy of valid."""
    lng, lat = lnglat()
    midx, mok = ingest.grid_offsets(mgt, mask.shape[1:], lng[p0:p1], lat[p0:p1])
    mval = np.take(mask[0].reshape(-1), midx)
    v = valid.copy()
    v &= ~(mok & (mval == 0))
    return v


def padded(n_bytes):
    """A canary-filled byte buffer with PAD bytes around n_bytes."""
    return np.full(n_bytes + 2 * PAD, CANARY, np.uint8)


def host_bands(src, gt, p0, p1, sel, extra=5, threads=3):
    """The host build over pixels p0..p1 with out_stride = n + extra, inside canaries: returns
    (planes [len(sel), n], valid [n]) after checking every canary."""
    n = p1 - p0
    stride = n + extra
    xo, yo = offsets(src, gt)
    ob = padded(len(sel) * stride * src.itemsize)
    vb = padded(n)
    out = ob[PAD:len(ob) - PAD].view(src.dtype).reshape(len(sel), stride)
    valid = vb[PAD:PAD + n]
    tiffcodec.grid_sample(src, xo, yo, p0, n, sel, out, stride, valid, 0, threads=threads)
    assert (ob[:PAD] == CANARY).all() and (ob[len(ob) - PAD:] == CANARY).all()
    assert (out[:, n:].view(np.uint8) == CANARY).all()  # the gap between the planes
    assert (vb[:PAD] == CANARY).all() and (vb[PAD + n:] == CANARY).all()
    return out[:, :n].copy(), valid.copy()


def host_mask(valid, mask, mgt, p0, p1, threads=3):
    n = p1 - p0
    xo, yo = offsets(mask, mgt)
    vb = padded(n)
    vb[PAD:PAD + n] = valid
    tiffcodec.grid_sample(mask, xo, yo, p0, n, [0], None, 0, vb[PAD:PAD + n], 1, threads=threads)
    assert (vb[:PAD] == CANARY).all() and (vb[PAD + n:] == CANARY).all()
    return vb[PAD:PAD + n].copy()


def same(a, b):
    """Exact equality, bytes for floating-point samples."""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
