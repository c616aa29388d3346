"""Shared by the mask_eqn tests (test_mask_eqn.py, test_gpu_mask.py): the numpy reference of a
mask expression, band arrays with the types' extremes, and a job directory whose rasters carry
a third (QA) band, laid out either for a `mask_eqn` job or for the equivalent `_cloudmask` job."""
import json
import os

import numpy as np

import jobfixture
from land_trendr_amd.raster import write_geotiff
from land_trendr_amd.synth import make_scene

DTYPES = (np.int16, np.uint16, np.uint8, np.int32, np.float32)

# expressions whose literals fit the band type, so that the installed numpy 2.x and the legacy
# promotion MaskProgram follows agree on every node type: (expression, band types)
ALL = DTYPES
SIGNED = (np.int16, np.int32, np.float32)
INTS = (np.int16, np.uint16, np.uint8, np.int32)
CORPUS = [
    ('B3 != 0', ALL),
    ('B1 != -9999', SIGNED),
    ('B3 & 6 == 0', INTS),
    ('(B1 > 0) & (B2 > 0)', ALL),
    ('~(B3 >> 3) & 1 == 1', INTS),
    ('(B4 - B3) / (B4 + B3) > 0', ALL),
    ('B1 == B1', ALL),
    ('(B1 <= B2) | (B3 >= 100) ^ (B2 < 7)', ALL),
    ('~(B1 == 0) == (B2 != 0)', ALL),
    ('(B3 << 1 | 1) & 3 == 3', INTS),
    ('(B2 - B1) * 2 + 1 >= B4 // 3', ALL),
    ('-B1 < 5', SIGNED),
    ('B1 * 0.5 > 0.25', (np.float32,)),
]


def numpy_mask(eqn, bands, numbers=(1, 2, 3, 4)):
    """numpy's own evaluation of the expression text on the band arrays (bands[s] is band
    numbers[s]). The product runs `/` as the reference's Python 2 did, classic division: floor
    division on integer arrays (pinned for index_eqn by test_index_eqn.py), where Python 3's `/`
    is true division; for integer bands the text is therefore evaluated with `//` in its place."""
    names = {'B%d' % n: np.asarray(bands[s]) for s, n in enumerate(numbers)}
    text = eqn
    if np.asarray(bands[0]).dtype.kind in 'iu':
        text = eqn.replace('//', '\0').replace('/', '//').replace('\0', '//')
    with np.errstate(all='ignore'):
        r = eval(text, {'__builtins__': {}}, names)  # test input only, never product code
    assert r.dtype == np.bool_
    return r


def band_values(dtype, shape, seed=0):
    """Random band samples of `dtype` seeded with the type's extremes, 0, -1 (its wrapped value
    for an unsigned type), small flag values and, for floats, NaN and infinities."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    if dtype.kind == 'f':
        a = rng.normal(0, 50, n).astype(dtype)
        special = [0.0, -0.0, -1.0, 1.0, np.nan, np.inf, -np.inf, np.finfo(dtype).max,
                   np.finfo(dtype).min, -9999.0, 0.5]
    else:
        info = np.iinfo(dtype)
        a = rng.integers(info.min, int(info.max) + 1, n, dtype=np.int64).astype(dtype)
        small = rng.integers(-4, 12, n).astype(np.int64).astype(dtype)  # flags, zeros, ties
        a = np.where(rng.random(n) < 0.6, small, a)
        special = [info.min, info.max, 0, np.array(-1).astype(dtype), 1, 6, 8,
                   np.array(-9999).astype(dtype), info.max - 1]
    # every plane along the first axis (a band) gets the special values
    a = a.reshape(shape[0], -1)
    k = min(a.shape[1], len(special))
    for row in a:
        row[rng.choice(a.shape[1], k, replace=False)] = np.array(special[:k], dtype)
    return a.reshape(shape)


SETTINGS_EQN = dict(jobfixture.SETTINGS, mask_eqn='B3 != 0')


def make_mask_job(root, mode, job='synth', rows=9, cols=13, both=False, seed=5):
    """The same int16 three-band rasters (B1, B2 as jobfixture's, B3 a QA band that is 0 on a
    quarter of the pixels) under `root`, for one of two equivalent jobs:
      mode 'eqn'   — settings.json has mask_eqn 'B3 != 0';
      mode 'cloud' — no mask_eqn; every date has a `_cloudmask` raster holding (B3 != 0) with the
                     raster's own georeferencing.
    both: some dates also carry a random cloud mask; the 'cloud' job's mask raster is then its AND
    with (B3 != 0), the 'eqn' job gets the random mask alone.
    Raster 1 is larger than the template, raster 3 smaller (grid points off it), raster 2 has a
    spare fourth band; all are LZW strip files the device decoder takes."""
    GT = jobfixture.GT
    sc = make_scene(rows * cols, n_years=12, k_min=1, k_max=2, mask_prob=0.2, seed=seed,
                    with_bands=True)
    rng = np.random.default_rng(seed + 1)
    rdir = os.path.join(root, job, 'input', 'rasters')
    os.makedirs(rdir, exist_ok=True)
    with open(os.path.join(root, job, 'input', 'settings.json'), 'w') as f:
        json.dump(SETTINGS_EQN if mode == 'eqn' else jobfixture.SETTINGS, f)
    b12 = sc.bands.numpy().astype(np.int16)
    shapes = {1: (14, 19, 2, 3, 3), 2: (rows, cols, 0, 0, 4), 3: (6, 8, -2, -3, 3)}
    for k, d in enumerate(sc.dates):
        stem = 'LT5045029_%d_%03d_20120124_104859' % (d.year, d.timetuple().tm_yday)
        r, c, dy, dx, nb = shapes.get(k, (rows, cols, 0, 0, 3))
        gt = (GT[0] - dx * GT[1], GT[1], 0.0, GT[3] - dy * GT[5], 0.0, GT[5])
        img = rng.integers(-2000, 2000, (nb, r, c)).astype(np.int16)
        qa = rng.choice(np.array([1, 2, 66, 130], np.int16), (r, c))
        img[2] = np.where(rng.random((r, c)) < 0.25, 0, qa)
        # the scene's samples where the raster covers the grid: pixel (y, x) is grid point
        # (y - dy, x - dx), p = x * rows + y (rast2grid's order)
        scene = b12[k].reshape(2, cols, rows).transpose(0, 2, 1)
        for y in range(r):
            for x in range(c):
                if 0 <= y - dy < rows and 0 <= x - dx < cols:
                    img[:2, y, x] = scene[:, y - dy, x - dx]
        write_geotiff(os.path.join(rdir, stem + '_ledaps.tif'), img, geotransform=gt, nodata=None)
        cloud = (rng.random((r, c)) < 0.7) if both and k % 2 == 0 else None
        if mode == 'cloud':
            m = img[2] != 0
            if cloud is not None:
                m &= cloud
        else:
            m = cloud
        if m is not None:
            write_geotiff(os.path.join(rdir, stem + '_cloudmask.tif'), m.astype(np.uint8),
                          geotransform=gt, nodata=None)
    return sc
