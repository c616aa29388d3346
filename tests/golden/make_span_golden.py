"""Generate the year-span golden vectors under tests/golden/ by running the REFERENCE itself: scenes
whose calendar years have gaps, so that year offsets run past 63 (up to the accepted span of 255),
and least-squares segments on such offsets. Every other golden set has consecutive years.

Needs the reference tree (see ref_shim.py), as make_golden.py does. Outputs are plain arrays,
committed as fixtures:
  span_<name>.npz   scenes in the layout of scene_<name>.npz (spanfixture.SpanScene(name),
                    spanfixture.span_names()); mode 'documented' throughout. One noise scene per
                    year list of spanfixture.YEAR_LISTS, a tie-heavy one and a collinear one
  lstsq_span.npz    3000 segments of 2..64 points, x a sorted subset of 0..255 with x.max() > 63
                    -> reference least_squares: slope, icpt, ssr (the four y kinds of
                    make_wide_golden.make_lstsq_wide). A third are x-sets the kernels' factor table
                    has a slot for (lt_lapack.h xset_key) that start at offsets 48..63 and end
                    past 63; a third are random subsets; a third dense runs (gaps 1-3) anywhere

Run: python tests/golden/make_span_golden.py   (a few minutes on 8 cores)
"""
import multiprocessing as mp
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402
import make_wide_golden as mwg  # noqa: E402
import spanfixture as sf  # noqa: E402

PREFIX = 'span_'


def span_x(rng, t):
    """The x values of case t: see the module docstring."""
    kind = t % 3
    if kind == 0:  # table-shaped, from an offset of 48..63 to past 63
        while True:
            x0 = int(rng.integers(48, 64))
            shape = int(rng.integers(0, 4))
            if shape == 0:
                gaps = rng.integers(1, 9, 1)
            elif shape == 1:
                gaps = rng.integers(1, 9, 2)
            elif shape == 2:
                gaps = rng.integers(1, 5, 3)
            else:
                gaps = np.ones(int(rng.integers(5, 65)) - 1, np.int64)
            x = x0 + np.concatenate([[0], np.cumsum(gaps)])
            if x[-1] > 63:
                return x
    if kind == 1:
        while True:
            m = int(rng.integers(2, 65))
            x = np.sort(rng.choice(np.arange(0, 256), m, replace=False))
            if x[-1] > 63:
                return x
    while True:
        m = int(rng.integers(2, 65))
        x = int(rng.integers(0, 201)) + np.concatenate([[0], np.cumsum(rng.integers(1, 4, m - 1))])
        if 63 < x[-1] <= 255:
            return x


def make_lstsq_span(pool, n=3000, seed=43):
    rng = np.random.default_rng(seed)
    M = 64
    xs = np.zeros((n, M), np.float64)
    ys = np.zeros((n, M), np.float64)
    ms = np.zeros(n, np.int32)
    jobs = []
    for t in range(n):
        x = span_x(rng, t).astype(np.float64)
        m = len(x)
        kind = (t // 3) % 4  # every x kind meets every y kind
        if kind == 0:
            y = rng.integers(-500, 1500, m).astype(np.float64)
        elif kind == 1:
            y = rng.normal(500, 300, m)
        elif kind == 2:
            y = np.round(rng.normal(0, 40, m)) + np.arange(m) * rng.integers(-50, 50)
        else:  # small integers: many exact rational ties in the DP
            y = rng.integers(0, 4, m).astype(np.float64) * 100
        xs[t, :m], ys[t, :m], ms[t] = x, y, m
        jobs.append((x.astype(np.int64), y))
    out = np.array(pool.map(mg._lstsq_case, jobs, chunksize=64))
    np.savez_compressed(os.path.join(HERE, 'lstsq_span.npz'), m=ms, x=xs, y=ys, slope=out[:, 0],
                        icpt=out[:, 1], ssr=out[:, 2])
    print('lstsq_span cases', n, flush=True)


def scene_on(name, ylist, values, valid, line_cost, rules):
    """A scene description (make_golden.evaluate_scene's input) of values [Y, P] on the July 1 of
    the years of spanfixture.YEAR_LISTS[ylist]."""
    valid = np.ones(values.shape, np.uint8) if valid is None else valid
    return dict(name=name, dates=[d.isoformat() for d in sf.dates_of(ylist)],
                values=np.ascontiguousarray(values, np.float64), valid=valid, line_cost=line_cost,
                rules=rules, target=sf.TARGET, mode='documented')


def tie_scene(name, ylist, n, seed, line_cost, rules):
    """make_wide_golden.tie_pixels with each series on the list's years."""
    Y = len(sf.YEAR_LISTS[ylist])
    px = mwg.tie_pixels(n, seed, Y)
    vals = np.array([[d['val'] for d in p] for p in px], np.float64).T  # [Y, n]
    return scene_on(name, ylist, vals, None, line_cost, rules)


def scenes():
    out = []
    for ylist, years in sf.YEAR_LISTS.items():  # c2-like: one observation a year, GD, line cost 10
        n = 128 if len(years) == 64 else 192
        out.append(scene_on(ylist, ylist, sf.noise_values(ylist, n), sf.span_mask(ylist, n), 10,
                            sf.GD))
    out.append(tie_scene('biennial_y64_ties', 'biennial_y64', 128, 126, 1e-4, sf.GD))
    out.append(scene_on('span255_y64_collinear', 'span255_y64',
                        sf.collinear_values('span255_y64', 128, 255), None, 1.0, sf.GD))
    return out


def evaluate_span(sc, pool):
    """make_golden.evaluate_scene, its scene_<name>.npz written to a scratch directory and kept as
    span_<name>.npz here: golden_io.scene_names() must not see these scenes."""
    with tempfile.TemporaryDirectory() as tmp:
        here, mg.HERE = mg.HERE, tmp
        try:
            mg.evaluate_scene(sc, pool)
        finally:
            mg.HERE = here
        shutil.move(os.path.join(tmp, 'scene_%s.npz' % sc['name']),
                    os.path.join(HERE, '%s%s.npz' % (PREFIX, sc['name'])))


def main():
    n = max(1, min(16, os.cpu_count() or 1))
    with mp.Pool(n) as pool:
        make_lstsq_span(pool)
        for sc in scenes():
            evaluate_span(sc, pool)
    print('done')


if __name__ == '__main__':
    main()
