"""Generate the wide golden vectors under tests/golden/ by running the REFERENCE itself: scenes of
49-64 years, 5-16 label rules and exactly full 32 / 48 / 64-year instances, and least-squares
segments of 41-64 points. The sizes of make_golden.py's sets stop at 40 years, 5 rules and 40-point
segments.

Needs the reference tree (see ref_shim.py), as make_golden.py does. Outputs are plain arrays,
committed as fixtures:
  wide_<name>.npz   scenes in the layout of scene_<name>.npz (widefixture.WideScene(name),
                    widefixture.wide_names()); mode 'documented' throughout
  lstsq_wide.npz    3000 segments of 41..64 points, x a sorted subset of 0..63 -> reference
                    least_squares: slope, icpt, ssr (the four y kinds of make_golden.make_lstsq)

Run: python tests/golden/make_wide_golden.py   (about a minute on 16 cores)
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
from widefixture import wide_rules  # noqa: E402

PREFIX = 'wide_'


def tie_pixels(n, seed, T):
    """make_golden.tie_pixels with every series T years long."""
    rng = np.random.default_rng(seed)
    px = []
    for _ in range(n):
        kind = rng.integers(0, 3)
        if kind == 0:
            v = rng.integers(0, 4, T) * 100
        elif kind == 1:
            v = np.cumsum(rng.integers(-1, 2, T)) * 50 + 500
        else:
            v = (np.arange(T) % int(rng.integers(2, 5))) * 100
        px.append(mg.yearly(v.tolist(), y0=1990, md='07-01'))
    return px


def make_lstsq_wide(pool, n=3000, seed=41):
    rng = np.random.default_rng(seed)
    M = 64
    xs = np.zeros((n, M), np.float64)
    ys = np.zeros((n, M), np.float64)
    ms = np.zeros(n, np.int32)
    jobs = []
    for t in range(n):
        m = int(rng.integers(41, M + 1))
        x = np.sort(rng.choice(np.arange(0, 64), m, replace=False)).astype(np.float64)
        kind = t % 4
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
    np.savez_compressed(os.path.join(HERE, 'lstsq_wide.npz'), m=ms, x=xs, y=ys, slope=out[:, 0],
                        icpt=out[:, 1], ssr=out[:, 2])
    print('lstsq_wide cases', n, flush=True)


def scenes():
    doc = dict(mode='documented')
    tie16 = wide_rules(16, first_year=1990, n_years=49, thr0=50, thr_step=30)
    return [
        mg.scene_from_synth('y64_r16', 192, 6416, 10, wide_rules(16), n_years=64, **doc),
        mg.scene_from_synth('y64_masks_r5', 128, 6405, 1.0, wide_rules(5), n_years=64, k_min=1,
                            k_max=3, mask_prob=0.2, **doc),
        mg.scene_from_lists('y49_ties_r16', tie_pixels(128, 49, 49), 1e-4, tie16, **doc),
        mg.scene_from_lists('y64_ties_r1', tie_pixels(128, 64, 64), 1e-4, mg.GD, **doc),
        mg.scene_from_synth('y32_r5', 64, 3205, 10, wide_rules(5, n_years=32), n_years=32, **doc),
        mg.scene_from_synth('y48_r1', 64, 4801, 10, mg.GD, n_years=48, **doc),
    ]


def evaluate_wide(sc, pool):
    """make_golden.evaluate_scene, its scene_<name>.npz written to a scratch directory and kept as
    wide_<name>.npz here: golden_io.scene_names() must not see these scenes."""
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
        make_lstsq_wide(pool)
        for sc in scenes():
            evaluate_wide(sc, pool)
    print('done')


if __name__ == '__main__':
    main()
