"""Generate tests/golden/ftv_second.npz: fit-to-vertex vectors made by the REFERENCE itself.

Survey container only (loads the reference through ref_shim.py). For about 300 accepted pixels of
the golden scenes c1, c3, edge and ties2 it takes the scene's own winner / spike / vertex planes
(what the reference's analyze found on the scene's values), makes a SECOND series for the pixel
with a seeded recipe of five kinds, and runs the reference's own vertices2eqns (utils.py:646-669)
and eqns2fitted_points (utils.py:682-722) on that series at those vertices. Data only: plain
arrays (np.savez_compressed, no pickles), committed as a fixture; the GPU box only reads it.

Per scene <s> the file holds
  <s>_pix     [n]      pixel ids in scene_<s>.npz
  <s>_kind    [n]      kind of the pixel's second series (KINDS)
  <s>_second  [K, n]   the second series: its value for every observation of the scene
  <s>_val_fit, <s>_fit_m, <s>_fit_b, <s>_right_m, <s>_right_b   [Y, n], NaN for absent years

Run: python tests/golden/make_ftv_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SCENES = (('c1', 100), ('c3', 100), ('edge', 100), ('ties2', 80))  # (scene, accepted pixels taken)
KINDS = ('int16 noise', 'zero', 'small', 'float', 'walk')
SEED = 1405


def second_series(rng, kind, K):
    """The seeded five-kind recipe; integer kinds stay inside int16."""
    if kind == 0:    # int16 noise over the full range
        return rng.integers(-32768, 32768, K).astype(np.float64)
    if kind == 1:    # all zero: dgelsd's B == 0 shortcut
        return np.zeros(K)
    if kind == 2:    # values in {0, 1, 2}: exact ties between the left and the right eqn
        return rng.integers(0, 3, K).astype(np.float64)
    if kind == 3:    # non-integer floats
        return rng.normal(500.0, 300.0, K)
    return 1000.0 + np.cumsum(rng.integers(-50, 51, K)).astype(np.float64)  # an int random walk


def main():
    import pandas as pd

    import golden_io
    import ref_shim
    utils, _ = ref_shim.load_reference()
    rng = np.random.default_rng(SEED)
    out = {}
    count = total = 0
    for name, take in SCENES:
        g = golden_io.GoldenScene(name)
        years = np.asarray(g.scene.years)
        K, Y = g.values.shape[0], len(years)
        pix = [p for p in range(g.n_pix) if g.err[p] in ('', 'label:AttributeError')][:take]
        n = len(pix)
        kind = np.zeros(n, np.int8)
        second = np.zeros((K, n))
        planes = {f: np.full((Y, n), np.nan) for f in ('val_fit', 'fit_m', 'fit_b', 'right_m',
                                                       'right_b')}
        for i, p in enumerate(pix):
            kind[i] = count % len(KINDS)
            count += 1
            s2 = second_series(rng, int(kind[i]), K)
            second[:, i] = s2
            w = g.ref['winner'][:, p]
            ys = np.nonzero(w >= 0)[0]
            vals = [np.nan if g.ref['spike'][y, p] else s2[w[y]] for y in ys]
            int_series = pd.Series(data=vals, index=[int(years[y] - years[ys[0]]) for y in ys])
            is_vertex = [bool(g.ref['vertex'][y, p]) for y in ys]
            eqns_right = utils.vertices2eqns(int_series, is_vertex)
            vals_fit, eqns_fit = utils.eqns2fitted_points(int_series, eqns_right)
            for t, y in enumerate(ys):
                planes['val_fit'][y, i] = float(vals_fit.iloc[t])
                planes['fit_m'][y, i], planes['fit_b'][y, i] = map(float, eqns_fit.iloc[t])
                planes['right_m'][y, i], planes['right_b'][y, i] = map(float, eqns_right.iloc[t])
        out[name + '_pix'] = np.asarray(pix, np.int32)
        out[name + '_kind'] = kind
        out[name + '_second'] = second
        for f, a in planes.items():
            out['%s_%s' % (name, f)] = a
        total += n
        print('scene %-6s %3d pixels' % (name, n), flush=True)
    path = os.path.join(HERE, 'ftv_second.npz')
    np.savez_compressed(path, kinds=np.array(KINDS), **out)
    print('%d pixels, %d bytes' % (total, os.path.getsize(path)))


if __name__ == '__main__':
    main()
