"""Shared inputs of the wide-instance tests (tests/test_wide_host.py, tests/test_gpu_wide.py) and
of tests/golden/make_wide_golden.py: scenes of 32-64 years with 1-16 label rules, the sizes at which
the analyze / resolve kernels are other (MAXY, RMAX) instances (lt_dispatch.hip) than the ones the
30- and 40-year tests run. Every series has consecutive calendar years; gaps come from masks only.
Nothing here needs a GPU."""
import datetime as dt
import glob
import json
import os

import numpy as np

import golden_io
from land_trendr_amd.scene import build_scene, parse_date
from land_trendr_amd.settings import compile_params
from land_trendr_amd.synth import make_scene

TARGET = '2014-07-01'
GD = [{'name': 'gd', 'val': 1, 'change_type': 'GD'}]
GD_LD = [{'name': 'gd', 'val': 1, 'change_type': 'GD'}, {'name': 'ld', 'val': 2, 'change_type': 'LD'}]


def wide_names():
    """The wide golden scenes (tests/golden/wide_<name>.npz, make_wide_golden.py). They are kept
    apart from golden_io.scene_names(), whose every user runs every scene."""
    return sorted(os.path.basename(p)[5:-4]
                  for p in glob.glob(os.path.join(golden_io.GOLDEN, 'wide_*.npz')))


class WideScene(golden_io.GoldenScene):
    """golden_io.GoldenScene of tests/golden/wide_<name>.npz (the same array layout), for
    golden_io.compare and the fixtures that take a GoldenScene."""

    def __init__(self, name):
        z = np.load(os.path.join(golden_io.GOLDEN, 'wide_%s.npz' % name))  # allow_pickle=False
        self.name = name
        self.meta = json.loads(str(z['meta']))
        self.values = z['values']
        self.valid = z['valid']
        self.err = [str(e) for e in z['err']]
        self.ref = {k: z[k] for k in z.files if k not in ('meta', 'values', 'valid', 'err')}
        self.scene = build_scene(self.meta['dates'], parse_date(self.meta['target']))
        self.params, self.rules = compile_params(self.meta['line_cost'], self.meta['rules'],
                                                 self.meta['mode'])
        assert list(self.scene.years) == self.meta['years']


def bits_equal(a, b):
    """Element-wise equality, floats by their bits (any NaN equal to any NaN)."""
    if a.dtype.kind == 'f':
        return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def wide_rules(n, first_year=1985, n_years=64, thr0=900, thr_step=40):
    """n <= 16 label rules: FD / GD / LD in turn; of every four, one unfiltered, one with an
    onset_year filter ('>=', '<=', '=' in turn, years spread over the scene), one with a duration
    filter ('>', '<') and one with a pre_threshold filter ('>', '<'; thr0 + thr_step * r). Rules 12
    and 14 of a 16-rule set repeat rules 1 and 3 under another name and val: two rule slots with the
    same decisions and different class values. One rule alone is the plain GD rule."""
    if n == 1:
        return [dict(GD[0])]
    out = []
    for r in range(16):
        d = {'name': 'r%d' % r, 'val': r + 1, 'change_type': ('FD', 'GD', 'LD')[r % 3]}
        g = r // 4
        if r % 4 == 1:
            d['onset_year'] = [('>=', '<=', '=')[g % 3], first_year + (2 * r + 1) * n_years // 32]
        elif r % 4 == 2:
            d['duration'] = [('>', '<')[g % 2], 1 + g]
        elif r % 4 == 3:
            d['pre_threshold'] = [('>', '<')[g % 2], thr0 + thr_step * r]
        out.append(d)
    for r, src in ((12, 1), (14, 3)):
        out[r] = dict(out[src], name='r%d' % r, val=r + 1)
    return out[:n]


def tie_values(T, P, seed):
    """The generator of test_tie_heavy_small_integers_tiny_line_cost_vs_oracle at T years: [T, P]
    small integers (levels of 100, unit random walks, short periods of 7) whose segment costs tie
    exactly, so many pixels are deferred to the exact DP of the resolve stage."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, P)
    vals = np.where(kind[None, :] == 0, rng.integers(0, 4, (T, P)) * 100,
                    np.where(kind[None, :] == 1, np.cumsum(rng.integers(-1, 2, (T, P)), 0),
                             (np.arange(T)[:, None] % rng.integers(2, 5, P)[None, :]) * 7))
    dates = [dt.date(1985 + t, 7, 1) for t in range(T)]
    return dates, vals.astype(np.float64)


def synth_case(years, n_rules, line_cost, P, seed=None, **kw):
    """A make_scene scene of `years` years with wide_rules(n_rules), as (meta, params, values
    [K, P] float64, valid [K, P] uint8 or None)."""
    sc = make_scene(P, n_years=years, seed=years * 100 + n_rules if seed is None else seed, **kw)
    meta = build_scene(sc.dates, parse_date(TARGET))
    params, _ = compile_params(line_cost, wide_rules(n_rules, n_years=years), 'documented')
    return meta, params, sc.values.numpy(), None if sc.valid is None else sc.valid.numpy()


def tie_case(T, rules, line_cost, P=1024):
    """tie_values(T, P, 4242 + T) under `rules` (a list of rule dicts)."""
    dates, vals = tie_values(T, P, 4242 + T)
    meta = build_scene(dates, parse_date(TARGET))
    params, _ = compile_params(line_cost, rules, 'documented')
    return meta, params, vals, None


def tie_rules16(T):
    """16 rules with pre_threshold values among the tie generator's levels."""
    return wide_rules(16, n_years=T, thr0=-40, thr_step=20)


def mixed_case(n_rules, P, line_cost=10.0, seed=65):
    """64 years, one observation a year; pixel p keeps p % 65 of them (0..64 points) chosen at
    random, so every wave mixes empty, single-year and full series."""
    rng = np.random.default_rng(seed)
    meta, params, vals, _ = synth_case(64, n_rules, line_cost, P, seed=seed)
    keep = np.arange(P) % 65
    order = np.argsort(rng.random((64, P)), axis=0)
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.arange(64)[:, None] * np.ones((1, P), np.int64), axis=0)
    return meta, params, vals, (rank < keep[None, :]).astype(np.uint8)


def obs_limit_case(P=256):
    """64 years x 16 observations a year = LT_MAX_OBS observations, 30 % masked."""
    return synth_case(64, 1, 10.0, P, seed=71, k_min=16, k_max=16, mask_prob=0.3)


def wide_values_case(years, P):
    """16 rules on values binary32 cannot hold (integers + 0.1). Binary64 values with more than 4
    rules take the binary32 analyze instance (lt_kernels.h series_kind), which sends such pixels to
    the binary64 resolve instance: here every pixel, so resolve<MAXY, 16, double> does all the
    work."""
    meta, params, vals, valid = synth_case(years, 16, 1.0, P, seed=years * 100 + 77)
    vals = vals + 0.1
    assert (vals.astype(np.float32).astype(np.float64) != vals).all()
    return meta, params, vals, valid


# §b of the wide GPU tests and their host twin: every (years, rules) pair, the line cost rotating
# through 10, 1 and 0.5 (early exits and deep starts)
MATRIX = [(y, r) for y in (32, 33, 48, 49, 64) for r in (1, 4, 5, 16)]


def matrix_case(years, n_rules, P):
    lc = (10.0, 1.0, 0.5)[MATRIX.index((years, n_rules)) % 3]
    return synth_case(years, n_rules, lc, P)
