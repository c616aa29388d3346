"""Shared inputs of the year-span tests (tests/test_span_host.py, tests/test_gpu_span.py) and of
tests/golden/make_span_golden.py: scenes whose calendar years have gaps, so a pixel's year offsets
(year - its first present year, the x of every least-squares fit) go past 63, up to the accepted
span of 255 (lt_abi.hip scene_from). The other fixtures have consecutive years: x <= 63. Past 63
the kernels take the wide zero-residual bound and vertex-fit width (lt_pixel.h zero_bound,
fit_width_factor), and the x-set factor table (lt_lapack.h xset_key) is read at slots whose x-set
ends above 63. Nothing here needs a GPU."""
import datetime as dt
import glob
import json
import os

import numpy as np

import golden_io
import widefixture as wf
from land_trendr_amd.scene import build_scene, parse_date
from land_trendr_amd.settings import compile_params
from land_trendr_amd.synth import make_scene

TARGET = wf.TARGET
GD = wf.GD
P = 1061  # 16 full waves and a partial one


def _gaps(n, hi, total, seed):
    """n seeded gaps of 1..hi years that sum to total."""
    rng = np.random.default_rng(seed)
    g = rng.integers(1, hi + 1, n)
    while g.sum() != total:
        i = int(rng.integers(n))
        step = 1 if g.sum() < total else -1
        if 1 <= g[i] + step <= hi:
            g[i] += step
    return g


def _from_gaps(first, gaps):
    return [int(y) for y in first + np.concatenate([[0], np.cumsum(gaps)])]


# name: the calendar years, one observation each on July 1
YEAR_LISTS = {
    # 32 consecutive years, then one year at offset 63: the control, every offset <= 63
    'span63_y33': list(range(1951, 1983)) + [2014],
    # the same with the last year at offset 64: the wide bounds at the smallest offset past 63
    'span64_y33': list(range(1950, 1982)) + [2014],
    # every second year: 64 slots, span 126
    'biennial_y64': list(range(1888, 2015, 2)),
    # one early year, then a dense run across offset 63: 64 slots, span 113
    'late_dense_y64': [1900] + list(range(1951, 2014)),
    # 30 slots over the full span, gaps of 1-16: the 32-slot instances and their 32-bit masks
    # (seed 31: offsets 61, 63, 71 lie side by side)
    'span255_y30': _from_gaps(1759, _gaps(29, 16, 255, 31)),
    # 64 slots over the full span, gaps of 1-8
    'span255_y64': _from_gaps(1759, _gaps(63, 8, 255, 64)),
}
CONTROL = 'span63_y33'


def offsets(name):
    y = np.array(YEAR_LISTS[name])
    return y - y[0]


def straddling_triples(name):
    """Slots a, a+1, a+2 with off[a] <= 63 < off[a+2] and both gaps <= 8: three neighbouring points
    of an unmasked pixel whose x-set has a slot in the factor table (xset_key, m = 3: x0 <= 63,
    gaps <= 8) and ends past offset 63."""
    off = offsets(name)
    return [a for a in range(len(off) - 2)
            if off[a] <= 63 < off[a + 2] and off[a + 1] - off[a] <= 8 and off[a + 2] - off[a + 1] <= 8]


def straddling_run(name):
    """The longest run of consecutive calendar years (in slots) that starts at an offset <= 63 and
    ends past 63: the table's m >= 5 keys."""
    off = offsets(name)
    best = 0
    for a in range(len(off)):
        b = a
        while b + 1 < len(off) and off[b + 1] - off[b] == 1:
            b += 1
        if off[a] <= 63 < off[b]:
            best = max(best, b - a + 1)
    return best


def _check_lists():
    for name, years in YEAR_LISTS.items():
        off = offsets(name)
        assert (np.diff(off) >= 1).all() and len(years) <= 64 and years[-1] <= 2014, name
    assert [len(v) for v in YEAR_LISTS.values()] == [33, 33, 64, 64, 30, 64]
    assert [int(offsets(n)[-1]) for n in YEAR_LISTS] == [63, 64, 126, 113, 255, 255]
    assert np.diff(offsets('span255_y30')).max() <= 16 and np.diff(offsets('span255_y64')).max() <= 8
    # the lists that reach a table slot whose x-set ends past offset 63. span64_y33 cannot: its only
    # offset past 63 lies 33 years after its neighbour, beyond every gap the table holds, so it
    # runs the wide bounds and the factor-on-the-fly path alone (a second control for the table)
    for name in YEAR_LISTS:
        assert bool(straddling_triples(name)) == (name not in (CONTROL, 'span64_y33')), name
    assert straddling_run('late_dense_y64') >= 5


_check_lists()


def dates_of(name):
    return [dt.date(y, 7, 1) for y in YEAR_LISTS[name]]


def meta_of(name):
    return build_scene(dates_of(name), parse_date(TARGET))


def span_mask(name, P, seed=113):
    """The cloud mask of a list's scenes: None, but for late_dense_y64 year 1900 is dropped for
    every third pixel (lanes with x <= 62 beside lanes with x up to 113 in every wave) and 20 % of
    all observations at random."""
    if name != 'late_dense_y64':
        return None
    rng = np.random.default_rng(seed)
    valid = (rng.random((len(YEAR_LISTS[name]), P)) >= 0.2).astype(np.uint8)
    valid[0, np.arange(P) % 3 == 0] = 0
    return valid


def noise_values(name, P, seed=None):
    """synth.make_scene's values (one observation a year) on the list's dates: [Y, P] float64."""
    Y = len(YEAR_LISTS[name])
    seed = 7000 + sorted(YEAR_LISTS).index(name) if seed is None else seed
    return make_scene(P, n_years=Y, seed=seed).values.numpy()


def span_rules(name, n_rules):
    """wide_rules with the onset years spread over the list's span."""
    years = YEAR_LISTS[name]
    return wf.wide_rules(n_rules, first_year=years[0], n_years=years[-1] - years[0] + 1)


def noise_case(name, line_cost, P=P, n_rules=1):
    """(meta, params, values [Y, P], valid or None) of the list's noise scene."""
    params, _ = compile_params(line_cost, span_rules(name, n_rules), 'documented')
    return meta_of(name), params, noise_values(name, P), span_mask(name, P)


def tie_case(name, line_cost, P=1024):
    """widefixture.tie_values on the list's dates under the GD / LD pair: exact rational ties, so
    the analyze kernel defers pixels to the resolve stage."""
    Y = len(YEAR_LISTS[name])
    _, vals = wf.tie_values(Y, P, 4242 + Y)
    params, _ = compile_params(line_cost, wf.GD_LD, 'documented')
    return meta_of(name), params, vals, None


def collinear_values(name, P, seed):
    """Continuous piecewise-linear integer series, exactly collinear in calendar years inside each
    piece (2-9 slots long, integer slope), within int16: [Y, P] float64. Every piece of three or
    more points has a zero residual."""
    rng = np.random.default_rng(seed)
    years = np.array(YEAR_LISTS[name])
    Y = len(years)
    vals = np.zeros((Y, P), np.int64)
    for p in range(P):
        v = int(rng.integers(-3000, 3000))
        vals[0, p] = v
        t = 0
        while t < Y - 1:
            run = int(rng.integers(1, 9))
            slope = int(rng.integers(-12, 13))
            end = min(Y - 1, t + run)
            if abs(v + slope * int(years[end] - years[t])) > 12000:
                slope = -slope
            for u in range(t + 1, end + 1):
                vals[u, p] = v + slope * int(years[u] - years[t])
            v = int(vals[end, p])
            t = end
    assert np.abs(vals).max() <= 32000
    return vals.astype(np.float64)


def collinear_case(name, line_cost, P=P):
    params, _ = compile_params(line_cost, GD, 'documented')
    seed = 9000 + sorted(YEAR_LISTS).index(name)
    return meta_of(name), params, collinear_values(name, P, seed), None


def span_names():
    """The span golden scenes (tests/golden/span_<name>.npz, make_span_golden.py)."""
    return sorted(os.path.basename(p)[5:-4]
                  for p in glob.glob(os.path.join(golden_io.GOLDEN, 'span_*.npz')))


class SpanScene(golden_io.GoldenScene):
    """golden_io.GoldenScene of tests/golden/span_<name>.npz (the same array layout)."""

    def __init__(self, name):
        z = np.load(os.path.join(golden_io.GOLDEN, 'span_%s.npz' % name))  # allow_pickle=False
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
