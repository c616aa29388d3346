"""The lazy DP's first start of >= 3 points priced as a triple (lt_pixel.h dp_triple_sse,
LT_DP_TRIPLE), on the host through liblt_hostcheck.so:

(a) the helper's formula, restated here in numpy with the helper's own operations, against the
    exact rational residual and against the emulated dgelsd residual ltx_lstsq (what the reference
    prices the start with): the error stays below the bound derived beside the helper, and that
    bound below the screening constant kScreen; N == 0 exactly where rational arithmetic says the
    three points are collinear;
(b) the argmins of dp_lazy, which prices every triple with the helper, equal those of the exact-OPT
    DP on every column it decides, over series families of which it defers at most a fifth each.
"""
import ctypes
import json
import math
import os
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, 'tests', 'native', 'build', 'liblt_hostcheck.so')
U = 2.0 ** -53
K_SCREEN = 2.0 ** -30
COSTS = (1e-4, 1.0, 10.0, 1000.0)
DEFER_CAP = 0.2
u8p = ctypes.POINTER(ctypes.c_uint8)
f64p = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope='module')
def hc():
    if not os.path.exists(HOSTCHECK):
        pytest.fail('host harness not built: run __graft_entry__.build()')
    L = ctypes.CDLL(HOSTCHECK)
    L.ltx_dp_lazy.argtypes = [ctypes.c_int, u8p, f64p, ctypes.c_double, u8p,
                              ctypes.POINTER(ctypes.c_int)]
    L.ltx_dp_lazy.restype = ctypes.c_uint64
    L.ltx_dp_exact.argtypes = [ctypes.c_int, u8p, f64p, ctypes.c_double, u8p]
    L.ltx_lstsq.argtypes = [ctypes.c_int, f64p, f64p, ctypes.c_int, f64p]
    return L


# ---- the bounds (lt_pixel.h dp_triple_sse; the dgelsd side as tests/test_screening_bounds.py) ----
def rcp_newton_err():
    """Relative error of v_rcp_f64 + one Newton step as measured (tools/rcp_check.hip), doubled."""
    with open(os.path.join(ROOT, 'profiles', 'r05_rcp_check.json')) as f:
        return max(2.0 * json.load(f)['rcp_newton_max_rel_err'], 2.0 * U)


def b_triple_int():
    """int16 values, offsets <= 255: N, N^2 and the denominator exact; the reciprocal and one
    product round."""
    return (rcp_newton_err() + 2 * U) * (1 + 2.0 ** -40)


def b_triple_float():
    """Any binary64 values: 16.4 u max(y)^2 from the roundings inside N, over |w|^2 >= 1.5 g^2."""
    return (16.4 * U + rcp_newton_err() + 2 * U) * (1 + 2.0 ** -40)


def b_lapack(x):
    """The emulated dgelsd residual's a-priori error relative to Syy (test_screening_bounds.py (B):
    Householder steps with gamma~(m) = gamma(8 m), the residual subspace moved by the perturbed
    x column)."""
    m = len(x)
    xa = np.asarray(x, float)
    g8 = 8 * m * U / (1 - 8 * m * U)
    eta = g8 * (float(np.linalg.norm(xa) / np.linalg.norm(xa - xa.mean())) + 2.0)
    g = m * U / (1 - m * U)
    return (2 * eta + eta * eta + g) * (1 + g)


def triple_sse(x, y):
    """dp_triple_sse's operations on binary64 (the fma through rationals: a Fraction converts to
    the nearest binary64), with the host's division in place of the device's reciprocal, whose
    measured error the bounds carry."""
    d1, d2 = int(x[2] - x[1]), int(x[1] - x[0])
    y0, y1, y2 = np.float64(y[2]), np.float64(y[1]), np.float64(y[0])
    p = np.float64(d1) * (y1 - y2)
    n = np.float64(float(F(d2) * F(float(y0 - y1)) - F(float(p))))
    den = np.float64(2 * (d1 * (d1 + d2) + d2 * d2))
    return max(n * n / den, 0.0), float(n), float(y0 * y0 + y1 * y1 + y2 * y2)


def exact_sse(x, y):
    d1, d2 = int(x[2] - x[1]), int(x[1] - x[0])
    n = d2 * (F(y[2]) - F(y[1])) - d1 * (F(y[1]) - F(y[0]))
    return n * n / (2 * (d1 * d1 + d1 * d2 + d2 * d2)), n, sum(F(v) * F(v) for v in y)


def _x_sets(rng):
    out = []
    for a in (1, 2, 3):
        for b in (1, 2, 3):
            out.append((0, b, a + b))           # gaps 1-3 at the origin
            out.append((60, 60 + b, 60 + a + b))
            out.append((255 - a - b, 255 - a, 255))  # reaching the largest offset
    out += [(0, 1, 255), (0, 254, 255), (0, 127, 255), (0, 128, 255), (252, 253, 255)]
    for _ in range(10):
        out.append(tuple(sorted(rng.choice(256, 3, replace=False).tolist())))
    return out


def _int_triples(rng):
    ext = (32767.0, -32767.0)
    ys = [(e0, e1, e2) for e0 in ext for e1 in ext for e2 in ext]
    ys += [(32767.0, 0.0, -32767.0), (-32767.0, 1.0, 32767.0), (1200.0, 1187.0, 1240.0),
           (20000.0, 20001.0, 19999.0), (100.0, 100.0, 30000.0), (0.0, 0.0, 1.0)]
    for _ in range(12):
        ys.append(tuple(float(v) for v in rng.integers(-32767, 32768, 3)))
    for _ in range(6):  # nearly collinear: a line plus one unit
        s, b = int(rng.integers(-100, 101)), int(rng.integers(-5000, 5000))
        ys.append(('line', s, b, int(rng.integers(-1, 2))))
    return ys


def _values(x, y):
    if y[0] == 'line':
        _, s, b, off = y
        return (float(b + s * x[0]), float(b + s * x[1] + off), float(b + s * x[2]))
    return y


def test_formula_against_exact_and_dgelsd_residuals(hc):
    rng = np.random.default_rng(31)
    out3 = np.zeros(3)
    n = 0
    worst = {'int_exact': 0.0, 'int_lapack': 0.0, 'float_exact': 0.0, 'float_lapack': 0.0}
    assert b_triple_int() < b_triple_float() < 2.0 ** -47
    for x in _x_sets(rng):
        bl = b_lapack(x)
        # the derived bounds lie far inside the screening constant
        assert bl + b_triple_float() < K_SCREEN
        xa = np.array(x, np.float64)
        cases = [('int', _values(x, y)) for y in _int_triples(rng)]
        for _ in range(8):  # binary32 values: index programs that divide or scale
            cases.append(('float', tuple(float(np.float32(v)) for v in
                                         rng.normal(0, 1, 3) * 10.0 ** rng.integers(-3, 5))))
        for k in range(4):  # binary32 values with heavy cancellation in N
            base = float(np.float32(rng.normal(0, 1) * 1e4))
            cases.append(('float', tuple(float(np.float32(base + (k > 1) * i * 0.37 + d))
                                         for i, d in zip(x, rng.normal(0, 1e-3, 3)))))
        for kind, y in cases:
            ya = np.array(y, np.float64)
            e, N, syy = triple_sse(x, ya)
            ex, Nx, syyx = exact_sse(x, y)
            if syyx == 0:
                continue
            bt = b_triple_int() if kind == 'int' else b_triple_float()
            if kind == 'int':
                assert F(N) == Nx and abs(N) < 2 ** 26, (x, y)  # the numerator is exact
            err = float(abs(F(e) - ex) / syyx)
            assert err <= bt, (x, y, err, bt)
            assert hc.ltx_lstsq(3, xa.ctypes.data_as(f64p), ya.ctypes.data_as(f64p), 0,
                                out3.ctypes.data_as(f64p)) >= 0
            errl = float(abs(F(e) - F(float(out3[2]))) / syyx)
            assert errl <= bl + bt, (x, y, errl, bl + bt)
            assert errl * float(syyx) <= K_SCREEN * syy
            worst[kind + '_exact'] = max(worst[kind + '_exact'], err / bt)
            worst[kind + '_lapack'] = max(worst[kind + '_lapack'], errl / (bl + bt))
            n += 1
    print('%d triples; worst error / bound: %s' % (n, {
        k: '2^%.1f' % math.log2(v or 2.0 ** -99) for k, v in worst.items()}))
    assert n > 1500


def test_numerator_is_zero_exactly_on_collinear_triples():
    rng = np.random.default_rng(32)
    n_zero = n_not = 0
    for x in _x_sets(rng):
        d1, d2 = x[2] - x[1], x[1] - x[0]
        for _ in range(40):
            s = int(rng.integers(-128, 129))
            # a line through integer points that stays inside int16 over the offsets, then one
            # value moved by -1, 0 or 1, and slopes p / d2 that are integers only at the points
            b = int(rng.integers(-32767 + 128 * 255, 32768 - 128 * 255)) - s * x[0]
            for off in (-1, 0, 0, 1):
                y = (float(b + s * x[0]), float(b + s * x[1] + off), float(b + s * x[2]))
                assert max(abs(v) for v in y) <= 32767
                _, N, _ = triple_sse(x, y)
                _, Nx, _ = exact_sse(x, y)
                assert (N == 0.0) == (Nx == 0) == (off == 0), (x, y)
                n_zero += off == 0
                n_not += off != 0
        # the same rise per unit of x with a non-integer slope: y = (0, p d2, p (d1 + d2)) / g
        g = math.gcd(d1, d2)
        p = int(rng.integers(1, 60))
        y = (0.0, float(p * d2 // g), float(p * (d1 + d2) // g))
        _, N, _ = triple_sse(x, y)
        assert N == 0.0 and exact_sse(x, y)[1] == 0, (x, y)
        n_zero += 1
    assert n_zero > 1000 and n_not > 1000


# ---- (b) series families: (x offsets, y) ----
def _gaps(rng, n, lo, hi):
    return np.cumsum(rng.integers(lo, hi + 1, n)) - 1


def _c2_like(rng):
    """The bench's synthetic pixel: a level, a drop with partial recovery, noise of sigma 40;
    30 years with 5 % of the points removed."""
    t = np.arange(30)
    d, drop = rng.integers(3, 26), rng.integers(100, 801)
    rec = np.minimum(rng.integers(0, drop // 10 + 1) * np.maximum(t - d, 0), drop)
    y = rng.integers(200, 1501) - np.where(t < d, 0, drop - rec) + np.round(rng.normal(0, 40, 30))
    keep = rng.random(30) >= 0.05
    keep[rng.integers(0, 30)] = True
    return t[keep], y[keep]


def _smooth(rng):
    """Piecewise-linear with x gaps of 1-3, long segments win: values in the thousands with noise
    of sigma 20, or (every second series) small values with noise of +-2, where the zero path's
    condition on Syy holds at every cost."""
    n = int(rng.integers(12, 31))
    x = _gaps(rng, n, 1, 3)
    if rng.random() < 0.5:
        y = np.full(n, float(rng.integers(500, 3000)))
        for _ in range(int(rng.integers(1, 4))):
            y = y + rng.integers(-60, 61) * np.maximum(x - x[rng.integers(1, n - 1)], 0)
        return x, y + np.round(rng.normal(0, 20, n))
    y = np.full(n, float(rng.integers(-20, 21)))
    for _ in range(int(rng.integers(1, 3))):
        y = y + rng.integers(-2, 3) * np.maximum(x - x[rng.integers(1, n - 1)], 0)
    return x, y + rng.integers(-2, 3, n)


def _collinear_runs(rng):
    """Exactly collinear runs (integer slopes, gaps 1-2) joined by jumps: runs of 3-8 points of
    values in the hundreds, or (every second series) runs of 3-5 points of small values."""
    small = rng.random() < 0.5
    xs, ys = [], []
    x, y = 0, int(rng.integers(-10, 10) if small else rng.integers(-500, 500))
    while len(xs) < 24:
        s = int(rng.integers(-2, 3) if small else rng.integers(-20, 21))
        for _ in range(int(rng.integers(3, 6 if small else 9))):
            xs.append(x)
            ys.append(y)
            g = int(rng.integers(1, 3))
            x, y = x + g, y + s * g
        y += int(rng.integers(-6, 7) if small else rng.integers(-300, 301))
    return np.array(xs[:30]), np.array(ys[:30], float)


def _one_line(rng):
    """Every triple collinear, gaps of 1-3: a plateau of a small level, a line of slope +-1 through
    zero (at most 9 points), or (two series in five) a line of slope up to +-20 at a level in the
    hundreds, whose residuals no longer round away at the smallest cost."""
    n = int(rng.integers(3, 31))
    x = _gaps(rng, n, 1, 3)
    k = rng.random()
    if k < 0.3:
        return x, np.full(n, float(rng.integers(-14, 15)))
    if k < 0.6:
        x = x[:min(n, 9)]
        return x, (int(rng.choice([-1, 1])) * (x - x[len(x) // 2])).astype(float)
    return x, (int(rng.integers(-300, 300)) + int(rng.integers(-20, 21)) * x).astype(float)


def _extremes(rng):
    """Noisy series (sigma 8000) with three values in ten at the extremes of int16, gaps of 1-3;
    one series in ten a plateau or a line that ends at an extreme."""
    n = int(rng.integers(4, 31))
    x = _gaps(rng, n, 1, 3)
    if rng.random() < 0.1:
        s = int(rng.integers(-300, 301)) * int(rng.integers(0, 2))
        top = int(rng.choice([-32767, 32767]))
        y = top - abs(s) * (x[-1] - x) * (1 if top > 0 else -1)
        return x, y.astype(float)
    y = np.round(rng.normal(0, 8000, n)).clip(-32767, 32767)
    ext = np.where(rng.random(n) < 0.5, 32767.0, -32767.0)
    return x, np.where(rng.random(n) < 0.3, ext, y)


def _short(rng):
    n = int(rng.integers(1, 5))
    return _gaps(rng, n, 1, 3), np.round(rng.normal(1000, 40, n))


def _wide(rng):
    """c2-like noise on year offsets that reach 255 (gaps of 5-9)."""
    n = int(rng.integers(20, 27))
    x = _gaps(rng, n, 5, 9)
    x = x + (255 - x[-1])
    return x, np.round(rng.integers(200, 1501) + rng.normal(0, 40, n))


def _ties(rng):
    """Values 0..3 on gaps of 1-2 (the family of tests/test_dp_neighbour_bound.py, unchanged): many
    exactly collinear small-integer triples and exact ties between starts, where the N == 0 zero
    path and the first-minimum rule decide at every cost."""
    n = int(rng.integers(5, 25))
    return _gaps(rng, n, 1, 2), rng.integers(0, 4, n).astype(float)


# The families of tests/test_dp_neighbour_bound.py: c2_like, ties and short as they are there;
# smooth and collinear changed to meet the cap on deferred series, which that file does not
# assert. As written there (noise of +-2 around values in the thousands; runs of values in the
# hundreds) today's dp_lazy defers 30 % of the smooth series over the four costs (69 % at cost
# 1e-4) and 25 % of the collinear ones (every one at 1e-4: with Syy of the order of 10^6 the
# residual of a collinear segment does not round away against so small a cost, the zero path is
# refused and the near ties stay ambiguous). Here smooth takes noise of sigma 20 and every second
# series of either family small values: 3 % and 12 % deferred. The collinear series of large
# values are still all deferred at 1e-4, so at that cost only the small-valued ones are compared;
# at 1, 10 and 1000 both kinds are. one_line, extremes and wide are new.
FAMILIES = (('c2_like', _c2_like, 300), ('smooth', _smooth, 200),
            ('collinear', _collinear_runs, 150), ('one_line', _one_line, 150),
            ('extremes', _extremes, 150), ('short', _short, 80), ('wide', _wide, 100),
            ('ties', _ties, 200))


def test_lazy_argmins_equal_the_exact_dp(hc):
    rng = np.random.default_rng(2025)
    lengths = set()
    for name, gen, count in FAMILIES:
        n_dec = n_def = n_cols = 0
        for _ in range(count):
            x, y = gen(rng)
            n = len(x)
            lengths.add(n)
            assert 0 <= x[0] and x[-1] <= 255
            xs = np.ascontiguousarray(x, np.uint8)
            ya = np.ascontiguousarray(y, np.float64)
            for c in COSTS:
                a1 = np.zeros(64, np.uint8)
                a2 = np.zeros(64, np.uint8)
                d = ctypes.c_int(0)
                assert hc.ltx_dp_exact(n, xs.ctypes.data_as(u8p), ya.ctypes.data_as(f64p), c,
                                       a2.ctypes.data_as(u8p)) == 0
                amb = hc.ltx_dp_lazy(n, xs.ctypes.data_as(u8p), ya.ctypes.data_as(f64p), c,
                                     a1.ctypes.data_as(u8p), ctypes.byref(d))
                if d.value:
                    n_def += 1
                    continue
                n_dec += 1
                cols = [j for j in range(n) if not (amb >> j) & 1]
                n_cols += len(cols)
                assert [a1[j] for j in cols] == [a2[j] for j in cols], (name, c, list(x), list(y))
        print('%s: decided %d series (%d columns compared), deferred %d'
              % (name, n_dec, n_cols, n_def))
        # the comparison may not be hollow: at most a fifth of a family is deferred
        assert n_def <= DEFER_CAP * (n_dec + n_def), (name, n_dec, n_def)
    assert {1, 2, 3} <= lengths
