"""The MMU sieve on the CPU: the kernels' phase steps compiled as a serial host twin
(tests/native/sieve_host_check.hip over land_trendr_amd/csrc/lt_sieve.h) against the pixel-pair
reference of sievefixture on every hand-made case, both connectivities, with and without a key,
blocks forwards and backwards; the argument checks; the export. Equality everywhere."""
import ctypes
import os

import numpy as np
import pytest

import sievefixture as sx
from land_trendr_amd import _abi


@pytest.fixture(scope='module')
def lib():
    return sx.load_host()


def test_the_cases_hold_what_they_are_named_for():
    tags = sx.case_tags()
    assert len(tags) == 16 * len(sx.SHAPES)
    t = '130x259'
    P = 130 * 259
    root, size = sx.case_reference('spiral-' + t, 8, True)
    m = sx.case('spiral-' + t)[1]
    assert m.sum() > P // 3 and (size[m != 0] == m.sum()).all()      # one long path
    assert (sx.case_reference('spiral-' + t, 4, True)[1] == size).all()
    root = sx.case_reference('comb-' + t, 8, True)[0]
    assert (root[root >= 0] == 0).all() and (root >= 0).sum() > P // 2   # all teeth joined
    r8, s8 = sx.case_reference('checkerboard-' + t, 8, True)
    r4, s4 = sx.case_reference('checkerboard-' + t, 4, True)
    assert s8.max() == (P + 1) // 2 and s4.max() == 1
    _, s8 = sx.case_reference('diagonals-' + t, 8, True)
    _, s4 = sx.case_reference('diagonals-' + t, 4, True)
    assert s8.max() == 2 and s4.max() == 1 and (s8 > 0).sum() == 2 * 16 * 32
    _, s = sx.case_reference('edge-columns-' + t, 8, True)
    assert s.max() == 130                                            # the row wrap joins nothing
    _, s = sx.case_reference('stripes-' + t, 8, True)
    assert (s == 130).all()                                          # a patch per column
    _, s = sx.case_reference('stripes-' + t, 8, False)
    assert (s == P).all()                                            # one patch by match
    root, s = sx.case_reference('all-' + t, 4, True)
    assert (s == P).all() and (root == 0).all()
    root, s = sx.case_reference('none-' + t, 8, True)
    assert (s == 0).all() and (root == -1).all()
    _, s = sx.case_reference('random-0.59-1keys-' + t, 8, True)
    assert s.max() > P // 4                                          # a giant tortuous patch


@pytest.mark.parametrize('tag', sx.case_tags())
def test_host_twin_equals_the_reference(lib, tag):
    shape, m, k = sx.case(tag)
    for conn in (4, 8):
        for with_key in (True, False):
            root, size = sx.case_reference(tag, conn, with_key)
            key = k if with_key else None
            t1, ts, ts1 = sx.thresholds(size)
            runs = [(t1, False), (ts, True), (ts1, False), (ts1, True)]
            for min_pixels, reverse in runs:
                r, s, mm = sx.run_host(lib, m, key, shape, min_pixels, conn, True, reverse)
                what = (tag, conn, with_key, min_pixels, reverse)
                assert (r == root).all(), what
                assert (s == size).all(), what
                assert (mm == sx.applied(m, size, min_pixels)).all(), what
            assert (sx.applied(m, size, t1) == m).all()              # min_pixels 1 clears nothing
            if size.max() > 0:                                       # ts keeps size ts, ts + 1 not
                keep = sx.applied(m, size, ts)[size == ts]
                assert (keep != 0).all() and (sx.applied(m, size, ts1)[size == ts] == 0).all()
            r, s, mm = sx.run_host(lib, m, key, shape, ts1, conn, apply=False)
            assert (r == root).all() and (s == size).all() and (mm == m).all()


def test_all_matched_at_1024_by_1500(lib):
    H, W = sx.BIG_ALL
    m = np.ones(H * W, np.uint8)
    k = np.full(H * W, 1999, np.int32)
    root, size = sx.reference(m, k, (H, W), 8)
    assert (root == 0).all() and (size == H * W).all()
    for reverse in (False, True):
        r, s, mm = sx.run_host(lib, m, k, (H, W), H * W, 8, True, reverse)
        assert (r == root).all() and (s == size).all() and (mm == m).all()
    r, s, mm = sx.run_host(lib, m, None, (H, W), H * W + 1, 4)
    assert (r == root).all() and (s == size).all() and (mm == 0).all()


def test_reference_against_scipy_label():
    ndimage = pytest.importorskip('scipy.ndimage')
    structure = {4: [[0, 1, 0], [1, 1, 1], [0, 1, 0]], 8: np.ones((3, 3), int)}
    for tag in sx.case_tags():
        if not tag.startswith('random'):
            continue
        shape, m, k = sx.case(tag)
        for conn in (4, 8):
            root, size = sx.case_reference(tag, conn, True)
            for key in np.unique(k):
                sel = (m != 0) & (k == key)
                lab, n = ndimage.label(sel.reshape(shape), structure=structure[conn])
                roots = np.unique(root[sel])
                assert n == len(roots), (tag, conn, key)
                want = np.sort(np.bincount(lab.reshape(-1))[1:])
                assert (np.sort(size[roots]) == want).all(), (tag, conn, key)


def test_argument_checks_launch_nothing(lib):
    A, L = sx.LT_ERR_ARG, sx.LT_ERR_LIMIT
    H, W = 7, 9
    P = H * W
    bufs = {'m': sx.guarded(P, np.uint8, sx.GUARD_U8, 1), 'k': sx.guarded(P, np.int32, sx.GUARD, 3),
            'r': sx.guarded(P, np.int32, sx.GUARD), 's': sx.guarded(P, np.int32, sx.GUARD),
            'w': sx.guarded(2 * P, np.int32, sx.GUARD)}
    before = {f: b.copy() for f, b in bufs.items()}
    ptr = {f: b.ctypes.data + sx.PAD * b.itemsize for f, b in bufs.items()}

    def call(rows=H, cols=W, conn=8, min_pixels=1, work_bytes=8 * P, drop=(), null=None,
             phases=0):
        p = {f: (0 if f in drop else v) for f, v in ptr.items()}
        sin, sout = sx.structs(rows, cols, p['m'], p['k'], conn, min_pixels, True, p['r'], p['s'],
                               p['w'], work_bytes, phases)
        rc = lib.ltx_sieve_labels(None if null == 'in' else ctypes.byref(sin),
                                  None if null == 'out' else ctypes.byref(sout), 0)
        if rc != sx.LT_OK or rows * cols == 0:
            for f, b in bufs.items():
                assert (b == before[f]).all(), f
        return rc
    assert call(null='in') == A and call(null='out') == A
    for f in 'mrsw':
        assert call(drop=(f,)) == A, f
    assert call(rows=-1) == A and call(cols=-1) == A
    for conn in (0, 1, 6, 16, -8):
        assert call(conn=conn) == A, conn
    assert call(min_pixels=0) == A and call(min_pixels=-5) == A
    assert call(work_bytes=8 * P - 1) == A and call(work_bytes=0) == A
    assert call(phases=16) == A and call(phases=-1) == A
    assert call(rows=1 << 14, cols=(1 << 14) + 1) == L
    assert call(rows=(1 << 28) + 1, cols=1) == L
    assert call(rows=1 << 40, cols=1 << 40) == L                     # no overflow in the product
    # nothing to do: LT_OK at once, whatever else is passed
    assert call(rows=0) == sx.LT_OK and call(cols=0, drop=tuple('mkrsw')) == sx.LT_OK
    assert call(rows=0, cols=1 << 40, conn=5, min_pixels=0, work_bytes=0) == sx.LT_OK
    assert call(drop=('k',)) == sx.LT_OK                             # a key is optional
    assert lib.ltx_sieve_workspace_bytes(H, W) == 8 * P
    assert lib.ltx_sieve_workspace_bytes(0, 5) == 8
    assert lib.ltx_sieve_workspace_bytes(-1, 5) == -1
    assert lib.ltx_sieve_workspace_bytes(1 << 14, 1 << 14) == 8 << 28
    assert lib.ltx_sieve_workspace_bytes(1 << 14, (1 << 14) + 1) == -1


def test_the_export_is_declared_and_the_abi_version_stays():
    assert 'lt_sieve_labels' in _abi.EXPORTS and 'lt_sieve_workspace_bytes' in _abi.EXPORTS
    assert _abi.LT_ABI_VERSION == 8
    lib = _abi.load_lib()
    assert lib.lt_abi_version() == 8
    assert hasattr(lib, 'lt_sieve_labels') and hasattr(lib, 'lt_sieve_workspace_bytes')
    assert lib.lt_sieve_workspace_bytes(3, 5) == 120                 # host only: no GPU needed
    hdr = open(os.path.join(sx.ROOT, 'include', 'lt_abi.h')).read()
    assert 'int lt_sieve_labels(' in hdr and '} lt_sieve_in;' in hdr and '} lt_sieve_out;' in hdr
    assert ctypes.sizeof(_abi.LtSieveIn) == 48 and ctypes.sizeof(_abi.LtSieveOut) == 32
