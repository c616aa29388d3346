"""The MMU sieve's test fixture: a plain numpy reference of lt_sieve_labels (a two-pass union-find
over the raster's neighbouring pixel pairs, independent of land_trendr_amd/csrc/lt_sieve.h), the
hand-made cases, and the host twin's loader (tests/native/build/liblt_sievecheck.so)."""
import ctypes
import functools
import os

import numpy as np

from land_trendr_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIEVECHECK = os.path.join(ROOT, 'tests', 'native', 'build', 'liblt_sievecheck.so')
LT_OK, LT_ERR_ARG, LT_ERR_LIMIT = 0, -1, -4
LT_MAX_TILE_PIX = 1 << 28
GUARD = -7          # int32 guard words round root / size / workspace
GUARD_U8 = 0xA5     # guard bytes round matched
SHAPES = ((1, 1), (1, 200), (200, 1), (67, 131), (130, 259))
BIG_ALL = (1024, 1500)


# ---- the reference ----

def _pairs(H, W, ok, key, conn):
    """Every pair (a, b), a > b, of neighbouring raster indices whose pixels are both matched with
    one key: west and north, with 8-connectivity also north-west and north-east. Built on the
    [H, W] view, so a row's end and the next row's start are never paired."""
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    ok2, key2 = ok.reshape(H, W), key.reshape(H, W)
    out = []
    offs = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if conn == 8 else [])
    for dy, dx in offs:  # pixel (y, x) with its neighbour (y - dy, x - dx)
        ys = slice(dy, H)
        yn = slice(0, H - dy)
        if dx >= 0:
            xs, xn = slice(dx, W), slice(0, W - dx)
        else:
            xs, xn = slice(0, W + dx), slice(-dx, W)
        both = ok2[ys, xs] & ok2[yn, xn] & (key2[ys, xs] == key2[yn, xn])
        out.append(np.stack([idx[ys, xs][both], idx[yn, xn][both]], 1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def reference(matched, key, shape, conn=8):
    """(root, size): int32 [P], by the contract of lt_sieve_labels. Pass one links the roots of
    every neighbouring pair (the larger root to the smallest root it meets) and flattens, until
    every pair agrees; pass two counts the pixels of each root."""
    H, W = shape
    P = H * W
    ok = np.asarray(matched).reshape(P) != 0
    k = np.zeros(P, np.int64) if key is None else np.asarray(key).reshape(P).astype(np.int64)
    pairs = _pairs(H, W, ok, k, conn)
    lab = np.arange(P, dtype=np.int64)
    while True:
        ra, rb = lab[pairs[:, 0]], lab[pairs[:, 1]]
        diff = ra != rb
        if not diff.any():
            break
        pairs, ra, rb = pairs[diff], ra[diff], rb[diff]
        np.minimum.at(lab, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:  # flatten: every label a root
            nxt = lab[lab]
            if (nxt == lab).all():
                break
            lab = nxt
    root = np.where(ok, lab, -1).astype(np.int32)
    count = np.bincount(lab[ok], minlength=max(P, 1))
    size = np.where(ok, count[lab] if P else 0, 0).astype(np.int32)
    return root, size


def applied(matched, size, min_pixels):
    """matched after the clear of the patches below min_pixels."""
    m = np.array(matched, np.uint8).reshape(-1)
    m[(size > 0) & (size < min_pixels)] = 0
    return m


def thresholds(size):
    """min_pixels in {1, s, s + 1} for a patch size s present in the case (the smallest above 1 if
    there is one, so that s clears something smaller wherever singletons exist)."""
    present = np.unique(size[size > 0])
    if len(present) == 0:
        return (1, 2, 3)
    big = present[present > 1]
    s = int(big[0] if len(big) else present[0])
    return (1, s, s + 1)


# ---- the hand-made cases ----

def spiral(H, W):
    """One 1-pixel-wide path that winds inwards from (0, 0), a free pixel between its arms."""
    m = np.zeros((H, W), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    turns = 0

    def inb(a, b):
        return 0 <= a < H and 0 <= b < W
    while turns < 2:
        ny, nx = y + dy, x + dx
        ahead = inb(ny + dy, nx + dx) and m[ny + dy, nx + dx]
        if inb(ny, nx) and not m[ny, nx] and not ahead:
            y, x = ny, nx
            m[y, x] = 1
            turns = 0
        else:
            dy, dx = dx, -dy
            turns += 1
    return m


def patterns(H, W):
    """(name, matched [H, W] uint8, key [H, W] int32) of every hand-made pattern."""
    yy, xx = np.mgrid[0:H, 0:W]
    one = np.full((H, W), 1987, np.int32)
    out = [('spiral', spiral(H, W), one)]
    comb = (xx % 2 == 0) | (yy == H - 1)
    out.append(('comb', comb.astype(np.uint8), one))
    out.append(('checkerboard', ((yy + xx) % 2 == 0).astype(np.uint8), one))
    # single diagonal contacts at every corner (8a, 8b): NW-SE where a + b is even, NE-SW else
    d = np.zeros((H, W), np.uint8)
    for a in range(1, (H - 1) // 8 + 1):
        for b in range(1, (W - 1) // 8 + 1):
            cy, cx = 8 * a, 8 * b
            if (a + b) % 2 == 0:
                d[cy - 1, cx - 1] = d[cy, cx] = 1
            else:
                d[cy - 1, cx] = d[cy, cx - 1] = 1
    out.append(('diagonals', d, one))
    edge = ((xx == 0) | (xx == W - 1)).astype(np.uint8)
    out.append(('edge-columns', edge, one))
    out.append(('stripes', np.ones((H, W), np.uint8), (1990 + xx % 2).astype(np.int32)))
    out.append(('all', np.ones((H, W), np.uint8), one))
    out.append(('none', np.zeros((H, W), np.uint8), one))
    for dens in (0.3, 0.45, 0.59, 0.9):
        for nk in (1, 3):
            rng = np.random.default_rng([int(dens * 100), nk, H, W])
            m = (rng.random((H, W)) < dens).astype(np.uint8) * rng.integers(1, 256, (H, W),
                                                                            dtype=np.uint8)
            k = (2000 + rng.integers(0, nk, (H, W))).astype(np.int32)
            out.append(('random-%.2f-%dkeys' % (dens, nk), m, k))
    return out


def cases():
    """(tag, (H, W), matched [P] uint8, key [P] int32) over every shape and pattern."""
    for H, W in SHAPES:
        for name, m, k in patterns(H, W):
            yield ('%s-%dx%d' % (name, H, W), (H, W), np.ascontiguousarray(m.reshape(-1)),
                   np.ascontiguousarray(k.reshape(-1)))


def random_scene(H, W, density, n_keys, seed):
    rng = np.random.default_rng(seed)
    m = (rng.random(H * W) < density).astype(np.uint8)
    k = (2000 + rng.integers(0, n_keys, H * W)).astype(np.int32)
    return m, k


@functools.lru_cache(maxsize=None)
def _case_table():
    return {tag: (shape, m, k) for tag, shape, m, k in cases()}


def case_tags():
    return list(_case_table())


def case(tag):
    return _case_table()[tag]


@functools.lru_cache(maxsize=None)
def case_reference(tag, conn, with_key):
    """The reference's (root, size) of a case, computed once and shared (read-only arrays)."""
    shape, m, k = case(tag)
    root, size = reference(m, k if with_key else None, shape, conn)
    root.setflags(write=False)
    size.setflags(write=False)
    return root, size


# ---- the host twin ----

def load_host():
    if not os.path.exists(SIEVECHECK):
        raise RuntimeError('%s not built: run __graft_entry__.build()' % SIEVECHECK)
    lib = ctypes.CDLL(SIEVECHECK)
    lib.ltx_sieve_labels.argtypes = [ctypes.POINTER(_abi.LtSieveIn),
                                     ctypes.POINTER(_abi.LtSieveOut), ctypes.c_int]
    lib.ltx_sieve_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64]
    lib.ltx_sieve_workspace_bytes.restype = ctypes.c_int64
    return lib


def structs(rows, cols, matched_ptr, key_ptr, conn, min_pixels, apply, root_ptr, size_ptr,
            work_ptr, work_bytes, phases=0):
    sin, sout = _abi.LtSieveIn(), _abi.LtSieveOut()
    sin.phases = phases
    sin.rows, sin.cols = rows, cols
    if matched_ptr:
        sin.matched = ctypes.cast(matched_ptr, _abi.c_u8p)
    if key_ptr:
        sin.key = ctypes.cast(key_ptr, _abi.c_i32p)
    sin.connectivity, sin.min_pixels, sin.apply = conn, min_pixels, int(apply)
    if root_ptr:
        sout.root = ctypes.cast(root_ptr, _abi.c_i32p)
    if size_ptr:
        sout.size = ctypes.cast(size_ptr, _abi.c_i32p)
    sout.workspace, sout.workspace_bytes = work_ptr or None, work_bytes
    return sin, sout


PAD = 5


def guarded(n, dtype, guard, fill=None):
    """A buffer of PAD guard elements, n payload elements and PAD guard elements."""
    b = np.full(n + 2 * PAD, guard, dtype)
    if fill is not None:
        b[PAD:PAD + n] = fill
    return b


def guards_intact(b, n, guard):
    return (b[:PAD] == guard).all() and (b[PAD + n:] == guard).all()


def run_host(lib, matched, key, shape, min_pixels=1, conn=8, apply=True, reverse=False):
    """The host twin on guarded buffers -> (root, size, matched afterwards); asserts LT_OK, the
    guards and that key is as it was."""
    H, W = shape
    P = H * W
    mb = guarded(P, np.uint8, GUARD_U8, matched)
    kb = None if key is None else guarded(P, np.int32, GUARD, key)
    rb, sb = guarded(P, np.int32, GUARD), guarded(P, np.int32, GUARD)
    nbytes = lib.ltx_sieve_workspace_bytes(H, W)
    assert nbytes == max(8 * P, 8)
    wb = guarded(nbytes // 4, np.int32, GUARD)

    def ptr(b):
        return b.ctypes.data + PAD * b.itemsize
    sin, sout = structs(H, W, ptr(mb), ptr(kb) if kb is not None else 0, conn, min_pixels, apply,
                        ptr(rb), ptr(sb), ptr(wb), nbytes)
    rc = lib.ltx_sieve_labels(ctypes.byref(sin), ctypes.byref(sout), int(reverse))
    assert rc == LT_OK, rc
    assert guards_intact(mb, P, GUARD_U8) and guards_intact(rb, P, GUARD)
    assert guards_intact(sb, P, GUARD) and guards_intact(wb, nbytes // 4, GUARD)
    if kb is not None:
        assert guards_intact(kb, P, GUARD) and (kb[PAD:PAD + P] == key).all()
    return rb[PAD:PAD + P].copy(), sb[PAD:PAD + P].copy(), mb[PAD:PAD + P].copy()


def make_twin_engine():
    """The CPU engine double (engine_double.OracleEngine) with a sieve over the host twin: host
    tensors in and out, the signature of Engine.sieve. For the job's CPU tests only (the product
    has no CPU path)."""
    import torch
    from engine_double import OracleEngine

    class SieveTwinEngine(OracleEngine):
        def sieve(self, matched, key, shape, min_pixels, connectivity=8, apply=True, out=None):
            P = shape[0] * shape[1]
            assert matched.dtype == torch.uint8 and matched.numel() == P
            assert P <= 1 or matched.stride(0) == 1
            r, s, mm = run_host(load_host(), matched.numpy(), None if key is None else
                                key.numpy(), shape, min_pixels, connectivity, apply)
            matched.copy_(torch.from_numpy(mm))
            if out is None:
                out = {'root': torch.empty(P, dtype=torch.int32),
                       'size': torch.empty(P, dtype=torch.int32)}
            out['root'].copy_(torch.from_numpy(r))
            out['size'].copy_(torch.from_numpy(s))
            return out
    return SieveTwinEngine()
