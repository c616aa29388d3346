"""The MMU sieve on the MI355X (lt_sieve_labels, lt_sieve.hip): every hand-made case of
sievefixture through Engine.sieve into guarded device buffers against the pixel-pair reference,
two larger scenes against the host twin, the argument checks through ctypes, and LocalJob with
settings.json mmu. Equality everywhere; a second launch agrees in every element."""
import ctypes

import numpy as np
import pytest
import torch

import sievefixture as sx
from land_trendr_amd import _abi
from land_trendr_amd.engine import LtError, get_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    return get_engine(0)


@pytest.fixture(scope='module')
def lib():
    return sx.load_host()


def run_dev(eng, matched, key, shape, min_pixels=1, conn=8, apply=True):
    """Engine.sieve on guarded device buffers -> (root, size, matched afterwards) on the host;
    checks the guards and that key is as it was."""
    P = shape[0] * shape[1]
    mb = torch.from_numpy(sx.guarded(P, np.uint8, sx.GUARD_U8, matched)).to(eng.device)
    kb = None if key is None else torch.from_numpy(sx.guarded(P, np.int32, sx.GUARD, key)).to(
        eng.device)
    rb = torch.from_numpy(sx.guarded(P, np.int32, sx.GUARD)).to(eng.device)
    sb = torch.from_numpy(sx.guarded(P, np.int32, sx.GUARD)).to(eng.device)
    cut = slice(sx.PAD, sx.PAD + P)
    out = eng.sieve(mb[cut], None if kb is None else kb[cut], shape, min_pixels, conn, apply,
                    out={'root': rb[cut], 'size': sb[cut]})
    assert out['root'].data_ptr() == rb[cut].data_ptr()
    torch.cuda.synchronize()
    mb, rb, sb = mb.cpu().numpy(), rb.cpu().numpy(), sb.cpu().numpy()
    assert sx.guards_intact(mb, P, sx.GUARD_U8) and sx.guards_intact(rb, P, sx.GUARD)
    assert sx.guards_intact(sb, P, sx.GUARD)
    if kb is not None:
        kb = kb.cpu().numpy()
        assert sx.guards_intact(kb, P, sx.GUARD) and (kb[cut] == key).all()
    return rb[cut], sb[cut], mb[cut]


@pytest.mark.parametrize('shape', sx.SHAPES, ids=lambda s: '%dx%d' % s)
def test_handmade_cases_equal_the_reference(eng, shape):
    for tag in sx.case_tags():
        if not tag.endswith('-%dx%d' % shape):
            continue
        _, m, k = sx.case(tag)
        for conn in (4, 8):
            for with_key in (True, False):
                root, size = sx.case_reference(tag, conn, with_key)
                key = k if with_key else None
                t1, ts, ts1 = sx.thresholds(size)
                first = None
                for min_pixels in (ts, ts1, ts1, t1):
                    r, s, mm = run_dev(eng, m, key, shape, min_pixels, conn)
                    what = (tag, conn, with_key, min_pixels)
                    assert (r == root).all(), what
                    assert (s == size).all(), what
                    assert (mm == sx.applied(m, size, min_pixels)).all(), what
                    if min_pixels == ts1:  # a second launch is bit-equal
                        if first is None:
                            first = (r, s, mm)
                        else:
                            assert all((a == b).all() for a, b in zip(first, (r, s, mm))), what
                r, s, mm = run_dev(eng, m, key, shape, ts1, conn, apply=False)
                assert (r == root).all() and (s == size).all() and (mm == m).all(), what


def test_larger_scenes_equal_the_host_twin(eng, lib):
    H = W = 2048
    m, k = sx.random_scene(H, W, 0.45, 3, seed=17)
    root, size, want = sx.run_host(lib, m, k, (H, W), 4, 8)
    # (0.15 of the pixels per key: below the percolation threshold, many small patches)
    assert size.max() >= 20 and (size == 1).sum() > 1000 and (want != m).any()
    for _ in range(2):
        r, s, mm = run_dev(eng, m, k, (H, W), 4, 8)
        assert (r == root).all() and (s == size).all() and (mm == want).all()
    H, W = sx.BIG_ALL
    m = np.ones(H * W, np.uint8)
    k = np.full(H * W, 1999, np.int32)
    for conn in (4, 8):
        r, s, mm = run_dev(eng, m, k, (H, W), H * W, conn)
        assert (r == 0).all() and (s == H * W).all() and (mm == 1).all()
    r, s, mm = run_dev(eng, m, None, (H, W), H * W + 1, 8)
    assert (r == 0).all() and (s == H * W).all() and (mm == 0).all()


def test_engine_refuses_wrong_tensors(eng):
    m = torch.ones(12, dtype=torch.uint8, device=eng.device)
    k = torch.zeros(12, dtype=torch.int32, device=eng.device)
    ok = eng.sieve(m, k, (3, 4), 2)
    assert sorted(ok) == ['root', 'size'] and ok['size'].dtype == torch.int32
    for bad in (dict(matched=m.cpu()), dict(matched=m.to(torch.int8)), dict(key=k.cpu()),
                dict(key=k.to(torch.int64)), dict(shape=(3, 5)), dict(shape=(12,)),
                dict(matched=torch.ones(24, dtype=torch.uint8, device=eng.device)[::2]),
                dict(min_pixels=0), dict(min_pixels=True), dict(min_pixels=2.0),
                dict(connectivity=6), dict(out={'root': ok['root']}),
                dict(out={'root': ok['root'], 'size': ok['size'].to(torch.int64)}),
                dict(out={'root': ok['root'][:11], 'size': ok['size']})):
        kw = dict(dict(matched=m, key=k, shape=(3, 4), min_pixels=2), **bad)
        with pytest.raises(LtError):
            eng.sieve(**kw)
    none = eng.sieve(m[:0], None, (0, 7), 1)
    assert none['root'].numel() == 0 and none['size'].numel() == 0


def test_abi_errors_launch_nothing(eng):
    """The error cases through ctypes with 1-element tensors: nothing is launched."""
    A, L = sx.LT_ERR_ARG, sx.LT_ERR_LIMIT
    m = torch.full((1,), 9, dtype=torch.uint8, device=eng.device)
    t = {f: torch.full((2,), sx.GUARD, dtype=torch.int32, device=eng.device) for f in 'krsw'}
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)

    def call(rows=1, cols=1, conn=8, min_pixels=1, work_bytes=8, drop=(), null=None):
        p = {f: (0 if f in drop else v.data_ptr()) for f, v in dict(t, m=m).items()}
        sin, sout = sx.structs(rows, cols, p['m'], p['k'], conn, min_pixels, True, p['r'], p['s'],
                               p['w'], work_bytes)
        return eng.lib.lt_sieve_labels(eng.ctx, None if null == 'in' else ctypes.byref(sin),
                                       None if null == 'out' else ctypes.byref(sout), st)
    assert call(null='in') == A and call(null='out') == A
    for f in 'mrsw':
        assert call(drop=(f,)) == A, f
    assert call(rows=-1) == A and call(cols=-1) == A
    for conn in (0, 6, 16):
        assert call(conn=conn) == A
    assert call(min_pixels=0) == A and call(work_bytes=7) == A
    assert call(rows=(1 << 28) + 1) == L and call(rows=1 << 40, cols=1 << 40) == L
    assert b'lt_sieve_labels' in eng.lib.lt_last_error(eng.ctx)
    assert call(rows=0, drop=tuple('mkrsw'), work_bytes=0) == sx.LT_OK
    torch.cuda.synchronize()
    assert int(m[0]) == 9 and all((v == sx.GUARD).all() for v in t.values())
    assert eng.lib.lt_sieve_workspace_bytes(3, 5) == 120


# ---- LocalJob ----

def run_job(root, job, settings, **kw):
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    make_job(root, job, rows=24, cols=40, seed=5, settings=settings)
    j = LocalJob(root, job, device=0, on_error='skip', raster_mode='typed', trendline=False, **kw)
    return j, j.run()


def read(files, key):
    from land_trendr_amd.geotiff import GeoTiff
    return GeoTiff(files[key][0]).read()[0]


def test_job_sieves_the_label_rasters(eng, tmp_path):
    from jobfixture import SETTINGS
    from land_trendr_amd.raster import LABEL_KEYS
    root = str(tmp_path)
    plain, files0 = run_job(root, 'plain', SETTINGS)
    assert plain.mmu_stats is None
    j, files = run_job(root, 'mmu', dict(SETTINGS, mmu={'min_pixels': 4}))
    assert sorted(files) == sorted(files0)
    nd = _abi.LT_NODATA
    for rule in j.rules:
        onset = read(files0, rule.name + '_onset_year')
        m = (onset != nd).astype(np.uint8).reshape(-1)
        _, size = sx.reference(m, onset.reshape(-1).astype(np.int32), onset.shape, 8)
        gone = ((size > 0) & (size < 4)).reshape(onset.shape)
        # the fixture provides both: a condition of the test
        assert gone.any() and (size >= 4).any(), rule.name
        # every label raster the job writes for the rule (raster.LABEL_KEYS: class_val,
        # onset_year, magnitude, duration)
        keys = sorted(k for k in files0 if k.startswith(rule.name + '_'))
        assert keys == sorted('%s_%s' % (rule.name, key) for key in LABEL_KEYS) and len(keys) >= 4
        for key in keys:
            a0, a = read(files0, key), read(files, key)
            want = np.where(gone, np.asarray(nd, a0.dtype), a0)
            assert a.dtype == a0.dtype and (a == want).all(), (rule.name, key)
        assert j.mmu_stats[rule.name] == {'matched': int(m.sum()), 'removed': int(gone.sum())}
    assert sorted(j.mmu_stats) == sorted(r.name for r in j.rules)
    # the device encoder writes the same files, byte for byte
    j2, files2 = run_job(root, 'mmu-dev', dict(SETTINGS, mmu={'min_pixels': 4}), encode='device')
    assert j2.mmu_stats == j.mmu_stats and sorted(files2) == sorted(files)
    for k in files:
        with open(files[k][0], 'rb') as fa, open(files2[k][0], 'rb') as fb:
            assert fa.read() == fb.read(), k
    # by 'match' with 4-connectivity: the sizes of the matched mask alone
    j3, files3 = run_job(root, 'mmu-match', dict(
        SETTINGS, mmu={'min_pixels': 3, 'connectivity': 4, 'by': 'match'}))
    for rule in j3.rules:
        onset = read(files0, rule.name + '_onset_year')
        m = (onset != nd).astype(np.uint8).reshape(-1)
        _, size = sx.reference(m, None, onset.shape, 4)
        gone = ((size > 0) & (size < 3)).reshape(onset.shape)
        a = read(files3, rule.name + '_onset_year')
        assert (a == np.where(gone, nd, onset)).all(), rule.name
