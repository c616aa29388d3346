"""The HIP grid sampling kernel (lt_grid_sample_dev, lt_sample.hip) through Engine.sample_grid,
GeoTiff.read_device and LocalJob(decode='device', sample='device'), against the host build of the
same core (liblt_io.so lt_grid_sample) and the numpy path of ingest_stack. Every comparison is
exact; the shapes are those of tests/samplefixture.py."""
import os

import numpy as np
import pytest

import samplefixture as sf
from land_trendr_amd import _abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from land_trendr_amd.engine import get_engine
    return get_engine(0)


def _dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)


def _dev_padded(eng, n_bytes):
    import torch
    return torch.full((n_bytes + 2 * sf.PAD,), sf.CANARY, dtype=torch.uint8, device=eng.device)


def _dev_bands(eng, src, gt, p0, p1, sel, extra=5, stream=None, device_offsets=False):
    """Engine.sample_grid over pixels p0..p1 with a row stride of n + extra, inside canaries."""
    import torch
    n = p1 - p0
    stride = n + extra
    xo, yo = sf.offsets(src, gt)
    if device_offsets:
        xo, yo = _dev(eng, xo), _dev(eng, yo)
    d_src = _dev(eng, src)
    ob = _dev_padded(eng, len(sel) * stride * src.itemsize)
    vb = _dev_padded(eng, n)
    out = ob[sf.PAD:ob.numel() - sf.PAD].view(d_src.dtype).view(len(sel), stride)[:, :n]
    eng.sample_grid([dict(src=d_src, xoff=xo, yoff=yo, p0=p0, n=n, sel=sel, out=out,
                          valid=vb[sf.PAD:sf.PAD + n], mode=_abi.LT_SAMPLE_BANDS)], stream=stream)
    torch.cuda.synchronize()
    hb, hv = ob.cpu().numpy(), vb.cpu().numpy()
    assert (hb[:sf.PAD] == sf.CANARY).all() and (hb[len(hb) - sf.PAD:] == sf.CANARY).all()
    planes = hb[sf.PAD:len(hb) - sf.PAD].view(src.dtype).reshape(len(sel), stride)
    assert (planes[:, n:].view(np.uint8) == sf.CANARY).all()
    assert (hv[:sf.PAD] == sf.CANARY).all() and (hv[sf.PAD + n:] == sf.CANARY).all()
    return planes[:, :n].copy(), hv[sf.PAD:sf.PAD + n].copy()


def _dev_mask(eng, valid, mask, mgt, p0, p1, stream=None):
    import torch
    n = p1 - p0
    xo, yo = sf.offsets(mask, mgt)
    vb = _dev_padded(eng, n)
    vb[sf.PAD:sf.PAD + n] = _dev(eng, valid)
    eng.sample_grid([dict(src=_dev(eng, mask), xoff=xo, yoff=yo, p0=p0, n=n,
                          valid=vb[sf.PAD:sf.PAD + n], mode=_abi.LT_SAMPLE_MASK)], stream=stream)
    torch.cuda.synchronize()
    hv = vb.cpu().numpy()
    assert (hv[:sf.PAD] == sf.CANARY).all() and (hv[sf.PAD + n:] == sf.CANARY).all()
    return hv[sf.PAD:sf.PAD + n].copy()


@pytest.mark.parametrize('dtype', sf.DTYPES)
@pytest.mark.parametrize('name', sorted(sf.SOURCES))
def test_bands_equal_the_host_build(eng, name, dtype):
    src, gt = sf.make_src(1, dtype, sf.SOURCES[name])
    for sel in sf.SELS:
        for k, (p0, p1) in enumerate(sf.RANGES):
            want, wv = sf.host_bands(src, gt, p0, p1, sel)
            got, gv = _dev_bands(eng, src, gt, p0, p1, sel, device_offsets=k % 2 == 1)
            assert sf.same(got, want), (sel, p0, p1)
            assert sf.same(gv, wv), (sel, p0, p1)
    want, wv = sf.numpy_bands(src, gt, 0, sf.P, [2, 4])  # and the numpy path itself
    got, gv = _dev_bands(eng, src, gt, 0, sf.P, [2, 4])
    assert sf.same(got, want) and sf.same(gv, wv)


@pytest.mark.parametrize('dtype', sf.INT_DTYPES)
def test_mask_equals_the_host_build(eng, dtype):
    src, gt = sf.make_src(2, 'int16', sf.SRC_A)
    mask, mgt = sf.make_src(5, dtype, sf.SRC_MASK, bands=2, zeros=0.4)
    for p0, p1 in sf.RANGES:
        _, valid = sf.numpy_bands(src, gt, p0, p1, [0])
        valid[np.random.default_rng(p0).random(len(valid)) < 0.2] = 0
        want = sf.host_mask(valid, mask, mgt, p0, p1)
        assert sf.same(want, sf.numpy_mask(valid, mask, mgt, p0, p1))
        assert sf.same(_dev_mask(eng, valid, mask, mgt, p0, p1), want), (p0, p1)


def test_more_than_one_block(eng):
    """300 x 300 grid points: 11250 groups, 44 blocks."""
    import torch
    from land_trendr_amd import ingest
    rng = np.random.default_rng(3)
    src = rng.integers(-30000, 30000, (2, 290, 310), dtype=np.int16)
    gt = sf.source_gt(4, -7)
    n = 300
    xv = sf.GT[0] + (np.arange(n) + 0.5) * sf.GT[1]
    yv = sf.GT[3] + (np.arange(n) + 0.5) * sf.GT[5]
    xo, yo = ingest.axis_offsets(gt, src.shape[1:], xv, yv)
    idx, ok = ingest.grid_offsets(gt, src.shape[1:], np.tile(xv, n), np.repeat(yv, n))
    want = np.take(src.reshape(2, -1), idx, axis=-1)
    want[:, ~ok] = 0
    out = torch.empty((2, n * n), dtype=torch.int16, device=eng.device)
    valid = torch.empty(n * n, dtype=torch.uint8, device=eng.device)
    eng.sample_grid([dict(src=_dev(eng, src), xoff=xo, yoff=yo, p0=0, n=n * n, sel=[0, 1],
                          out=out, valid=valid)])
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(valid.cpu().numpy(), ok.astype(np.uint8))


def test_two_jobs_in_one_call_on_a_side_stream(eng):
    """Bands then mask in one call on a side stream: the result of two calls."""
    import torch
    src, gt = sf.make_src(7, 'int16', sf.SRC_A)
    mask, mgt = sf.make_src(8, 'uint8', sf.SRC_MASK, bands=1, zeros=0.4)
    p0, p1 = 60, 191
    n = p1 - p0
    want, wv = sf.numpy_bands(src, gt, p0, p1, [1, 0])
    wv = sf.numpy_mask(wv, mask, mgt, p0, p1)
    xo, yo = sf.offsets(src, gt)
    mxo, myo = sf.offsets(mask, mgt)
    st = torch.cuda.Stream(device=eng.device)
    d_src, d_mask = _dev(eng, src), _dev(eng, mask)
    out = torch.empty((2, n), dtype=torch.int16, device=eng.device)
    valid = torch.empty(n, dtype=torch.uint8, device=eng.device)
    torch.cuda.synchronize()
    eng.sample_grid([dict(src=d_src, xoff=xo, yoff=yo, p0=p0, n=n, sel=[1, 0], out=out,
                          valid=valid),
                     dict(src=d_mask, xoff=mxo, yoff=myo, p0=p0, n=n, valid=valid,
                          mode=_abi.LT_SAMPLE_MASK)], stream=st)
    st.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), wv)
    two, tv = _dev_bands(eng, src, gt, p0, p1, [1, 0])
    tv = _dev_mask(eng, tv, mask, mgt, p0, p1)
    assert np.array_equal(two, want) and np.array_equal(tv, wv)


def test_rejected_arguments_write_nothing(eng):
    import torch
    from land_trendr_amd.engine import LtError
    src, gt = sf.make_src(9, 'int16', sf.SRC_A)
    xo, yo = sf.offsets(src, gt)
    d_src = _dev(eng, src)
    n = 64
    out = torch.full((2, n), 0x5A5A, dtype=torch.int16, device=eng.device)
    valid = torch.full((n,), sf.CANARY, dtype=torch.uint8, device=eng.device)
    good = dict(src=d_src, xoff=xo, yoff=yo, p0=10, n=n, sel=[1, 0], out=out, valid=valid)
    too_far = xo.copy()
    too_far[5] = src.shape[2]
    below = yo.copy()
    below[0] = -2
    bad = [dict(mode=2), dict(sel=[]), dict(sel=list(range(6)) * 3), dict(sel=[6, 0]),
           dict(sel=[0, -1]), dict(n=-1), dict(p0=-1), dict(p0=sf.P - 63), dict(n=sf.P + 1),
           dict(xoff=too_far), dict(yoff=below), dict(xoff=xo.astype(np.int64)),
           dict(src=d_src[:, :, ::2]), dict(src=d_src.cpu()), dict(out=out[:, :n - 1]),
           dict(out=out.view(torch.uint8)[:, :n].contiguous()), dict(out=out[:1]),
           dict(out=None), dict(valid=valid[:n - 1]), dict(valid=valid.view(torch.int8)),
           dict(mode=_abi.LT_SAMPLE_MASK, src=d_src.to(torch.float32))]
    for b in bad:
        with pytest.raises(LtError):
            eng.sample_grid([good, dict(good, **b)])
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A).all() and (valid.cpu().numpy() == sf.CANARY).all()
    eng.sample_grid([good])
    torch.cuda.synchronize()
    want, wv = sf.numpy_bands(src, gt, 10, 74, [1, 0])
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), wv)


def test_c_side_rejects_and_launches_nothing(eng):
    """lt_grid_sample_dev itself: LT_ERR_ARG for each bad field of the second job of a call, and
    the first (good) job not run either."""
    import ctypes
    import torch
    src, gt = sf.make_src(9, 'int16', sf.SRC_A)
    xo, yo = sf.offsets(src, gt)
    d_src, d_xo, d_yo = _dev(eng, src), _dev(eng, xo), _dev(eng, yo)
    n = 64
    out = torch.full((2, n), 0x5A5A, dtype=torch.int16, device=eng.device)
    valid = torch.full((n,), sf.CANARY, dtype=torch.uint8, device=eng.device)

    def job(**kw):
        a = _abi.LtSampleJob()
        a.src, a.bps, a.src_bands, a.src_h, a.src_w = d_src.data_ptr(), 2, 6, 29, 61
        a.xoff, a.yoff, a.grid_w, a.grid_h = d_xo.data_ptr(), d_yo.data_ptr(), sf.W, sf.H
        a.p0, a.n, a.n_sel = 10, n, 2
        a.sel[0], a.sel[1] = 1, 0
        a.out, a.out_stride, a.valid, a.mode = out.data_ptr(), n, valid.data_ptr(), 0
        for k, v in kw.items():
            if k == 'sel0':
                a.sel[0] = v
            else:
                setattr(a, k, v)
        return a

    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    bad = [dict(bps=3), dict(bps=0), dict(mode=2), dict(mode=-1), dict(n_sel=0), dict(n_sel=17),
           dict(sel0=6), dict(sel0=-1), dict(src_h=-1), dict(src_w=-1), dict(grid_w=-1),
           dict(grid_h=-1), dict(p0=-1), dict(n=-1), dict(out_stride=n - 1), dict(p0=sf.P - 63),
           dict(src_h=1 << 31), dict(src=d_src.data_ptr() + 1), dict(out=out.data_ptr() + 1),
           dict(src=None), dict(out=None), dict(valid=None), dict(xoff=None), dict(yoff=None)]
    for b in bad:
        arr = (_abi.LtSampleJob * 2)(job(), job(**b))
        rc = eng.lib.lt_grid_sample_dev(eng.ctx, arr, 2, st)
        assert rc == -1, b  # LT_ERR_ARG
        assert b'sample job' in eng.lib.lt_last_error(eng.ctx)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A5A).all() and (valid.cpu().numpy() == sf.CANARY).all()


def test_read_device_then_sample_equals_read_then_numpy(eng, tmp_path):
    """An LZW predictor-2 strip file with an extent of its own, decoded and sampled on the
    device."""
    import torch
    from land_trendr_amd.geotiff import GeoTiff
    from land_trendr_amd.raster import write_geotiff
    src, gt = sf.make_src(11, 'int16', sf.SRC_A, bands=3)
    p = str(tmp_path / 'r.tif')
    write_geotiff(p, src, geotransform=gt, nodata=None, predictor=2)
    g = GeoTiff(p)
    assert g.compression == 5 and g.predictor == 2 and 273 in g.tags and g.device_eligible()
    assert g.geotransform() == gt
    host = g.read()
    want, wv = sf.numpy_bands(host, g.geotransform(), 0, sf.P, [2, 0])
    d, err = g.read_device(eng)
    xo, yo = sf.offsets(host, g.geotransform())
    out = torch.empty((2, sf.P), dtype=torch.int16, device=eng.device)
    valid = torch.empty(sf.P, dtype=torch.uint8, device=eng.device)
    eng.sample_grid([dict(src=d, xoff=xo, yoff=yo, p0=0, n=sf.P, sel=[2, 0], out=out,
                          valid=valid)])
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), wv)


# ---- the job ------------------------------------------------------------------------------------

def _extend_job(root, sc_names):
    """Onto jobfixture.make_job's directory (9 x 13 pixels, 2 bands): raster 5 rewritten larger
    than the template, raster 7 smaller, raster 8 with four bands (the equation reads two); masks
    with an extent of their own for rasters 5 and 7; raster 6's mask rewritten with Deflate.
    Returns the number of Deflate masks."""
    import jobfixture
    from land_trendr_amd.geotiff import GeoTiff
    from land_trendr_amd.raster import write_geotiff
    rdir = os.path.join(root, 'synth', 'input', 'rasters')
    GT = jobfixture.GT
    rng = np.random.default_rng(17)

    def gt_of(dy, dx):
        return (GT[0] - dx * GT[1], GT[1], 0.0, GT[3] - dy * GT[5], 0.0, GT[5])

    def rewrite(name, rows, cols, dy, dx, bands):
        fn = os.path.join(rdir, name)
        old = GeoTiff(fn).read()
        a = rng.integers(-2000, 2000, (bands, rows, cols)).astype(old.dtype)
        # the old samples where the new extent covers them: pixel (y, x) is grid point (y - dy, x - dx)
        for y in range(rows):
            for x in range(cols):
                if 0 <= y - dy < old.shape[1] and 0 <= x - dx < old.shape[2]:
                    a[:2, y, x] = old[:, y - dy, x - dx]
        write_geotiff(fn, a, geotransform=gt_of(dy, dx), nodata=None)
        return fn

    plain = [n for n in sc_names if n.endswith('.tif')]
    assert len(plain) >= 6
    big, small, four, defl = plain[1], plain[2], plain[3], plain[4]
    rewrite(big, 14, 19, 2, 3, 2)      # larger than the template, the template inside it
    rewrite(small, 6, 8, -2, -3, 2)    # smaller: grid points off it on every side
    rewrite(four, 9, 13, 0, 0, 4)      # co-registered, two spare bands
    for name, (rows, cols, dy, dx) in ((big, (11, 10, 1, -2)), (small, (12, 16, 0, 1))):
        m = (rng.random((rows, cols)) < 0.7).astype(np.uint8)
        write_geotiff(os.path.join(rdir, name.replace('ledaps', 'cloudmask')), m,
                      geotransform=gt_of(dy, dx), nodata=None)
    m = (rng.random((9, 13)) < 0.7).astype(np.uint8)
    write_geotiff(os.path.join(rdir, defl.replace('ledaps', 'cloudmask')), m, geotransform=GT,
                  nodata=None, compress='deflate')
    return 1


def _make(tmp_path, mode):
    from jobfixture import make_job
    root = str(tmp_path / mode)
    _, names = make_job(root)
    return root, _extend_job(root, names)


def test_job_device_sample_equals_host(tmp_path):
    from land_trendr_amd.job import LocalJob
    jobs, files = {}, {}
    for mode in ('host', 'device'):
        root, n_deflate = _make(tmp_path, mode)
        kw = {} if mode == 'host' else {'decode': 'device', 'sample': 'device'}
        j = jobs[mode] = LocalJob(root, 'synth', device=0, tile_pixels=50, on_error='skip', **kw)
        files[mode] = j.run()
    h, d = jobs['host'], jobs['device']
    assert h.sample == 'host' and h.sample_stats['rasters'] == 0
    assert h.decode_stats['device'] == 0
    K = len(d.rast_fns)
    # every raster is a strip-organised LZW file: all of them decode on the device
    assert d.decode_stats == {'device': K, 'host': 0}
    assert d.sample_stats['rasters'] >= 1
    assert d.sample_stats['masks_host'] == n_deflate
    n_masks = sum(1 for m in d.mask_fns if m)
    assert d.sample_stats['masks_device'] == n_masks - n_deflate and n_masks > n_deflate
    assert sorted(h.planes) == sorted(d.planes)
    for k in h.planes:
        assert h.planes[k].dtype == d.planes[k].dtype, k
        assert np.asarray(h.planes[k]).tobytes() == np.asarray(d.planes[k]).tobytes(), k
    assert sorted(files['host']) == sorted(files['device'])
    for k, paths in files['host'].items():
        for ph, pd in zip(paths, files['device'][k]):
            assert os.path.basename(ph) == os.path.basename(pd)
            assert open(ph, 'rb').read() == open(pd, 'rb').read(), k
    hb, db = h.stack['bands'], d.stack['bands']
    assert hb.dtype == db.dtype and hb.tobytes() == db.tobytes()
    hv, dv = h.stack['valid'], d.stack['valid']
    assert hv.dtype == dv.dtype and hv.tobytes() == dv.tobytes()
    # the fixture does what it is for: off-raster points, masked points, and valid ones
    assert 0 < int(hv.sum()) < hv.size and (hv == 0).any(axis=1).sum() >= 4


def test_multi_rank_shape_without_a_process_group(tmp_path, monkeypatch):
    """The pixel ranges of a two-rank job (round-robin tiles, three or more per rank), each rank
    parsed in this process."""
    from land_trendr_amd.job import LocalJob
    for rank in (1, 0):
        stacks = {}
        for mode in ('host', 'device'):
            root, _ = _make(tmp_path / ('r%d' % rank), mode)
            kw = {} if mode == 'host' else {'decode': 'device', 'sample': 'device'}
            j = LocalJob(root, 'synth', device=0, tile_pixels=17, on_error='skip', **kw)
            j.setup()
            monkeypatch.setattr(LocalJob, '_dist', staticmethod(lambda: (None, 2, rank)))
            j.parse()
            monkeypatch.undo()
            assert len(j.mosaic.mine) >= 3
            stacks[mode] = (j.stack, j.decode_stats, j.sample_stats)
        (hs, hd, _), (ds, dd, dsm) = stacks['host'], stacks['device']
        assert hd['device'] == 0 and dd['device'] > 0 and dsm['rasters'] == dd['device']
        assert hs['ranges'] == ds['ranges'] and len(hs['ranges']) >= 3
        assert hs['bands'].dtype == ds['bands'].dtype and hs['valid'].dtype == ds['valid'].dtype
        assert hs['bands'].tobytes() == ds['bands'].tobytes()
        assert hs['valid'].tobytes() == ds['valid'].tobytes()
        assert hs['dates'] == ds['dates']


def test_sample_device_needs_decode_device(tmp_path):
    from land_trendr_amd.job import LocalJob
    with pytest.raises(ValueError):
        LocalJob(str(tmp_path), 'synth', decode='host', sample='device')
    with pytest.raises(ValueError):
        LocalJob(str(tmp_path), 'synth', sample='device')
    with pytest.raises(ValueError):
        LocalJob(str(tmp_path), 'synth', decode='device', sample='gpu')


def test_cpu_engine_double_falls_back_to_the_host_path(tmp_path):
    """sample='device' on a job whose engine is the CPU double: no device stack, the host path."""
    from engine_double import OracleEngine
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    stacks = {}
    for mode in ('host', 'device'):
        root = str(tmp_path / mode)
        make_job(root)
        kw = {} if mode == 'host' else {'decode': 'device', 'sample': 'device'}
        j = LocalJob(root, 'synth', tile_pixels=50, on_error='skip', engine=OracleEngine(), **kw)
        j.setup()
        stacks[mode] = j.parse()
        assert j.decode_stats['device'] == 0 and j.sample_stats['rasters'] == 0
        assert j.sample_stats['masks_device'] == 0
        assert j.sample_stats['masks_host'] == sum(1 for m in j.mask_fns if m)
    assert np.array_equal(stacks['host']['bands'], stacks['device']['bands'])
    assert np.array_equal(stacks['host']['valid'], stacks['device']['valid'])
