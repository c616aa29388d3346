"""settings.json mask_eqn on the GPU: the hiprtc-compiled mask kernels (Engine.apply_mask) against
numpy's own evaluation of the expression text, analysis_reducer_batch with the key against the
same call fed the numpy mask and against the CPU oracle, and LocalJob against the equivalent
`_cloudmask` job. Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import maskfixture as mf
from land_trendr_amd.index_eqn import MaskProgram

pytestmark = pytest.mark.gpu
NUMBERS = [1, 2, 3, 4]
SIZES = (1, 3, 4, 5, 63, 64, 65, 257, 1027)
OFFSETS = (0, 1, 2, 7)
CANARY = 0xA5


@pytest.fixture(scope='module')
def engine():
    from land_trendr_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope='module')
def stacks():
    """Per band type: a [3, 4, 1040] stack with the type's extremes in every plane (host array and
    device tensor), made once and never written."""
    out = {}
    for dt in mf.DTYPES:
        host = mf.band_values(dt, (3, 4, 1040), seed=11)
        out[np.dtype(dt)] = (host, torch.from_numpy(host).cuda())
    return out


def _valid_in(K, P, stride, seed):
    """A [K, stride] validity buffer whose [K][P] part holds zeros and several non-zero values,
    the rest a canary; with a canary row before and after."""
    rng = np.random.default_rng(seed)
    buf = np.full((K + 2, stride), CANARY, np.uint8)
    buf[1:K + 1, :P] = rng.choice(np.array([0, 1, 1, 1, 255, 7], np.uint8), (K, P))
    return buf


def _check(engine, fn, eqn, host, dev, K, P, off, stride_pad, counter=None):
    """One apply_mask on the view [:K, :, off:off+P] of the stack; returns the exact count."""
    b_host, b_dev = host[:K, :, off:off + P], dev[:K, :, off:off + P]
    stride = P + stride_pad
    buf = _valid_in(K, P, stride, seed=K * 4096 + P * 8 + off)
    # the validity view starts at the same pixel offset as the band view (as the job's slices do)
    dbuf = torch.from_numpy(np.pad(buf.ravel(), (off, 64))).cuda()
    view = dbuf[off:off + buf.size].view(K + 2, stride)[1:K + 1, :P]
    engine.apply_mask(fn, b_dev, view, dropped=counter)
    keep = mf.numpy_mask(eqn, np.moveaxis(b_host, 1, 0))
    want = buf.copy()
    want[1:K + 1, :P] = np.where(keep, buf[1:K + 1, :P], 0)
    got = dbuf.cpu().numpy()
    assert np.array_equal(got[off:off + buf.size].reshape(K + 2, stride), want), (eqn, K, P, off)
    assert not got[:off].any() and not got[off + buf.size:].any()  # the padding stays zero
    return int(np.count_nonzero((buf[1:K + 1, :P] != 0) & ~keep))


@pytest.mark.parametrize('dt', mf.DTYPES)
def test_apply_mask_vs_numpy(engine, stacks, dt):
    """Every size (tail only, exact vector multiples, vector + tail, several blocks) at every
    start offset (head / vector / tail alignment) for K = 1 and 3, with validity zeros already
    present and canaries around [K][P]; `dropped` is exact per call."""
    host, dev = stacks[np.dtype(dt)]
    eqns = [e for e, dts in mf.CORPUS if dt in dts]
    fns = {e: engine.compile_mask(MaskProgram(e, dt, NUMBERS)) for e in eqns}
    counter = torch.zeros(1, dtype=torch.int64, device=engine.device)
    total = 0
    n = 0
    for K in (1, 3):
        for P in SIZES:
            for off in OFFSETS:
                eqn = eqns[n % len(eqns)]  # every expression meets every kind of shape
                n += 1
                # rows of P bytes, and rows padded to a multiple of 16 (every vector width
                # can then be aligned: head, vector part and tail by the offset)
                for pad in (0, (-P) % 16 + 16):
                    total += _check(engine, fns[eqn], eqn, host, dev, K, P, off, pad, counter)
    # the counter accumulates over the calls
    assert int(counter.item()) == total and total > 0
    # each expression on one shape with head, vector part and tail, for all of the corpus
    for eqn in eqns:
        c = torch.zeros(1, dtype=torch.int64, device=engine.device)
        want = _check(engine, fns[eqn], eqn, host, dev, 3, 1027, 1, 13, c)
        assert int(c.item()) == want
        _check(engine, fns[eqn], eqn, host, dev, 3, 1027, 1, 13, None)  # no counter


def test_apply_mask_row_stride_keeps_the_vector_path_exact(engine, stacks):
    """valid_stride > P with aligned rows (a multiple of 16) and unaligned ones."""
    host, dev = stacks[np.dtype(np.uint8)]
    eqn = 'B3 & 6 == 0'
    fn = engine.compile_mask(MaskProgram(eqn, np.uint8, NUMBERS))
    for pad in (16, 32 - 1027 % 32, 3):
        for off in (0, 5):
            _check(engine, fn, eqn, host, dev, 3, 1027 if pad != 16 else 1024, off, pad)


def test_apply_mask_interleaved_and_sparse_slots(engine, stacks):
    host, dev = stacks[np.dtype(np.int16)]
    K, P = 3, 301
    # pixel-interleaved planes: band stride 1, pixel stride NB
    inter = dev[:, :, :P].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert inter.stride() == (4 * P, 1, 4)
    eqn = '(B1 > 0) & (B4 != B2)'
    fn = engine.compile_mask(MaskProgram(eqn, np.int16, NUMBERS))
    valid = torch.ones((K, P), dtype=torch.uint8, device=engine.device)
    engine.apply_mask(fn, inter, valid)
    keep = mf.numpy_mask(eqn, np.moveaxis(host[:, :, :P], 1, 0))
    assert np.array_equal(valid.cpu().numpy(), keep.astype(np.uint8))
    # a program over bands 2 and 6 of a three-plane stack holding bands 2, 4, 6: slots 0 and 2
    eqn = 'B6 - B2 > 100'
    prog = MaskProgram(eqn, np.int16, [2, 4, 6])
    assert prog.slots == [0, 2]
    three = dev[:, 1:4, 3:3 + P]
    valid = torch.ones((K, P), dtype=torch.uint8, device=engine.device)
    c = torch.zeros(1, dtype=torch.int64, device=engine.device)
    engine.apply_mask(engine.compile_mask(prog), three, valid, dropped=c)
    keep = mf.numpy_mask(eqn, np.moveaxis(host[:, 1:4, 3:3 + P], 1, 0), numbers=(2, 4, 6))
    assert np.array_equal(valid.cpu().numpy(), keep.astype(np.uint8))
    assert int(c.item()) == int((~keep).sum())


def test_apply_mask_rejected_arguments_launch_nothing(engine, stacks):
    from land_trendr_amd import _abi
    from land_trendr_amd.engine import LtError
    import ctypes
    host, dev = stacks[np.dtype(np.int16)]
    fn = engine.compile_mask(MaskProgram('B3 != 0', np.int16, NUMBERS))
    K, P = 3, 64
    bands = dev[:, :, :P]
    valid = torch.full((K, P), 3, dtype=torch.uint8, device=engine.device)
    bad = [
        (bands.to(torch.int32), valid, None),                       # band type
        (bands[:, :3], valid, None),                                # plane count
        (bands.cpu(), valid, None),                                 # device
        (bands, valid[:2], None),                                   # shape
        (bands, valid.to(torch.int16), None),                       # validity type
        (bands, torch.full((K, 2 * P), 3, dtype=torch.uint8, device=engine.device)[:, ::2], None),
        (bands, valid, torch.zeros(1, dtype=torch.int32, device=engine.device)),
        (bands, valid, torch.zeros(2, dtype=torch.int64, device=engine.device)),
    ]
    for b, v, d in bad:
        with pytest.raises(LtError):
            engine.apply_mask(fn, b, v, dropped=d)
    # the C entry point: null and negative arguments are LT_ERR_ARG
    lib = engine.lib
    io = _abi.LtMaskIO()
    io.n_pix, io.n_obs, io.obs_stride, io.band_stride, io.band_pix_stride = P, K, 4 * 1040, 1040, 1
    io.bands, io.valid, io.valid_stride = bands.data_ptr(), valid.data_ptr(), P
    for field, value in (('bands', None), ('valid', None), ('n_pix', -1), ('n_obs', -1),
                         ('obs_stride', -1), ('band_stride', -1), ('band_pix_stride', 0),
                         ('valid_stride', P - 1), ('n_obs', 65536)):
        keep = getattr(io, field)
        setattr(io, field, value)
        assert lib.lt_mask_apply(engine.ctx, fn.handle, ctypes.byref(io), None) != 0, field
        setattr(io, field, keep)
    assert lib.lt_mask_apply(engine.ctx, None, ctypes.byref(io), None) != 0
    assert lib.lt_mask_apply(engine.ctx, fn.handle, None, None) != 0
    torch.cuda.synchronize()
    assert (valid == 3).all()  # nothing ran
    # compile: a malformed program is LT_ERR_ARG, the same program is compiled once
    p = MaskProgram('B3 != 0', np.int16, NUMBERS).to_c()
    p.n_ops = 2
    h = ctypes.c_void_p()
    assert lib.lt_mask_compile(engine.ctx, ctypes.byref(p), ctypes.byref(h)) != 0
    again = engine.compile_mask(MaskProgram('B3 != 0', np.int16, NUMBERS))
    assert again.handle.value == fn.handle.value


# ---- analysis_reducer_batch ----
SETTINGS = {'line_cost': 10, 'target_date': '2014-07-01', 'index_eqn': 'B1 - B2',
            'mask_eqn': '(B3 & 6 == 0) & (B1 != -9999)',
            'label_rules': [{'name': 'gd', 'val': 1, 'change_type': 'GD'}]}


def _bits_equal(a, b):
    if a.dtype.kind == 'f':
        return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def test_analysis_reducer_batch_with_mask_eqn(engine):
    from land_trendr_amd.engine import ALL_FIELDS
    from land_trendr_amd.scene import build_scene, parse_date
    from land_trendr_amd.settings import compile_params
    from land_trendr_amd.synth import make_scene
    from land_trendr_amd.utils import analysis_reducer_batch
    from oracle import oracle
    sc = make_scene(389, seed=23, n_years=20, k_min=1, k_max=3, mask_prob=0.15, with_bands=True)
    K, _, P = sc.bands.shape
    rng = np.random.default_rng(4)
    qa = rng.choice(np.array([0, 0, 0, 1, 2, 4, 8, 66], np.int16), (K, 1, P))
    b = np.concatenate([sc.bands.numpy(), qa], axis=1)
    b[:, 0][rng.random((K, P)) < 0.05] = -9999  # fill pixels in B1
    keep = mf.numpy_mask(SETTINGS['mask_eqn'], np.moveaxis(b, 1, 0), numbers=(1, 2, 3))
    assert 0.2 < keep.mean() < 0.9
    dev = engine.device
    bands = torch.from_numpy(b).to(dev)
    values = torch.from_numpy((b[:, 0] - b[:, 1]).astype(np.int16)).to(dev)
    plain = {k: v for k, v in SETTINGS.items() if k != 'mask_eqn'}
    for valid in (None, sc.valid.numpy()):
        v_dev = None if valid is None else torch.from_numpy(valid).to(dev)
        before = None if valid is None else v_dev.clone()
        got = analysis_reducer_batch(sc.dates, None, v_dev, SETTINGS, fields=ALL_FIELDS,
                                     bands=bands)
        both = keep.astype(np.uint8) if valid is None else np.where(keep, valid, 0)
        want = analysis_reducer_batch(sc.dates, values, torch.from_numpy(both).to(dev), plain,
                                      fields=ALL_FIELDS)
        torch.cuda.synchronize()
        if valid is not None:
            assert torch.equal(v_dev, before)  # the caller's tensor is untouched
        meta = build_scene(sc.dates, parse_date(SETTINGS['target_date']))
        params, _ = compile_params(SETTINGS['line_cost'], SETTINGS['label_rules'])
        ora = oracle.analyze_tile(meta, params, values.cpu().numpy().astype(np.float64), both,
                                  n_threads=min(os.cpu_count() or 1, 16))
        for f in ALL_FIELDS:
            assert _bits_equal(got[f].cpu().numpy(), want[f].cpu().numpy()).all(), f
        assert len(ora) >= 10
        for f in ora:
            assert _bits_equal(got[f].cpu().numpy(), ora[f]).all(), f
    # without the key the same call ignores the third band
    a = analysis_reducer_batch(sc.dates, None, None, plain, bands=bands)
    c = analysis_reducer_batch(sc.dates, values, None, plain)
    assert torch.equal(a['matched'], c['matched'])


# ---- LocalJob ----
def _run(tmp_path, name, mode, both=False, **kw):
    from land_trendr_amd.job import LocalJob
    root = str(tmp_path / name)
    mf.make_mask_job(root, mode, both=both)
    kw.setdefault('tile_pixels', 1 << 20)
    j = LocalJob(root, 'synth', device=0, on_error='skip', **kw)
    return j, j.run()


def _same_job(a, fa, b, fb):
    assert sorted(a.planes) == sorted(b.planes)
    for k in a.planes:
        assert a.planes[k].dtype == b.planes[k].dtype, k
        assert np.asarray(a.planes[k]).tobytes() == np.asarray(b.planes[k]).tobytes(), k
    assert sorted(fa) == sorted(fb) and len(fa) > 0
    for k, paths in fa.items():
        for pa, pb in zip(paths, fb[k]):
            assert os.path.basename(pa) == os.path.basename(pb)
            assert open(pa, 'rb').read() == open(pb, 'rb').read(), k


@pytest.fixture(scope='module')
def cloud_job(tmp_path_factory):
    """The `_cloudmask` job every mask_eqn job below must equal (host decode and sampling)."""
    return _run(tmp_path_factory.mktemp('cloud'), 'cloud', 'cloud')


def _expect_stats(j):
    b, v = j.stack['bands'], j.stack['valid']
    assert j.stack['band_numbers'] == [1, 2, 3]
    drop = (v != 0) & (b[:, 2, :] == 0)
    assert j.mask_stats == {'eqn': 'B3 != 0', 'observations': int(np.count_nonzero(v)),
                            'dropped': int(np.count_nonzero(drop))}
    assert 0 < j.mask_stats['dropped'] < j.mask_stats['observations']


@pytest.mark.parametrize('decode,sample', [('host', 'host'), ('device', 'host'),
                                           ('device', 'device')])
def test_job_mask_eqn_equals_the_cloudmask_job(tmp_path, cloud_job, decode, sample):
    c, fc = cloud_job
    assert c.mask_stats is None  # a job without the key
    e, fe = _run(tmp_path, 'eqn', 'eqn', decode=decode, sample=sample)
    _same_job(e, fe, c, fc)
    _expect_stats(e)
    if decode == 'device':
        assert e.decode_stats['device'] > 0
    if sample == 'device':
        assert e.sample_stats['rasters'] >= 2
    # stack['valid'] keeps the ingest validity: coverage only, the QA zeros still valid there
    v = e.stack['valid']
    assert ((e.stack['bands'][:, 2, :] == 0) & (v != 0)).any()
    assert np.array_equal(np.where(e.stack['bands'][:, 2, :] != 0, v, 0), c.stack['valid'])


def test_job_mask_eqn_several_tiles(tmp_path, cloud_job):
    e, fe = _run(tmp_path, 'eqn', 'eqn', tile_pixels=17)
    assert len(e.mosaic.mine) >= 5
    _same_job(e, fe, *cloud_job)
    _expect_stats(e)


def test_job_mask_eqn_tile_upload(tmp_path, cloud_job, monkeypatch):
    monkeypatch.setenv('LT_JOB_UPLOAD', 'tile')
    e, fe = _run(tmp_path, 'eqn', 'eqn', tile_pixels=50)
    assert len(e.mosaic.mine) >= 2
    _same_job(e, fe, *cloud_job)
    _expect_stats(e)


def test_job_cloudmask_and_mask_eqn_combine_with_and(tmp_path):
    c, fc = _run(tmp_path, 'cloud', 'cloud', both=True)
    e, fe = _run(tmp_path, 'eqn', 'eqn', both=True, decode='device', sample='device')
    assert sum(1 for m in e.mask_fns if m) >= 3 and all(c.mask_fns)
    _same_job(e, fe, c, fc)
    _expect_stats(e)
