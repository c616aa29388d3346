"""The zonal table on the MI355X (lt_zonal_stats, lt_zonal.hip): the cases of zonalfixture through
Engine.zonal_stats on every path the table allows against the numpy reference, guarded buffers, a
second launch, a 1024 x 1024 field against the host twin, the argument checks, and LocalJob on the
HIP engine against the CPU double's run. Integer sums: no tolerance anywhere."""
import ctypes
import os

import numpy as np
import pytest
import torch

import changefixture as cx
import zonalfixture as zx
from land_trendr_amd.engine import LtError, get_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    return get_engine(0)


@pytest.fixture(scope='module')
def lib():
    return zx.load_host()


def dev(eng, a):
    return None if a is None else torch.from_numpy(np.array(a, order='C')).to(eng.device)


def run_case(eng, c, path, planes=None):
    """Engine.zonal_stats on a case, c['times'] calls into one table that starts from c['start']
    (None: the engine's own zeroed table) -> the device table."""
    t = planes or {f: dev(eng, a) for f, a in zx.planes(c).items()}
    out = dev(eng, c['start'])
    for _ in range(c['times']):
        res = eng.zonal_stats(t['matched'], t['zone'], t['key'], c['key_lo'], c['n_bins'],
                              c['n_zones'], duration=t['duration'], value=t['value'], out=out,
                              _path=path)
        assert out is None or res is out
        out = res
    return out


def check_device_sparse(table, sparse, what):
    """A device table that started from zero holds exactly the reference's cells and words (the
    non-zero cells are found on the device: only they come down)."""
    cells, words = sparse
    flat = table.view(-1, 4)
    got = flat.ne(0).any(dim=1).nonzero().squeeze(1)
    assert np.array_equal(got.cpu().numpy(), cells), what
    assert np.array_equal(flat[got].cpu().numpy(), words), what


@pytest.mark.parametrize('pattern', zx.PATTERNS)
def test_cases_against_the_reference_on_every_path(eng, pattern):
    n = 0
    for P, Z, B in zx.shapes(pattern):
        c = zx.case(pattern, P, Z, B)
        planes = {f: dev(eng, a) for f, a in zx.planes(c).items()}
        for path in (0,) + zx.paths(Z, B):
            got = run_case(eng, c, path, planes)
            what = (pattern, P, Z, B, path)
            assert got.dtype == torch.int64 and tuple(got.shape) == (Z + 1, B + 1, 4)
            if c['start'] is None and c['times'] == 1:
                check_device_sparse(got, zx.case_sparse(pattern, P, Z, B), what)
            else:
                assert np.array_equal(got.cpu().numpy(), zx.case_dense(pattern, P, Z, B)), what
            n += 1
    assert n >= 2 * len(zx.shapes(pattern))


def test_null_planes_leave_their_words(eng):
    for pattern, kept in (('null_dur', [1]), ('null_val', [2, 3]), ('null_both', [1, 2, 3])):
        c = zx.case(pattern, 70001, 7, 30)
        for path in (1, 2):
            got = run_case(eng, c, path).cpu().numpy()
            assert np.array_equal(got[..., kept], c['start'][..., kept]), (pattern, path)
            assert (got[..., 0] != c['start'][..., 0]).any()


@pytest.mark.parametrize('pattern, P, Z, B', [('mixed', 16385, 7, 30), ('lane_cells', 70001, 300, 30),
                                              ('one_cell', 257, 2, 256), ('runs', 65, 300, 1)])
def test_guarded_buffers_and_a_second_launch(eng, pattern, P, Z, B):
    """The planes end where an unrelated buffer begins and the table sits between guard words:
    nothing outside the table is written, and a second launch agrees in every word."""
    c = zx.case(pattern, P, Z, B)
    G = 64
    planes = {}
    for f, a in zx.planes(c).items():
        buf = np.full(P + 2 * G, 0x55, a.dtype) if a.dtype.kind != 'f' else np.full(P + 2 * G, 1e9)
        buf[G:G + P] = a
        planes[f] = dev(eng, buf)[G:G + P]
    n = (Z + 1) * (B + 1) * 4
    want = zx.case_dense(pattern, P, Z, B)
    for path in zx.paths(Z, B):
        seen = []
        for _ in range(2):
            buf = torch.full((n + 2 * G,), 0x5555, dtype=torch.int64, device=eng.device)
            out = buf[G:G + n].view(Z + 1, B + 1, 4)
            out.zero_()
            assert eng.zonal_stats(planes['matched'], planes['zone'], planes['key'], c['key_lo'],
                                   B, Z, planes['duration'], planes['value'], out=out,
                                   _path=path) is out
            h = buf.cpu().numpy()
            assert (h[:G] == 0x5555).all() and (h[G + n:] == 0x5555).all(), (pattern, path)
            seen.append(h[G:G + n].reshape(Z + 1, B + 1, 4))
        assert np.array_equal(seen[0], want) and np.array_equal(seen[1], want), (pattern, path)


def test_block_zones_field_equals_the_host_twin(eng, lib):
    """1024 x 1024 pixels, 64 x 64-pixel block zones, 30 onset years: every word of the device
    table is the host twin's, on both paths and in a second launch."""
    H = W = 1024
    rng = np.random.default_rng(11)
    r, col = np.divmod(np.arange(H * W), W)
    zone = ((r // 64) * (W // 64) + col // 64).astype(np.int32)
    # onset years in patches of 8 x 8 with single-pixel noise, a fifth of the pixels matched
    patch = rng.integers(0, 30, (H // 8, W // 8))[r // 8, col // 8]
    key = (1985 + np.where(rng.random(H * W) < 0.1, rng.integers(0, 30, H * W), patch)).astype(
        np.int32)
    matched = (rng.random(H * W) < 0.2).astype(np.uint8)
    matched[:64 * W] = 1            # (the first row of zones: every pixel matched)
    duration = rng.integers(1, 12, H * W).astype(np.int32)
    value = rng.normal(400.0, 250.0, H * W)
    c = dict(matched=matched, zone=zone, key=key, duration=duration, value=value, key_lo=1985,
             n_bins=30, n_zones=256, start=None, times=1)
    want = zx.host_table(lib, c)
    # every zone and every year has pixels, most cells do, and no pixel is outside
    assert want[:256, :30, 0].sum(axis=1).min() > 0 and want[:256, :30, 0].sum(axis=0).min() > 0
    assert (want[:256, :30, 0] > 0).mean() > 0.9 and want[256].sum() == 0 and want[:, 30].sum() == 0
    planes = {f: dev(eng, a) for f, a in zx.planes(c).items()}
    for path in (0, 2, 2):
        got = run_case(eng, c, path, planes).cpu().numpy()
        assert np.array_equal(got, want), path
    # the same field over 3 zones takes the LDS path
    c3 = dict(c, zone=(zone % 3).astype(np.int32), n_zones=3)
    want3 = zx.host_table(lib, c3)
    planes['zone'] = dev(eng, c3['zone'])
    for path in (0, 1, 1, 2):
        assert np.array_equal(run_case(eng, c3, path, planes).cpu().numpy(), want3), path


def test_engine_argument_checks(eng):
    m = dev(eng, np.ones(9, np.uint8))
    z = dev(eng, np.zeros(9, np.int32))
    k = dev(eng, np.full(9, 2, np.int32))
    d = dev(eng, np.ones(9, np.int32))
    v = dev(eng, np.ones(9))
    ok = eng.zonal_stats(m, z, k, 0, 4, 2, d, v)
    assert ok.cpu().numpy()[0, 2].tolist() == [9, 9, 9 * 16, 9]
    for args, kw in (((m, z, k, 0, 0, 2), {}), ((m, z, k, 0, 257, 2), {}), ((m, z, k, 0, 4, 0), {}),
                     ((m, z, k, 0, 4, 65537), {}), ((m, z, k, 2 ** 31, 4, 2), {}),
                     ((m, z, k, 0.0, 4, 2), {}), ((m, z, k, 0, True, 2), {}),
                     ((m.cpu(), z, k, 0, 4, 2), {}), ((m, z[:8], k, 0, 4, 2), {}),
                     ((m, z.long(), k, 0, 4, 2), {}), ((m, z, k.float(), 0, 4, 2), {}),
                     ((m, z, k, 0, 4, 2), {'duration': d.long()}),
                     ((m, z, k, 0, 4, 2), {'value': v.float()}),
                     ((m, z, k, 0, 4, 2), {'value': v[:8]}),
                     ((m, z, k, 0, 4, 2), {'out': torch.zeros((3, 5, 4), dtype=torch.int32,
                                                              device=eng.device)}),
                     ((m, z, k, 0, 4, 2), {'out': torch.zeros((3, 5, 3), dtype=torch.int64,
                                                              device=eng.device)}),
                     ((m, z, k, 0, 4, 2), {'_path': 3}),
                     ((m, z, k, 0, 30, 300), {'_path': 1})):
        with pytest.raises(LtError):
            eng.zonal_stats(*args, **kw)
    e = dev(eng, np.zeros(0, np.uint8)), dev(eng, np.zeros(0, np.int32))
    assert eng.zonal_stats(e[0], e[1], e[1], 0, 4, 2).cpu().numpy().sum() == 0


def test_argument_errors_launch_nothing(eng):
    m = dev(eng, np.ones(9, np.uint8))
    z = dev(eng, np.zeros(9, np.int32))
    k = dev(eng, np.full(9, 2, np.int32))
    st = ctypes.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
    t = torch.full((3, 5, 4), 77, dtype=torch.int64, device=eng.device)
    M, Zp, K, T = m.data_ptr(), z.data_ptr(), k.data_ptr(), t.data_ptr()

    def call(mp=M, zp=Zp, kp=K, n=9, n_bins=4, n_zones=2, path=0, tp=T):
        return eng.lib.lt_zonal_stats(eng.ctx, mp, zp, kp, None, None, n, 0, n_bins, n_zones,
                                      path, tp, st)
    A = zx.LT_ERR_ARG
    assert call(mp=None) == A and call(zp=None) == A and call(kp=None) == A and call(tp=None) == A
    assert call(n=-1) == A and call(n_bins=0) == A and call(n_bins=257) == A
    assert call(n_zones=0) == A and call(n_zones=65537) == A
    assert call(path=-1) == A and call(path=3) == A and call(path=1, n_zones=300) == A
    assert call(n=(1 << 28) + 1) == zx.LT_ERR_LIMIT
    assert call(n=0) == zx.LT_OK and call(n=0, mp=None, tp=None, n_bins=0, n_zones=0) == zx.LT_OK
    assert eng.lib.lt_zonal_stats(None, M, Zp, K, None, None, 9, 0, 4, 2, 0, T, st) == A
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == 77).all()
    assert call() == zx.LT_OK
    torch.cuda.synchronize()
    h = t.cpu().numpy()
    assert h[0, 2].tolist() == [77 + 9, 77, 77, 77] and (np.delete(h.reshape(-1, 4), 2, 0) == 77).all()


# ---- LocalJob on the HIP engine ----

def gpu_job(root, job, settings, **kw):
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    make_job(root, job, rows=zx.SHAPE[0], cols=zx.SHAPE[1], seed=5, settings=settings)
    zx.write_zones(root, job)
    j = LocalJob(root, job, device=0, tile_pixels=400, on_error='skip', **kw)
    return j, j.run()


def csv_bytes(j):
    out = {}
    for name, path in j.zonal_files.items():
        with open(path, 'rb') as fh:
            out[name] = fh.read()
    return out


def test_job_gives_the_cpu_runs_tables(eng, tmp_path):
    """The 24 x 40 job on the HIP engine: the tables and the CSV bytes of the CPU double's run, in
    both raster modes and with either encoder; without the key no tables/ and the same rasters."""
    from jobfixture import SETTINGS, make_job
    from land_trendr_amd.job import LocalJob
    root = str(tmp_path)
    settings = dict(SETTINGS, change_maps=cx.JOB_MAPS, mmu=3,
                    zonal_stats={'zones': 'zones.tif', 'ignore': [zx.ZONE_IGNORED]})
    make_job(root, 'cpu', rows=zx.SHAPE[0], cols=zx.SHAPE[1], seed=5, settings=settings)
    zx.write_zones(root, 'cpu')
    cpu = LocalJob(root, 'cpu', on_error='skip', engine=zx.make_twin_engine(), trendline=False)
    cpu.run()
    want_csv = csv_bytes(cpu)
    assert len(want_csv) == 3 + len(cx.JOB_MAPS)
    assert all(t['pixels'].sum() > 0 for t in cpu.zonal_stats.values())
    rasters = {}
    for mode, encode in (('reference', 'host'), ('typed', 'device'), ('typed', 'host')):
        job = 'z_%s_%s' % (mode, encode)
        j, files = gpu_job(root, job, settings, trendline=False, raster_mode=mode, encode=encode)
        assert sorted(j.zonal_stats) == sorted(cpu.zonal_stats)
        for name, t in cpu.zonal_stats.items():
            for f, a in t.items():
                assert np.array_equal(j.zonal_stats[name][f], a, equal_nan=(f[:4] == 'mean')), \
                    (job, name, f)
        assert csv_bytes(j) == want_csv, job
        assert j.zonal_s > 0
        rasters[(mode, encode)] = cx.file_bytes(files)
    nokey = dict(settings)
    del nokey['zonal_stats']
    j0, files0 = gpu_job(root, 'nokey', nokey, trendline=False, raster_mode='typed')
    assert j0.zonal_stats is None
    assert not os.path.exists(os.path.join(root, 'nokey', 'output', 'tables'))
    assert cx.file_bytes(files0) == rasters[('typed', 'host')] == rasters[('typed', 'device')]
