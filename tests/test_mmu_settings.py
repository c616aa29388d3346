"""settings.json mmu on the CPU: every accepted and rejected form (settings.check_mmu), that the C
settings reader ignores the key, and LocalJob: what it refuses and when, that a job without the key
writes what it wrote before, and the sieved label rasters through a CPU double whose sieve is the
kernels' host twin."""
import json
import os

import numpy as np
import pytest

import sievefixture as sx
from land_trendr_amd import _abi

BASE = {'index_eqn': 'B1', 'line_cost': 10, 'target_date': '2014-07-01'}


def test_accepted_forms():
    from land_trendr_amd.settings import check_mmu, load_settings, mmu_options
    assert mmu_options(BASE) is None and check_mmu(dict(BASE)) == BASE
    full = {'min_pixels': 11, 'connectivity': 8, 'by': 'onset_year'}
    assert mmu_options(dict(BASE, mmu=11)) == full
    assert mmu_options(dict(BASE, mmu={'min_pixels': 11})) == full
    assert mmu_options(dict(BASE, mmu={'min_pixels': 1, 'connectivity': 4, 'by': 'match'})) == {
        'min_pixels': 1, 'connectivity': 4, 'by': 'match'}
    for good in (1, 2 ** 31 - 1, {'min_pixels': 2 ** 31 - 1}, {'min_pixels': 3, 'by': 'match'},
                 {'min_pixels': 3, 'connectivity': 4}, {'min_pixels': 3, 'connectivity': 8,
                                                        'by': 'onset_year'}):
        assert load_settings(json.dumps(dict(BASE, mmu=good)))['mmu'] == good
        assert load_settings(dict(BASE, mmu=good))['mmu'] == good


@pytest.mark.parametrize('bad', [
    0, -1, 2 ** 31, True, False, 4.0, '4', None, [4], {}, {'connectivity': 8},
    {'min_pixels': 0}, {'min_pixels': True}, {'min_pixels': 2.0}, {'min_pixels': '3'},
    {'min_pixels': 2 ** 31}, {'min_pixels': None},
    {'min_pixels': 3, 'connectivity': 6}, {'min_pixels': 3, 'connectivity': '8'},
    {'min_pixels': 3, 'connectivity': True}, {'min_pixels': 3, 'connectivity': 8.0},
    {'min_pixels': 3, 'by': 'year'}, {'min_pixels': 3, 'by': None}, {'min_pixels': 3, 'by': 8},
    {'min_pixels': 3, 'minimum': 3}, {'min_pixels': 3, 'Connectivity': 8}], ids=repr)
def test_rejected_forms(bad):
    from land_trendr_amd.settings import check_mmu, load_settings, mmu_options
    for f in (check_mmu, load_settings, mmu_options):
        with pytest.raises(ValueError, match='mmu'):
            f(dict(BASE, mmu=bad))
    with pytest.raises(ValueError, match='mmu'):
        load_settings(json.dumps(dict(BASE, mmu=bad)))


def test_the_c_settings_reader_ignores_the_key():
    import ctypes
    lib = _abi.load_lib()

    def compiled(settings):
        st, n = _abi.LtSettings(), ctypes.c_int32(0)
        err = ctypes.create_string_buffer(512)
        rc = lib.lt_settings_compile(json.dumps(settings).encode(), 1, 0, 2, 0, ctypes.byref(st),
                                     ctypes.byref(n), err, 512)
        return rc, bytes(st), n.value
    from jobfixture import SETTINGS
    plain = compiled(SETTINGS)
    assert plain[0] == 0
    assert compiled(dict(SETTINGS, mmu=11)) == plain
    assert compiled(dict(SETTINGS, mmu={'min_pixels': 4, 'connectivity': 4, 'by': 'match'})) == plain


# ---- LocalJob ----

def run_job(root, job, settings, engine, **kw):
    from jobfixture import make_job
    from land_trendr_amd.job import LocalJob
    make_job(root, job, rows=24, cols=40, seed=5, settings=settings)
    j = LocalJob(root, job, on_error='skip', engine=engine, trendline=False, **kw)
    return j, j.run()


def file_bytes(files):
    out = {}
    for k, (path,) in files.items():
        with open(path, 'rb') as fh:
            out[k] = fh.read()
    return out


def test_the_oracle_double_has_no_sieve_and_output_says_so(tmp_path):
    from engine_double import OracleEngine
    from jobfixture import SETTINGS, make_job
    from land_trendr_amd.job import LocalJob
    root = str(tmp_path)
    make_job(root, 'mmu', rows=6, cols=7, settings=dict(SETTINGS, mmu=3))
    j = LocalJob(root, 'mmu', on_error='skip', engine=OracleEngine(), trendline=False)
    j.setup()
    j.parse()
    j.analyze()
    with pytest.raises(RuntimeError, match='mmu needs the HIP engine'):
        j.output()


def test_world_size_two_and_bad_keys_are_refused_at_construction(tmp_path, monkeypatch):
    from jobfixture import SETTINGS, make_job
    from land_trendr_amd.job import LocalJob
    root = str(tmp_path)
    make_job(root, 'mmu', rows=3, cols=3, settings=dict(SETTINGS, mmu=3))
    make_job(root, 'bad', rows=3, cols=3, settings=dict(SETTINGS, mmu={'min_pixels': 3, 'x': 1}))
    make_job(root, 'plain', rows=3, cols=3, settings=SETTINGS)
    with pytest.raises(ValueError, match='mmu'):
        LocalJob(root, 'bad', engine=sx.make_twin_engine())
    monkeypatch.setattr(LocalJob, '_dist', staticmethod(lambda: (object(), 2, 0)))
    with pytest.raises(ValueError, match='one rank'):
        LocalJob(root, 'mmu', engine=sx.make_twin_engine())
    LocalJob(root, 'plain', engine=sx.make_twin_engine())  # without the key: no objection


@pytest.mark.parametrize('mode', ['reference', 'typed'])
def test_job_through_the_host_twin(tmp_path, mode):
    """The job's pass with the host twin as the engine's sieve: a job without the key writes what
    the plain engine double writes; with it, the label rasters of each rule lose exactly the
    patches the reference finds on the first run's planes."""
    from engine_double import OracleEngine
    from jobfixture import SETTINGS
    from land_trendr_amd.geotiff import GeoTiff
    from land_trendr_amd.raster import LABEL_KEYS, label_rasters
    root = str(tmp_path)
    _, before = run_job(root, 'before', SETTINGS, OracleEngine(), raster_mode=mode)
    plain, files0 = run_job(root, 'plain', SETTINGS, sx.make_twin_engine(), raster_mode=mode)
    assert plain.mmu_stats is None
    assert file_bytes(files0) == file_bytes(before)
    one, files1 = run_job(root, 'one', dict(SETTINGS, mmu=1), sx.make_twin_engine(),
                          raster_mode=mode)
    assert file_bytes(files1) == file_bytes(files0)  # min_pixels 1 changes nothing
    assert all(v['removed'] == 0 and v['matched'] > 0 for v in one.mmu_stats.values())
    j, files = run_job(root, 'mmu', dict(SETTINGS, mmu={'min_pixels': 4}), sx.make_twin_engine(),
                       raster_mode=mode)
    assert j._raster_hw == (24, 40)
    pl = {f: a.copy() for f, a in plain.planes.items()}
    tmpl = GeoTiff(j.rast_fns[0])
    for r, rule in enumerate(j.rules):
        m = (pl['matched'][r] != 0).astype(np.uint8)
        _, size = sx.reference(m, pl['onset_year'][r], (24, 40), 8)
        gone = (size > 0) & (size < 4)
        assert gone.any() and (size >= 4).any(), rule.name
        assert j.mmu_stats[rule.name] == {'matched': int(m.sum()), 'removed': int(gone.sum())}
        pl['matched'][r][gone] = 0
    want = label_rasters(pl, j.rules, (24, 40), tmpl.dtype.newbyteorder('='), mode)
    assert len(want) == len(j.rules) * len(LABEL_KEYS) and sorted(want) == sorted(files)
    for k, w in want.items():
        a = GeoTiff(files[k][0]).read()[0]
        assert a.dtype == w.dtype and (a == w).all(), k
