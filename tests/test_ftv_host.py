"""Fit to vertex (lt_ftv_tile) without a GPU: the kernel's per-pixel code (lt_ftv.h) compiled for
the host against the reference goldens, the reference's own vertices2eqns / eqns2fitted_points on
second series (tests/golden/ftv_second.npz) and a numpy restatement on hand-made flags; the
ftv_eqns settings key; the ABI additions."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ftvfixture as fx
import golden_io
from land_trendr_amd import _abi
from land_trendr_amd.settings import load_settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def host():
    return fx.load_host()


@pytest.fixture(scope='module')
def fixture():
    return fx.load_fixture()


@pytest.mark.parametrize('name', golden_io.scene_names())
def test_host_twin_reproduces_the_golden_planes(host, name):
    g = golden_io.GoldenScene(name)
    winner = fx.rejected_winners(g)
    out = fx.run_host(host, g.scene, winner, g.ref['spike'], g.ref['vertex'], g.values)
    fx.check_golden(g, out, winner)


@pytest.mark.parametrize('name', fx.FIXTURE_SCENES)
@pytest.mark.parametrize('integer', [True, False])
def test_host_twin_equals_the_reference_on_second_series(host, fixture, name, integer):
    g = golden_io.GoldenScene(name)
    winner, spike, vertex, vals, want = fx.fixture_inputs(g, fixture[name], integer)
    assert winner.shape[1] > 0
    out = fx.run_host(host, g.scene, winner, spike, vertex, vals)
    fx.check_fixture(out, winner, vals, want, (name, integer))


def test_fixture_covers_the_five_kinds(fixture):
    kinds = np.concatenate([fixture[s]['kind'] for s in fx.FIXTURE_SCENES])
    assert len(kinds) >= 290 and set(kinds.tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize('Y,P,K,dtype', [(40, 130, 40, np.int16), (40, 130, 47, np.float64),
                                         (2, 9, 2, np.int16), (64, 40, 64, np.int32),
                                         (33, 70, 33, np.float32)])
def test_host_twin_equals_the_numpy_restatement_on_handmade_flags(host, Y, P, K, dtype):
    scene = fx.yearly_scene(Y, K)
    assert scene.n_years == Y and scene.n_obs == K
    winner, spike, vertex = fx.handmade(Y, P, K, seed=Y * 1000 + P)
    rng = np.random.default_rng(7 + Y)
    if np.dtype(dtype).kind == 'i':
        vals = rng.integers(-32768, 32768, (K, P)).astype(dtype)
        vals[:, 5 % P] = 0                      # an all-zero series: dgelsd's B == 0 shortcut
        vals[:, 6 % P] = rng.choice([32767, -32768], K)
    else:
        vals = rng.normal(300, 200, (K, P)).astype(dtype)
    want = fx.ftv_numpy(scene.years, winner, spike, vertex, vals)
    out = fx.run_host(host, scene, winner, spike, vertex, vals)
    for f in fx.FTV_FIELDS:
        m = ~fx.bits_equal(out[f], want[f])
        assert not m.any(), (f, int(m.sum()), np.argwhere(m)[:5].tolist())
    assert (out['status'] == want['status']).all()
    if Y == 40:  # the long segments are there: m from 5 to 38 with gaps
        ms = [int(((winner[:, p] >= 0) & (spike[:, p] == 0)).sum()) for p in range(0, P, 4)]
        assert min(ms) <= 9 and max(ms) >= 36, ms


def test_host_twin_rejected_and_malformed_pixels(host):
    Y = K = 10
    scene = fx.yearly_scene(Y)
    winner = np.tile(np.arange(Y, dtype=np.int16)[:, None], (1, 5))
    spike = np.zeros((Y, 5), np.uint8)
    vertex = np.zeros((Y, 5), np.uint8)
    vertex[0] = vertex[-1] = 1
    winner[:, 0] = -1                  # empty
    winner[:, 1] = -1
    winner[4, 1] = 4                   # one year
    vertex[:, 2] = 0                   # malformed: no vertex with T >= 2
    winner[3, 3] = K                   # malformed: not an observation -> absent
    winner[5, 3] = -7
    vals = np.arange(K * 5, dtype=np.float64).reshape(K, 5) ** 1.5
    out = fx.run_host(host, scene, winner, spike, vertex, vals)
    st = out['status']
    assert st[0] == _abi.LT_ST_EMPTY and st[1] == _abi.LT_ST_SINGLE_YEAR
    assert st[2] & _abi.LT_ST_NUMERIC and st[3] & _abi.LT_ST_NUMERIC and st[4] == 0
    for f in fx.FIT_FIELDS:
        assert np.isnan(out[f][:, :2]).all()
    assert out['val_raw'][4, 1] == vals[4, 1] and np.isnan(out['val_raw'][:, 0]).all()
    assert np.isnan(out['val_raw'][[3, 5], 3]).all()
    want = fx.ftv_numpy(scene.years, winner[:, 4:], spike[:, 4:], vertex[:, 4:], vals[:, 4:])
    for f in fx.FTV_FIELDS:
        assert fx.bits_equal(out[f][:, 4:], want[f]).all(), f


def test_host_twin_writes_only_the_requested_planes(host):
    scene = fx.yearly_scene(12)
    winner, spike, vertex = fx.handmade(12, 8, 12, seed=3)
    vals = np.random.default_rng(3).integers(-500, 500, (12, 8)).astype(np.int16)
    full = fx.run_host(host, scene, winner, spike, vertex, vals)
    one = fx.run_host(host, scene, winner, spike, vertex, vals, fields=('val_fit',))
    assert set(one) == {'val_fit', 'status'}
    assert fx.bits_equal(one['val_fit'], full['val_fit']).all()


# ---- settings.json ftv_eqns ----

BASE = {'index_eqn': 'B1 - B2', 'line_cost': 10, 'target_date': '2014-07-01', 'label_rules': []}


@pytest.mark.parametrize('eqns', [{}, {'b3': 'B3'}, {'sum': 'B1 + B3', 'TCW_2': '(B1-B2)/2',
                                                    '9': 'B1'}])
def test_ftv_eqns_accepted(eqns):
    s = dict(BASE, ftv_eqns=eqns)
    assert load_settings(s) is s
    import json
    assert load_settings(json.dumps(s))['ftv_eqns'] == eqns


@pytest.mark.parametrize('eqns', [{'a b': 'B1'}, {'': 'B1'}, {'a/b': 'B1'}, {'a-b': 'B1'},
                                  {'x\n': 'B1'}, {'b3': 3}, {'b3': None}, {'b3': ['B3']},
                                  {'b3': ''}, ['B3'], 'B3', 7, None])
def test_ftv_eqns_rejected(eqns):
    with pytest.raises(ValueError):
        load_settings(dict(BASE, ftv_eqns=eqns))


def test_settings_without_ftv_eqns_are_untouched(tmp_path):
    import json
    assert load_settings(BASE) is BASE and 'ftv_eqns' not in BASE
    path = tmp_path / 'settings.json'
    path.write_text(json.dumps(BASE))
    assert load_settings(str(path)) == BASE


# ---- ABI ----

def test_abi_struct_and_export():
    assert 'lt_ftv_tile' in _abi.EXPORTS
    assert hasattr(_abi.load_lib(), 'lt_ftv_tile')
    assert _abi.load_lib().lt_abi_version() == 8
    header = os.path.join(ROOT, 'include', 'lt_abi.h')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % header,
             'int main(void){', 'printf("size %zu\\n", sizeof(lt_ftv_in));']
    for f, _ in _abi.LtFtvIn._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(lt_ftv_in, %s));' % (f, f))
    lines.append('return 0;}')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 'l.c')
        with open(c, 'w') as fh:
            fh.write('\n'.join(lines))
        exe = os.path.join(d, 'l')
        subprocess.check_call(['gcc', '-o', exe, c])
        got = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    assert int(got['size']) == ctypes.sizeof(_abi.LtFtvIn)
    for f, _ in _abi.LtFtvIn._fields_:
        assert int(got[f]) == getattr(_abi.LtFtvIn, f).offset, f


# ---- LocalJob: what a job with ftv_eqns cannot do is said at construction ----

def _job_dir(tmp_path, settings):
    import json
    d = tmp_path / 'j' / 'input'
    d.mkdir(parents=True)
    (d / 'settings.json').write_text(json.dumps(settings))
    return str(tmp_path)


def test_job_with_ftv_eqns_needs_the_trendline_and_one_rank(tmp_path, monkeypatch):
    from land_trendr_amd.job import LocalJob
    root = _job_dir(tmp_path, dict(BASE, ftv_eqns={'b3': 'B3'}))
    assert LocalJob(root, 'j').ftv_s == {}
    with pytest.raises(ValueError, match='trendline=True'):
        LocalJob(root, 'j', trendline=False)
    monkeypatch.setattr(LocalJob, '_dist', staticmethod(lambda: (None, 2, 0)))
    with pytest.raises(ValueError, match='one rank'):
        LocalJob(root, 'j')


def test_job_rejects_bad_ftv_eqns_and_ignores_an_absent_key(tmp_path):
    from land_trendr_amd.job import LocalJob
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    with pytest.raises(ValueError, match='ftv_eqns'):
        LocalJob(_job_dir(tmp_path / 'a', dict(BASE, ftv_eqns={'a b': 'B1'})), 'j')
    LocalJob(_job_dir(tmp_path / 'b', BASE), 'j', trendline=False)   # no key: nothing changes
