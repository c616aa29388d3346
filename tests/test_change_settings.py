"""settings.json change_maps on the CPU: every accepted and rejected form
(settings.check_change_maps), the defaults change_map_options fills in, the map-level / top-level
mmu precedence, that the C settings reader ignores the key, and what LocalJob refuses and when."""
import json

import pytest

import changefixture as cx
from land_trendr_amd import _abi

BASE = {'index_eqn': 'B1', 'line_cost': 10, 'target_date': '2014-07-01'}
A = {'name': 'a', 'delta': 'loss'}


def test_accepted_forms_and_defaults():
    from land_trendr_amd.settings import (CHANGE_SORTS, change_map_options, check_change_maps,
                                          load_settings)
    assert change_map_options(BASE) is None and check_change_maps(dict(BASE)) == BASE
    full = {'name': 'a', 'delta': 'loss', 'sort': 'greatest', 'index_sign': 1, 'year': None,
            'mag': None, 'dur': None, 'preval': None, 'mmu': None}
    assert change_map_options(dict(BASE, change_maps=[A])) == [full]
    every = {'name': 'Gain_2', 'delta': 'gain', 'sort': 'steepest', 'index_sign': -1,
             'year': [1990, 1990], 'mag': ['>', 130], 'dur': ['<=', 4.5], 'preval': ['>=', -3],
             'mmu': {'min_pixels': 3, 'connectivity': 4, 'by': 'match'}}
    assert change_map_options(dict(BASE, change_maps=[every])) == [every]
    assert CHANGE_SORTS == cx.SORTS
    goods = [[dict(A, sort=s)] for s in CHANGE_SORTS]
    goods += [[dict(A, **{k: [op, 0]})] for k in ('mag', 'dur', 'preval')
              for op in ('>', '<', '>=', '<=')]
    goods += [[dict(A, year=[-5, 3000])], [dict(A, mmu=1)], [dict(A, mmu=7)],
              [dict(A, name='m%d' % i) for i in range(8)],
              [dict(A, index_sign=-1), {'name': 'b', 'delta': 'gain'}]]
    for good in goods:
        assert load_settings(json.dumps(dict(BASE, change_maps=good)))['change_maps'] == good
        assert load_settings(dict(BASE, change_maps=good))['change_maps'] == good
        assert len(change_map_options(dict(BASE, change_maps=good))) == len(good)


def test_mmu_precedence():
    from land_trendr_amd.settings import change_map_options
    top = {'min_pixels': 5, 'connectivity': 4, 'by': 'match'}
    maps = [A, dict(A, name='own', mmu=9), dict(A, name='off', mmu=1),
            dict(A, name='long', mmu={'min_pixels': 2, 'by': 'match'})]
    opts = change_map_options(dict(BASE, mmu=top, change_maps=maps))
    assert [o['mmu'] for o in opts] == [
        top, {'min_pixels': 9, 'connectivity': 8, 'by': 'onset_year'},
        {'min_pixels': 1, 'connectivity': 8, 'by': 'onset_year'},
        {'min_pixels': 2, 'connectivity': 8, 'by': 'match'}]
    opts = change_map_options(dict(BASE, mmu=3, change_maps=maps))
    assert opts[0]['mmu'] == {'min_pixels': 3, 'connectivity': 8, 'by': 'onset_year'}
    opts = change_map_options(dict(BASE, change_maps=maps))
    assert opts[0]['mmu'] is None and opts[1]['mmu']['min_pixels'] == 9


@pytest.mark.parametrize('bad', [
    [], {}, None, 'loss', 3, True, [A] * 2, [dict(A, name='m%d' % i) for i in range(9)],
    [['a', 'loss']], [None], [{'delta': 'loss'}], [{'name': 'a'}], [dict(A, name='a b')],
    [dict(A, name='')], [dict(A, name=3)], [dict(A, name='a/b')],
    [dict(A, delta='both')], [dict(A, delta=None)], [dict(A, delta=['loss'])],
    [dict(A, sort='biggest')], [dict(A, sort=0)], [dict(A, sort=None)],
    [dict(A, index_sign=0)], [dict(A, index_sign=2)], [dict(A, index_sign=True)],
    [dict(A, index_sign=1.0)], [dict(A, index_sign='-1')],
    [dict(A, year=1990)], [dict(A, year=[1990])], [dict(A, year=[1990, 1991, 1992])],
    [dict(A, year=[1991, 1990])], [dict(A, year=[1990.0, 1991])], [dict(A, year=[1990, True])],
    [dict(A, year=['1990', '1991'])], [dict(A, year=[1990, 2 ** 31])], [dict(A, year=None)],
    [dict(A, mag=5)], [dict(A, mag=['>'])], [dict(A, mag=['==', 5])], [dict(A, mag=['>', '5'])],
    [dict(A, mag=['>', True])], [dict(A, mag=['>', None])], [dict(A, mag=[5, '>'])],
    [dict(A, dur=['=>', 2])], [dict(A, dur=['>', 2, 3])], [dict(A, dur=None)],
    [dict(A, preval=['!=', 0])], [dict(A, preval=[None, 0])], [dict(A, preval={'>': 0})],
    [dict(A, mmu=0)], [dict(A, mmu=True)], [dict(A, mmu={'connectivity': 8})],
    [dict(A, mmu={'min_pixels': 3, 'by': 'year'})], [dict(A, mmu=2.0)],
    [dict(A, magnitude=['>', 5])], [dict(A, Sort='least')], [dict(A, pre_threshold=['>', 1])]],
    ids=repr)
def test_rejected_forms(bad):
    from land_trendr_amd.settings import change_map_options, check_change_maps, load_settings
    for f in (check_change_maps, load_settings, change_map_options):
        with pytest.raises(ValueError, match='change_maps'):
            f(dict(BASE, change_maps=bad))
    with pytest.raises(ValueError, match='change_maps'):
        load_settings(json.dumps(dict(BASE, change_maps=bad)))


def test_the_rule_struct_follows_the_options():
    from land_trendr_amd.settings import change_map_options
    opt, = change_map_options(dict(BASE, change_maps=[
        {'name': 'x', 'delta': 'gain', 'sort': 'gentlest', 'index_sign': -1, 'year': [1988, 1994],
         'mag': ['>', 130], 'dur': ['<=', 4], 'preval': ['>=', 600.5]}]))
    r = _abi.change_rule(opt)
    assert (r.delta, r.sort, r.index_sign) == (_abi.LT_CM_GAIN, _abi.LT_CS_GENTLEST, -1)
    assert (r.year_set, r.year_lo, r.year_hi) == (1, 1988, 1994)
    assert (r.mag_op, r.dur_op, r.pre_op) == (_abi.LT_Q_GT, _abi.LT_Q_LE, _abi.LT_Q_GE)
    assert (r.mag_val, r.dur_val, r.pre_val) == (130.0, 4.0, 600.5)
    r = _abi.change_rule({'delta': 'loss'})
    assert (r.delta, r.sort, r.index_sign, r.year_set) == (0, 0, 1, 0)
    assert (r.mag_op, r.dur_op, r.pre_op) == (0, 0, 0)


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
    assert compiled(dict(SETTINGS, change_maps=[A])) == plain
    assert compiled(dict(SETTINGS, change_maps=[
        dict(A, sort='newest', year=[1990, 1991], mag=['>', 5], mmu={'min_pixels': 4})])) == plain


def test_world_size_two_and_bad_keys_are_refused_at_construction(tmp_path, monkeypatch):
    from jobfixture import SETTINGS, make_job
    from land_trendr_amd.job import LocalJob
    root = str(tmp_path)
    make_job(root, 'cm', rows=3, cols=3, settings=dict(SETTINGS, change_maps=[A]))
    make_job(root, 'bad', rows=3, cols=3, settings=dict(SETTINGS, change_maps=[dict(A, x=1)]))
    make_job(root, 'plain', rows=3, cols=3, settings=SETTINGS)
    with pytest.raises(ValueError, match='change_maps'):
        LocalJob(root, 'bad', engine=cx.make_twin_engine())
    LocalJob(root, 'cm', engine=cx.make_twin_engine())
    monkeypatch.setattr(LocalJob, '_dist', staticmethod(lambda: (object(), 2, 0)))
    with pytest.raises(ValueError, match='one rank'):
        LocalJob(root, 'cm', engine=cx.make_twin_engine())
    LocalJob(root, 'plain', engine=cx.make_twin_engine())  # without the key: no objection


def test_an_engine_without_change_maps_is_refused(tmp_path):
    from engine_double import OracleEngine
    from jobfixture import SETTINGS, make_job
    from land_trendr_amd.job import LocalJob
    root = str(tmp_path)
    make_job(root, 'cm', rows=6, cols=7, settings=dict(SETTINGS, change_maps=[A]))
    j = LocalJob(root, 'cm', on_error='skip', engine=OracleEngine(), trendline=False)
    j.setup()
    j.parse()
    with pytest.raises(RuntimeError, match='change_maps needs the HIP engine'):
        j.analyze()
