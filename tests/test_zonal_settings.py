"""settings.json zonal_stats: every accepted and every rejected form (settings.check_zonal_stats,
zonal_stats_options), and that the key leaves the compiled settings alone."""
import pytest

from land_trendr_amd.settings import (check_zonal_stats, load_settings, zonal_stats_options)

MAP = {'name': 'A', 'delta': 'loss'}
RULES = [{'name': 'gd', 'val': 3, 'change_type': 'GD'}]


def test_an_absent_key_changes_nothing():
    s = {'line_cost': 10}
    assert check_zonal_stats(s) is s and zonal_stats_options(s) is None


@pytest.mark.parametrize('value, maps, want', [
    ('zones.tif', False, {'zones': 'zones.tif', 'band': 1, 'ignore': [], 'of': ['labels']}),
    ('zones.tif', True, {'zones': 'zones.tif', 'band': 1, 'ignore': [],
                         'of': ['labels', 'change_maps']}),
    ({'zones': '/abs/z.tif'}, False, {'zones': '/abs/z.tif', 'band': 1, 'ignore': [],
                                      'of': ['labels']}),
    ({'zones': 'z.tif', 'band': 3, 'ignore': [9, 0, -4, 9]}, True,
     {'zones': 'z.tif', 'band': 3, 'ignore': [-4, 0, 9], 'of': ['labels', 'change_maps']}),
    ({'zones': 'z.tif', 'of': ['change_maps']}, True,
     {'zones': 'z.tif', 'band': 1, 'ignore': [], 'of': ['change_maps']}),
    ({'zones': 'z.tif', 'of': ['change_maps', 'labels']}, True,
     {'zones': 'z.tif', 'band': 1, 'ignore': [], 'of': ['labels', 'change_maps']}),
    ({'zones': 'z.tif', 'of': ['labels'], 'ignore': []}, False,
     {'zones': 'z.tif', 'band': 1, 'ignore': [], 'of': ['labels']}),
])
def test_accepted_forms(value, maps, want):
    s = {'label_rules': RULES, 'zonal_stats': value}
    if maps:
        s['change_maps'] = [MAP]
    assert check_zonal_stats(s) is s
    assert zonal_stats_options(s) == want
    assert load_settings(s) is s


@pytest.mark.parametrize('value', [
    7, 1.5, True, None, [], ['zones.tif'], '', '  ',
    {}, {'band': 1}, {'zones': ''}, {'zones': 3}, {'zones': None}, {'zones': ['z.tif']},
    {'zones': 'z.tif', 'bands': 1}, {'zones': 'z.tif', 'x': None},
    {'zones': 'z.tif', 'band': 0}, {'zones': 'z.tif', 'band': -1}, {'zones': 'z.tif', 'band': 1.0},
    {'zones': 'z.tif', 'band': True}, {'zones': 'z.tif', 'band': '1'},
    {'zones': 'z.tif', 'band': 65536},
    {'zones': 'z.tif', 'ignore': 9}, {'zones': 'z.tif', 'ignore': [9.0]},
    {'zones': 'z.tif', 'ignore': [True]}, {'zones': 'z.tif', 'ignore': ['9']},
    {'zones': 'z.tif', 'ignore': None}, {'zones': 'z.tif', 'ignore': [2 ** 63]},
    {'zones': 'z.tif', 'of': []}, {'zones': 'z.tif', 'of': 'labels'},
    {'zones': 'z.tif', 'of': ['label']}, {'zones': 'z.tif', 'of': ['labels', 'labels']},
    {'zones': 'z.tif', 'of': [1]}, {'zones': 'z.tif', 'of': None},
])
def test_rejected_forms(value):
    s = {'label_rules': RULES, 'change_maps': [MAP], 'zonal_stats': value}
    with pytest.raises(ValueError, match='zonal_stats'):
        check_zonal_stats(s)
    with pytest.raises(ValueError, match='zonal_stats'):
        zonal_stats_options(s)
    with pytest.raises(ValueError, match='zonal_stats'):
        load_settings(s)


def test_of_change_maps_needs_the_change_maps_key():
    with pytest.raises(ValueError, match='zonal_stats: of names change_maps'):
        check_zonal_stats({'zonal_stats': {'zones': 'z.tif', 'of': ['change_maps']}})


def test_one_name_one_table():
    s = {'label_rules': RULES, 'change_maps': [dict(MAP, name='gd')], 'zonal_stats': 'z.tif'}
    with pytest.raises(ValueError, match="zonal_stats: the name 'gd'"):
        check_zonal_stats(s)
    check_zonal_stats(dict(s, zonal_stats={'zones': 'z.tif', 'of': ['labels']}))


def test_the_key_leaves_the_compiled_settings_alone():
    import ctypes
    import json

    from jobfixture import SETTINGS
    from land_trendr_amd import _abi
    lib = _abi.load_lib()

    def compiled(settings):
        st, n = _abi.LtSettings(), ctypes.c_int32(0)
        err = ctypes.create_string_buffer(512)
        rc = lib.lt_settings_compile(json.dumps(settings).encode(), 1, 0, 2, 0, ctypes.byref(st),
                                     ctypes.byref(n), err, 512)
        return rc, bytes(st), n.value
    plain = compiled(SETTINGS)
    assert plain[0] == 0
    assert compiled(dict(SETTINGS, zonal_stats='zones.tif')) == plain
    assert compiled(dict(SETTINGS, zonal_stats={'zones': 'z.tif', 'band': 2, 'ignore': [0]})) == plain
