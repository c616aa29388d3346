"""settings.json semantics (README.md:46-85 of the reference) → the C ABI's lt_params.

Only the analysis keys matter on this path: index_eqn, line_cost, target_date, label_rules.
NODATA mirrors /root/reference/settings.py:16. The S3 bucket / key templates of that file belong
to the storage layer, which is out of scope.
"""
import json
import re

from . import _abi
from .classes import LabelRule

NODATA = _abi.LT_NODATA


def compile_params(line_cost, label_rules=(), pre_threshold_mode='reference'):
    """line_cost + LabelRule list (or settings dicts) → LtParams.

    pre_threshold_mode 'reference' reproduces classes.py:207 (any pre_threshold filter raises
    AttributeError); 'documented' applies the filter the docstring describes (classes.py:26-29).
    """
    rules = [r if isinstance(r, LabelRule) else LabelRule(r) for r in label_rules]
    if len(rules) > _abi.LT_MAX_RULES:
        raise ValueError('at most %d label rules' % _abi.LT_MAX_RULES)
    if pre_threshold_mode not in ('reference', 'documented'):
        raise ValueError('pre_threshold_mode must be "reference" or "documented"')
    p = _abi.LtParams()
    p.line_cost = float(line_cost)
    p.n_rules = len(rules)
    p.pre_threshold_mode = (_abi.LT_PRE_REFERENCE if pre_threshold_mode == 'reference'
                            else _abi.LT_PRE_DOCUMENTED)
    for i, r in enumerate(rules):
        p.rules[i] = r.to_c()
    return p, rules


_FTV_NAME = re.compile(r'[A-Za-z0-9_]+\Z')


def check_ftv_eqns(settings):
    """settings['ftv_eqns'], if present: an object mapping a name ([A-Za-z0-9_]+: it becomes the
    'ftv/<name>/' part of the output keys) to an equation string, which means what index_eqn
    would mean. Anything else is a ValueError; an absent key changes nothing."""
    if 'ftv_eqns' not in settings:
        return settings
    eqns = settings['ftv_eqns']
    if not isinstance(eqns, dict):
        raise ValueError('ftv_eqns must be an object mapping names to equations')
    for name, eqn in eqns.items():
        if not isinstance(name, str) or not _FTV_NAME.match(name):
            raise ValueError('ftv_eqns name %r must match [A-Za-z0-9_]+' % (name,))
        if not isinstance(eqn, str) or not eqn.strip():
            raise ValueError('ftv_eqns[%r] must be an equation string' % (name,))
    return settings


def check_vertex_table(settings):
    """settings['vertex_table'], if present: true (a vertex table with as many vertex slots as the
    scene has years) or an integer cap on the slots in [2, LT_MAX_YEARS]. Anything else (false,
    a float, a string, a cap outside the range) is a ValueError; an absent key changes nothing."""
    if 'vertex_table' not in settings:
        return settings
    v = settings['vertex_table']
    if v is True:
        return settings
    if isinstance(v, bool) or not isinstance(v, int) or not 2 <= v <= _abi.LT_MAX_YEARS:
        raise ValueError('vertex_table must be true or an integer in [2, %d], not %r'
                         % (_abi.LT_MAX_YEARS, v))
    return settings


def vertex_cap(settings, n_years):
    """The vertex slots V of a scene with n_years year slots under settings['vertex_table'] (a
    pixel has at most n_years vertices, so a larger cap adds nothing), or None if the key is
    absent."""
    if 'vertex_table' not in check_vertex_table(settings):
        return None
    v = settings['vertex_table']
    return max(n_years, 1) if v is True else min(v, max(n_years, 1))


_MMU_KEYS = ('min_pixels', 'connectivity', 'by')


def check_mmu(settings):
    """settings['mmu'], if present: the minimum mapping unit of the label rasters. An integer N
    is short for {"min_pixels": N}; the long form is {"min_pixels": N, "connectivity": 4 | 8,
    "by": "onset_year" | "match"} with connectivity 8 and by "onset_year" when left out.
    min_pixels is an integer in [1, 2^31 - 1] (1 changes nothing). Anything else (a bool, a float,
    a string, an unknown sub-key, a missing min_pixels) is a ValueError; an absent key changes
    nothing."""
    if 'mmu' not in settings:
        return settings
    v = settings['mmu']
    long_form = isinstance(v, dict)
    if long_form:
        unknown = sorted(set(v) - set(_MMU_KEYS), key=str)
        if unknown:
            raise ValueError('mmu has unknown keys %r (known: %s)' % (unknown, ', '.join(_MMU_KEYS)))
        if 'min_pixels' not in v:
            raise ValueError('mmu needs min_pixels')
        n = v['min_pixels']
    else:
        n = v
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 2 ** 31 - 1:
        raise ValueError('mmu min_pixels must be an integer in [1, 2^31 - 1], not %r' % (n,))
    if long_form:
        c = v.get('connectivity', 8)
        if isinstance(c, bool) or not isinstance(c, int) or c not in (4, 8):
            raise ValueError('mmu connectivity must be 4 or 8, not %r' % (c,))
        if v.get('by', 'onset_year') not in ('onset_year', 'match'):
            raise ValueError('mmu by must be "onset_year" or "match", not %r' % (v['by'],))
    return settings


def mmu_options(settings):
    """settings['mmu'] in full, {'min_pixels', 'connectivity', 'by'} with the defaults filled in,
    or None if the key is absent."""
    if 'mmu' not in check_mmu(settings):
        return None
    v = settings['mmu']
    if not isinstance(v, dict):
        v = {'min_pixels': v}
    return {'min_pixels': v['min_pixels'], 'connectivity': v.get('connectivity', 8),
            'by': v.get('by', 'onset_year')}


CHANGE_DELTAS = ('loss', 'gain')
CHANGE_SORTS = ('greatest', 'least', 'newest', 'oldest', 'longest', 'shortest', 'steepest',
                'gentlest')
CHANGE_OPS = ('>', '<', '>=', '<=')
_CHANGE_KEYS = ('name', 'delta', 'sort', 'index_sign', 'year', 'mag', 'dur', 'preval', 'mmu')
MAX_CHANGE_MAPS = 8  # LT_MAX_CHANGE_MAPS


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def check_change_maps(settings):
    """settings['change_maps'], if present: a list of 1 to 8 objects, one change map each, with
    the keys
      name        [A-Za-z0-9_]+, unique: the 'change/<name>-...' part of the output keys (required)
      delta       "loss" or "gain" (required)
      sort        "greatest" (default), "least", "newest", "oldest", "longest", "shortest",
                  "steepest" or "gentlest": which of a pixel's kept segments the map shows
      index_sign  1 (default: a loss is a fall of the index) or -1 (a loss is a rise)
      year        [lo, hi], integers with lo <= hi: lo <= onset_year <= hi
      mag, dur, preval   [op, v]: op one of ">", "<", ">=", "<=", v a number, on the segment's
                  magnitude, duration and value before the change
      mmu         the forms check_mmu accepts: the map's own sieve (else the top-level mmu's)
    Anything else (an unknown key, a bool for a number, a float for a year, lo > hi, a ninth map,
    a duplicate name, an empty list) is a ValueError that names change_maps; an absent key changes
    nothing."""
    if 'change_maps' not in settings:
        return settings
    maps = settings['change_maps']

    def bad(msg):
        return ValueError('change_maps: ' + msg)
    if not isinstance(maps, list) or not 1 <= len(maps) <= MAX_CHANGE_MAPS:
        raise bad('must be a list of 1 to %d objects' % MAX_CHANGE_MAPS)
    seen = set()
    for i, m in enumerate(maps):
        if not isinstance(m, dict):
            raise bad('entry %d must be an object' % i)
        unknown = sorted(set(m) - set(_CHANGE_KEYS), key=str)
        if unknown:
            raise bad('entry %d has unknown keys %r (known: %s)'
                      % (i, unknown, ', '.join(_CHANGE_KEYS)))
        name = m.get('name')
        if not isinstance(name, str) or not _FTV_NAME.match(name):
            raise bad('entry %d needs a name that matches [A-Za-z0-9_]+, not %r' % (i, name))
        if name in seen:
            raise bad('the name %r is used twice' % name)
        seen.add(name)
        if m.get('delta') not in CHANGE_DELTAS or not isinstance(m.get('delta'), str):
            raise bad('%s: delta must be "loss" or "gain", not %r' % (name, m.get('delta')))
        s = m.get('sort', 'greatest')
        if not isinstance(s, str) or s not in CHANGE_SORTS:
            raise bad('%s: sort must be one of %s, not %r' % (name, ', '.join(CHANGE_SORTS), s))
        sign = m.get('index_sign', 1)
        if not _is_int(sign) or sign not in (1, -1):
            raise bad('%s: index_sign must be 1 or -1, not %r' % (name, sign))
        if 'year' in m:
            y = m['year']
            if (not isinstance(y, list) or len(y) != 2 or not all(_is_int(v) for v in y) or
                    not all(-2 ** 31 <= v <= 2 ** 31 - 1 for v in y) or y[0] > y[1]):
                raise bad('%s: year must be [lo, hi], integers with lo <= hi, not %r' % (name, y))
        for key in ('mag', 'dur', 'preval'):
            if key in m:
                f = m[key]
                if (not isinstance(f, list) or len(f) != 2 or not isinstance(f[0], str) or
                        f[0] not in CHANGE_OPS or not _is_number(f[1])):
                    raise bad('%s: %s must be [op, number] with op one of %s, not %r'
                              % (name, key, ' '.join(CHANGE_OPS), f))
        if 'mmu' in m:
            try:
                check_mmu({'mmu': m['mmu']})
            except ValueError as e:
                raise bad('%s: %s' % (name, e))
    return settings


def change_map_options(settings):
    """settings['change_maps'] in full: the list of maps, each {'name', 'delta', 'sort',
    'index_sign', 'year' ([lo, hi] or None), 'mag', 'dur', 'preval' ([op, v] or None), 'mmu'
    (mmu_options' dict or None)} with the defaults filled in, or None if the key is absent. A
    map's own mmu wins; without one the top-level mmu applies to the map as well; neither means
    no sieve."""
    if 'change_maps' not in check_change_maps(settings):
        return None
    top = mmu_options(settings)
    out = []
    for m in settings['change_maps']:
        out.append({'name': m['name'], 'delta': m['delta'], 'sort': m.get('sort', 'greatest'),
                    'index_sign': m.get('index_sign', 1),
                    'year': list(m['year']) if 'year' in m else None,
                    'mag': list(m['mag']) if 'mag' in m else None,
                    'dur': list(m['dur']) if 'dur' in m else None,
                    'preval': list(m['preval']) if 'preval' in m else None,
                    'mmu': mmu_options({'mmu': m['mmu']}) if 'mmu' in m else
                    (dict(top) if top is not None else None)})
    return out


_ZONAL_KEYS = ('zones', 'band', 'ignore', 'of')
ZONAL_OF = ('labels', 'change_maps')


def check_zonal_stats(settings):
    """settings['zonal_stats'], if present: the per-zone, per-onset-year tables of the label rules
    and the change maps. A string is short for {"zones": that string}; the long form is
      zones   a GeoTIFF of integer zone ids: a file name under <root>/<job>/input/, or an absolute
              path (required, non-empty)
      band    the band that holds the ids, an integer >= 1 (default 1)
      ignore  a list of integer zone ids to leave out (default none; the raster's own GDAL_NODATA
              value is always left out)
      of      a non-empty list out of "labels" and "change_maps", no entry twice: whose tables are
              made (default: both where present); "change_maps" needs the change_maps key
    Anything else (a number, a bool, an empty name, an unknown sub-key, a float id, a band below 1)
    is a ValueError that names zonal_stats; an absent key changes nothing."""
    if 'zonal_stats' not in settings:
        return settings
    v = settings['zonal_stats']

    def bad(msg):
        return ValueError('zonal_stats: ' + msg)
    if isinstance(v, str):
        v = {'zones': v}
    if not isinstance(v, dict):
        raise bad('must be a file name or an object, not %r' % (v,))
    unknown = sorted(set(v) - set(_ZONAL_KEYS), key=str)
    if unknown:
        raise bad('unknown keys %r (known: %s)' % (unknown, ', '.join(_ZONAL_KEYS)))
    z = v.get('zones')
    if not isinstance(z, str) or not z.strip():
        raise bad('zones must be a file name, not %r' % (z,))
    b = v.get('band', 1)
    if not _is_int(b) or not 1 <= b <= 65535:
        raise bad('band must be an integer in [1, 65535], not %r' % (b,))
    ig = v.get('ignore', [])
    if not isinstance(ig, list) or not all(_is_int(i) and -2 ** 63 <= i < 2 ** 63 for i in ig):
        raise bad('ignore must be a list of integer zone ids, not %r' % (ig,))
    if 'of' in v:
        of = v['of']
        if (not isinstance(of, list) or not of or
                not all(isinstance(o, str) and o in ZONAL_OF for o in of) or
                len(set(of)) != len(of)):
            raise bad('of must be a non-empty list out of %s, not %r'
                      % (', '.join('"%s"' % o for o in ZONAL_OF), of))
        if 'change_maps' in of and 'change_maps' not in settings:
            raise bad('of names change_maps, which this settings.json does not have')
    # a table is named after its label rule or change map ('zonal-<name>.csv'): one name, one table
    rules = [r.get('name') for r in settings.get('label_rules') or () if isinstance(r, dict)]
    maps = [m.get('name') for m in settings.get('change_maps') or () if isinstance(m, dict)]
    both = sorted(n for n in set(rules) & set(maps) if isinstance(n, str))
    if both and set(v.get('of', ZONAL_OF)) == set(ZONAL_OF):
        raise bad('the name %r is a label rule and a change map' % both[0])
    return settings


def zonal_stats_options(settings):
    """settings['zonal_stats'] in full, {'zones', 'band', 'ignore' (sorted, distinct), 'of' (in
    ZONAL_OF's order)} with the defaults filled in, or None if the key is absent. Without "of",
    'of' is "labels" and, where the settings have change_maps, "change_maps"."""
    if 'zonal_stats' not in check_zonal_stats(settings):
        return None
    v = settings['zonal_stats']
    if isinstance(v, str):
        v = {'zones': v}
    of = v.get('of', [o for o in ZONAL_OF if o == 'labels' or 'change_maps' in settings])
    return {'zones': v['zones'], 'band': v.get('band', 1),
            'ignore': sorted(set(v.get('ignore', []))), 'of': [o for o in ZONAL_OF if o in of]}


def _check_added(settings):
    return check_zonal_stats(
        check_change_maps(check_mmu(check_vertex_table(check_ftv_eqns(settings)))))


def load_settings(path_or_dict):
    """Read a settings.json (path, JSON text or dict) the way get_settings does (utils.py:241).
    The keys the reference does not have, ftv_eqns, vertex_table, mmu, change_maps and
    zonal_stats, are validated here (check_ftv_eqns, check_vertex_table, check_mmu,
    check_change_maps, check_zonal_stats)."""
    if isinstance(path_or_dict, dict):
        return _check_added(path_or_dict)
    if path_or_dict.lstrip().startswith('{'):
        return _check_added(json.loads(path_or_dict))
    with open(path_or_dict) as fh:
        return _check_added(json.load(fh))
