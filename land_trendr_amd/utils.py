"""Drop-in counterparts of the reference's hot-path functions (/root/reference/utils.py).

    analyze(pix_datas, line_cost, target_date) -> Trendline        utils.py:735-789
    change_labeling(trendline, label_rules) -> dict                utils.py:795-820
    analysis_reducer(point_wkt, pix_datas, settings) -> generator  mr_land_trendr_job.py:83-126
    analysis_reducer_batch(tile, settings) -> dense rasters        (the batched form of the above)

Same names, arguments, results and exception types as the reference; every number comes from
the HIP kernels of liblt_hip.so (one pixel per lane). The per-pixel functions exist for
drop-in compatibility; throughput comes from the batched tile path (analyze_tile).
"""
import datetime as _dt

import numpy as np
import torch

from . import _abi
from .classes import Disturbance, LabelRule, Trendline, TrendlinePoint
from .engine import ALL_FIELDS, FTV_FIELDS, LABELS, get_engine, label_tile
from .scene import build_scene, parse_date
from .settings import compile_params, load_settings, vertex_cap

__all__ = ['parse_date', 'analyze', 'change_labeling', 'analysis_reducer',
           'analysis_reducer_batch', 'analyze_tile', 'index_tile', 'match_rules_gpu',
           'fit_to_vertices_tile', 'vertex_table', 'disturbances_from_vertices', 'sieve_labels',
           'change_maps', 'label_counts', 'zonal_stats']


def _raise_for_status(status, n_obs_valid):
    """Raise what the reference raises for a pixel (classes.py:207)."""
    if status & _abi.LT_ST_FEB29:
        raise ValueError('day is out of range for month')
    if status & _abi.LT_ST_EMPTY:
        raise IndexError('index 0 is out of bounds for axis 0 with size 0')
    if status & _abi.LT_ST_SINGLE_YEAR:
        raise ValueError('Length of values (2) does not match length of index (1)')
    if status & _abi.LT_ST_NUMERIC:
        raise FloatingPointError('least-squares path outside the emulated LAPACK range')


def analyze_tile(scene, params, values, valid=None, fields=ALL_FIELDS, out=None, device=None):
    """Batched analyze + label of a pixel tile on the GPU (see Engine.analyze_tile)."""
    return get_engine(device).analyze_tile(scene, params, values, valid, fields, out)


def fit_to_vertices_tile(scene, winner, spike, vertex, values, fields=FTV_FIELDS, out=None,
                         device=None):
    """Fit to vertex on the GPU: the winner / spike / vertex planes of an analysis ([Y, P]) and a
    second index's values ([K, P]) -> that index's trendline planes at the same vertices
    (vertices2eqns + eqns2fitted_points, utils.py:646-722; see Engine.ftv_tile)."""
    return get_engine(device).ftv_tile(scene, winner, spike, vertex, values, fields, out)


def vertex_table(years, val_fit, vertex, present=None, winner=None, val_raw=None,
                 max_vertices=None, out=None, device=None):
    """The vertex table on the GPU: per-year planes ([Y, P]) -> one row per vertex per pixel,
    'n_vertices' [P] and 'vertex_year' / 'vertex_fit' / 'vertex_raw' [V, P] (see
    Engine.vertex_table)."""
    return get_engine(device).vertex_table(years, val_fit, vertex, present, winner, val_raw,
                                           max_vertices, out)


def sieve_labels(matched, key, shape, min_pixels, connectivity=8, apply=True, out=None,
                 device=None):
    """The minimum mapping unit on the GPU: a label plane's matched pixels ([P] uint8 over a
    shape = (rows, cols) raster) grouped into patches of one key ([P] int32, or None), 'root' and
    'size' [P] int32 returned, the patches below min_pixels cleared in `matched` (see
    Engine.sieve)."""
    return get_engine(device).sieve(matched, key, shape, min_pixels, connectivity, apply, out)


def change_maps(years, rules, val_fit, vertex, present=None, winner=None, val_raw=None,
                spike=None, device=None):
    """The change maps on the GPU: per-year planes ([Y, P]) and 1 to 8 map rules -> 'matched',
    'onset_year', 'duration', 'magnitude', 'preval', 'rate' [M, P] and, with val_raw and spike,
    'dsnr' [M, P], 'rmse' and 'n_fit' [P] (see Engine.change_maps). numpy arrays in, numpy arrays
    out: the planes go up, the maps come down; device tensors are taken and returned as they
    are."""
    eng = get_engine(device)
    planes = (val_fit, vertex, present, winner, val_raw, spike)
    host = not any(isinstance(t, torch.Tensor) for t in planes)
    if host:
        dts = (np.float64, np.uint8, np.uint8, np.int16, np.float64, np.uint8)
        planes = [None if a is None else
                  torch.from_numpy(np.ascontiguousarray(a, dt)).to(eng.device)
                  for a, dt in zip(planes, dts)]
    out = eng.change_maps(years, rules, *planes)
    return {f: t.cpu().numpy() for f, t in out.items()} if host else out


def label_counts(matched, key, key_lo, n_bins, device=None):
    """A label plane counted per key on the GPU: matched [P] uint8 and key [P] int32 -> int64
    [n_bins + 1] (see Engine.label_counts). numpy arrays in, a numpy array out; device tensors
    are taken and returned as they are."""
    eng = get_engine(device)
    if isinstance(matched, torch.Tensor):
        return eng.label_counts(matched, key, key_lo, n_bins)
    m = torch.from_numpy(np.ascontiguousarray(matched, np.uint8).reshape(-1)).to(eng.device)
    k = torch.from_numpy(np.ascontiguousarray(key, np.int32).reshape(-1)).to(eng.device)
    return eng.label_counts(m, k, key_lo, n_bins).cpu().numpy()


def zonal_stats(matched, zone, key, key_lo, n_bins, n_zones, duration=None, value=None,
                device=None):
    """A label plane summed per zone and key on the GPU: matched [P] uint8, zone and key [P]
    int32 and, optionally, duration [P] int32 and value [P] float64 -> int64 [n_zones + 1,
    n_bins + 1, 4] (see Engine.zonal_stats). numpy arrays in, a numpy array out; device tensors
    are taken and returned as they are."""
    eng = get_engine(device)
    if isinstance(matched, torch.Tensor):
        return eng.zonal_stats(matched, zone, key, key_lo, n_bins, n_zones, duration, value)

    def up(a, dt):
        return None if a is None else torch.from_numpy(
            np.ascontiguousarray(a, dt).reshape(-1)).to(eng.device)
    return eng.zonal_stats(up(matched, np.uint8), up(zone, np.int32), up(key, np.int32), key_lo,
                           n_bins, n_zones, up(duration, np.int32),
                           up(value, np.float64)).cpu().numpy()


def disturbances_from_vertices(table):
    """Trendline.parse_disturbances (classes.py:156-176) from a vertex table, in numpy on the
    host: table holds 'n_vertices' [P], 'vertex_year' and 'vertex_fit' [V, P] (tensors or
    arrays). Returns {'n_segments' [P] int32, 'onset_year', 'duration' [V-1, P] int32,
    'initial_val', 'magnitude' [V-1, P] float64}: segment j of a pixel runs from vertex j to
    vertex j + 1, onset = year[j], duration = year[j+1] - year[j], initial_val = fit[j],
    magnitude = fit[j] - fit[j+1] (the reference's one subtraction, so its bits). Slots from
    n_segments on hold LT_NODATA; a table capped below a pixel's count yields its first V - 1
    segments."""
    def arr(t):
        return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    n = arr(table['n_vertices']).astype(np.int64)
    year, fit = arr(table['vertex_year']), arr(table['vertex_fit'])
    V = year.shape[0]
    n_seg = np.clip(np.minimum(n, V) - 1, 0, None).astype(np.int32)
    live = np.arange(V - 1)[:, None] < n_seg[None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        mag = fit[:-1] - fit[1:]
    nd = _abi.LT_NODATA
    return {'n_segments': n_seg,
            'onset_year': np.where(live, year[:-1], nd).astype(np.int32),
            'duration': np.where(live, year[1:] - year[:-1], nd).astype(np.int32),
            'initial_val': np.where(live, fit[:-1], float(nd)),
            'magnitude': np.where(live, mag, float(nd))}


def analyze(pix_datas, line_cost, target_date):
    """utils.analyze: [{'date': 'YYYY-MM-DD', 'val': v}, ...] -> Trendline."""
    pix_datas = list(pix_datas)
    dates = [parse_date(d['date']) for d in pix_datas]
    vals = [float(d['val']) for d in pix_datas]
    if not vals:  # pick_winners -> [] then despike indexes an empty series (utils.py:569)
        raise IndexError('index 0 is out of bounds for axis 0 with size 0')
    scene = build_scene(dates, target_date)
    eng = get_engine()
    v = torch.tensor(vals, dtype=torch.float64).reshape(len(vals), 1).to(eng.device)
    params, _ = compile_params(line_cost)
    fields = ('winner', 'val_raw', 'val_fit', 'fit_m', 'fit_b', 'right_m', 'right_b', 'spike',
              'vertex', 'status', 'n_years')
    out = eng.analyze_tile(scene, params, v, None, fields)
    host = {k: t.cpu().numpy() for k, t in out.items()}
    _raise_for_status(int(host['status'][0]), len(vals))
    points = []
    y0 = None
    for y in range(scene.n_years):
        w = int(host['winner'][y, 0])
        if w < 0:
            continue
        yr = int(scene.years[y])
        if y0 is None:
            y0 = yr
        points.append(TrendlinePoint(
            val_raw=float(host['val_raw'][y, 0]), val_fit=float(host['val_fit'][y, 0]),
            eqn_fit=(float(host['fit_m'][y, 0]), float(host['fit_b'][y, 0])),
            eqn_right=(float(host['right_m'][y, 0]), float(host['right_b'][y, 0])),
            index_date=dates[w].strftime('%Y-%m-%d'), index_day=yr - y0,
            spike=bool(host['spike'][y, 0]), vertex=bool(host['vertex'][y, 0])))
    return Trendline(points)


def match_rules_gpu(trendline, rules, pre_threshold_mode='reference'):
    """Trendline.match_rule for each rule, on the GPU label stage. -> [Disturbance | None]."""
    rules = [r if isinstance(r, LabelRule) else LabelRule(r) for r in rules]
    params, _ = compile_params(0.0, rules, pre_threshold_mode)
    pts = trendline.points
    eng = get_engine()
    if not pts:
        return [None] * len(rules)
    years = [parse_date(p.index_date).year for p in pts]
    vf = torch.tensor([[float(p.val_fit)] for p in pts], dtype=torch.float64).to(eng.device)
    vx = torch.tensor([[1 if p.vertex else 0] for p in pts], dtype=torch.uint8).to(eng.device)
    out = label_tile(eng, years, params, vf, vx)
    host = {k: t.cpu().numpy() for k, t in out.items()}
    if int(host['status'][0]) & _abi.LT_ST_PRE_THRESHOLD_ATTR:
        raise AttributeError("LabelRule instance has no attribute 'threshold'")
    res = []
    for r in range(len(rules)):
        if not host['matched'][r, 0]:
            res.append(None)
            continue
        res.append(Disturbance(int(host['onset_year'][r, 0]), float(host['initial_val'][r, 0]),
                               float(host['magnitude'][r, 0]), int(host['duration'][r, 0])))
    return res


def change_labeling(pix_trendline, label_rules, pre_threshold_mode='reference'):
    """utils.change_labeling: {rule.name: {class_val, onset_year, magnitude, duration}} for the
    rules the trendline matches."""
    label_rules = list(label_rules)
    matches = match_rules_gpu(pix_trendline, label_rules, pre_threshold_mode)
    labels = {}
    for rule, match in zip(label_rules, matches):
        if match:
            labels[rule.name] = {'class_val': rule.val, 'onset_year': match.onset_year,
                                 'magnitude': match.magnitude, 'duration': match.duration}
    return labels


def analysis_reducer(point_wkt, pix_datas, settings, pre_threshold_mode='reference'):
    """MRLandTrendrJob.analysis_reducer (mr_land_trendr_job.py:83-126) for one grid point:
    yields ('trendline/<date>-<attr>', {...}) for every point, then ('<label>_<field>', {...})."""
    settings = load_settings(settings)
    pix_trendline = analyze(list(pix_datas), settings['line_cost'],
                            parse_date(settings['target_date']))
    for label, val in pix_trendline.mr_label_output().items():
        yield 'trendline/%s' % label, {'pix_ctr_wkt': point_wkt, 'value': val}
    label_rules = [LabelRule(lr) for lr in settings['label_rules']]
    change_labels = change_labeling(pix_trendline, label_rules, pre_threshold_mode)
    for label_name, data in change_labels.items():
        for key in ['class_val', 'onset_year', 'magnitude', 'duration']:
            yield '%s_%s' % (label_name, key), {'pix_ctr_wkt': point_wkt, 'value': data[key]}


def analysis_reducer_batch(dates, values, valid, settings, fields=LABELS + ('status',),
                           pre_threshold_mode='reference', device=None, bands=None,
                           band_numbers=None):
    """Batched analysis_reducer: a co-registered tile (obs `dates`, values [K, P] — float64 or
    an index raster in its stored type — valid [K, P] uint8 or None, on the GPU) -> dict of dense
    output planes (GPU tensors): the label rasters the reference emits per grid point as
    '<label>_<field>' values, and, when requested, the trendline planes
    ('trendline/<date>-<attr>' values, per year slot).

    bands: instead of values, the raw band planes [K, n_bands, P] (their dtype is the raster's);
    settings['index_eqn'] is then evaluated on the GPU first (parse_mapper's rast_algebra,
    mr_land_trendr_job.py:67-68). band_numbers: the reference band number of each plane (default
    1..n_bands). settings['mask_eqn'], if present, is evaluated on the same planes and ANDed into
    a copy of valid (all ones when valid is None): the caller's tensor is not modified.

    settings['ftv_eqns'] ({name: equation}; needs bands): when the trendline planes winner,
    spike and vertex are among `fields`, every equation is evaluated on the bands as index_eqn
    would be and fitted to the analysis's vertices; out['ftv'][name][field] holds its FTV_FIELDS
    planes and its 'status'.

    settings['vertex_table'] (true, or a cap on the vertex slots): out['vertex_table'] holds the
    analysis's vertex table (Engine.vertex_table: n_vertices, vertex_year, vertex_fit,
    vertex_raw), and out['ftv'][name]['vertex_table'] each equation's: its val_fit / val_raw at
    the analysis's vertices. The planes the table is made from are analysed even if `fields`
    does not name them; only the fields asked for are returned."""
    settings = load_settings(settings)
    scene = build_scene(dates, parse_date(settings['target_date']))
    params, rules = compile_params(settings['line_cost'], settings.get('label_rules', ()),
                                   pre_threshold_mode)
    if bands is not None:
        if settings.get('mask_eqn'):
            valid = mask_tile(settings['mask_eqn'], bands, valid, band_numbers, device=device)
        values = index_tile(settings['index_eqn'], bands, band_numbers, device=device)
    V = vertex_cap(settings, scene.n_years)
    asked = tuple(fields)
    if V is not None:
        fields = asked + tuple(f for f in ('winner', 'val_raw', 'val_fit', 'vertex')
                               if f not in asked)
    out = analyze_tile(scene, params, values, valid, fields, device=device)
    if settings.get('ftv_eqns') and all(f in asked for f in ('winner', 'spike', 'vertex')):
        if bands is None:
            raise ValueError('ftv_eqns needs the band planes (bands=...)')
        out['ftv'] = {
            name: fit_to_vertices_tile(scene, out['winner'], out['spike'], out['vertex'],
                                       index_tile(eqn, bands, band_numbers, device=device),
                                       device=device)
            for name, eqn in settings['ftv_eqns'].items()}
    if V is not None:
        years = scene.years
        out['vertex_table'] = vertex_table(years, out['val_fit'], out['vertex'],
                                           winner=out['winner'], val_raw=out['val_raw'],
                                           max_vertices=V, device=device)
        for f in out.get('ftv', {}).values():
            f['vertex_table'] = vertex_table(years, f['val_fit'], out['vertex'],
                                             winner=out['winner'], val_raw=f['val_raw'],
                                             max_vertices=V, device=device)
        for f in set(fields) - set(asked):
            del out[f]
    out['_scene'] = scene
    out['_rules'] = rules
    return out


def mask_tile(mask_eqn, bands, valid=None, band_numbers=None, device=None):
    """rast_algebra's mask_eqn on the GPU: bands [K, n_bands, P] -> a new validity plane [K, P]
    uint8, `valid` (ones when None) cleared where the expression is false."""
    import torch
    from .index_eqn import MaskProgram
    eng = get_engine(device)
    K, nb, P = bands.shape
    numbers = list(band_numbers) if band_numbers is not None else list(range(1, nb + 1))
    prog = MaskProgram(mask_eqn, np.dtype(str(bands.dtype).replace('torch.', '')), numbers,
                       raster_count=max(numbers))
    if valid is None:
        out = torch.ones((K, P), dtype=torch.uint8, device=bands.device)
    else:
        out = valid.clone(memory_format=torch.contiguous_format)
    return eng.apply_mask(eng.compile_mask(prog), bands, out)


def index_tile(index_eqn, bands, band_numbers=None, device=None):
    """rast_algebra (utils.py:447-484) on the GPU: bands [K, n_bands, P] (the raster's dtype) ->
    the index raster [K, P] in the same dtype (array2raster's template type, utils.py:396-397)."""
    from .index_eqn import IndexProgram
    eng = get_engine(device)
    nb = bands.shape[1]
    numbers = list(band_numbers) if band_numbers is not None else list(range(1, nb + 1))
    prog = IndexProgram(index_eqn, band_dtype=np.dtype(str(bands.dtype).replace('torch.', '')),
                        raster_count=max(numbers))
    slots = [numbers.index(b) for b in prog.bands]  # the planes the equation reads, in order
    sel = bands[:, slots, :] if slots != list(range(nb)) else bands
    return eng.index_tile(eng.compile_index(prog), sel.contiguous() if sel.stride(2) != 1 else sel)
