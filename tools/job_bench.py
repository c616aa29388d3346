"""Job-level throughput: the whole local job
(land_trendr_amd/job.py: setup -> parse -> analysis -> output) on a Landsat-scene-sized stack,
timed per stage.

The stack is generated on the box, not shipped: the seeded SURVEY §8(d) scene (synth.make_scene,
on the GPU) written as one LZW GeoTIFF per acquisition — two int16 bands (B1, B2 = B1 - index),
GDAL-like ~8 KB strips, north-up georeferencing — named like the reference's LEDAPS keys
(filename2date reads the year and day of year), plus settings.json ('B1 - B2', line_cost 10, one
GD rule: the c2 configuration). The job then runs exactly as `python -m land_trendr_amd.job`
would, on cuda:0, and the script prints one JSON line:
  * per stage: seconds; parse also as decoded band GB/s and Mpx/s;
  * the whole job in Mpx/s (setup + parse + analysis + output);
  * a seeded sample of pixels re-analysed by the CPU oracle from the job's own ingested bands,
    compared with every output plane (the oracle is the checker here, never a producer).

    python tools/job_bench.py --rows 7000 --cols 7000 --years 30 [--trendline] [--check 20000]
                              [--decode {host,device}] [--encode {host,device}]
                              [--sample {host,device}] [--shift N] [--mask PROB]
                              [--mask-eqn EQN | --qa-cloudmask] [--ftv EQN]
                              [--vertex-table [CAP]] [--mmu N] [--change-maps [N]]
                              [--zonal [BLOCK]]

--zonal [BLOCK]: a zone raster of BLOCK x BLOCK-pixel block zones (default 64; int32 ids from 1) is
written beside the stack and settings.json gets zonal_stats, so the output step sums every rule's
(and, with --change-maps, every map's) planes per zone and onset year on the GPU and writes the
'tables/zonal-<name>.csv' files; the line reports the zones, the tables, their pixel totals, the
CSV bytes and the pass's seconds (LocalJob.zonal_s, the zone raster's read and sampling included).

--change-maps [N]: settings.json gets change_maps with the first N (default 8) of eight maps (loss /
gain, several sorts and filters), so every tile's change maps are made on the GPU during the
analysis and the output step clears, sieves (with --mmu), counts and writes the 'change/...' rasters;
the line reports LocalJob.change_stats' totals, the seconds (LocalJob.change_s), the planes' device
bytes and the rasters' number and bytes.

--mmu N: settings.json gets mmu N, so the output step first sieves every rule's matches on the GPU
(patches of fewer than N 8-connected pixels with one onset year lose their match); the line reports
LocalJob.mmu_stats and the pass's seconds.

--vertex-table [CAP] (with or without --trendline): settings.json gets vertex_table true, or the
integer CAP, so every tile's vertices are compacted on the GPU during the analysis and the output
step writes the 'vertices/...' rasters; the line reports their number, their bytes and the table's
device bytes.

--ftv EQN (needs --trendline): settings.json gets ftv_eqns {'ftv': EQN} (e.g. 'B1'), so the output
step also runs the fit-to-vertex pass for that equation and writes its 'ftv/ftv/<date>-<attr>'
rasters; the line reports the pass's seconds (LocalJob.ftv_s).

--mask-eqn EQN: the rasters carry a third band, a QA band that is 0 with the --mask probability
and 1 elsewhere, instead of cloudmask rasters; settings.json gets mask_eqn EQN (e.g. 'B3 != 0') and
the line reports LocalJob.mask_stats and the mask pass's device time. --qa-cloudmask: the same
three-band rasters, but the QA band reaches the job as `_cloudmask` rasters and no mask_eqn is
set: the job the mask_eqn one is compared with.
"""
import argparse
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

GT = (500000.0, 30.0, 0.0, 4200000.0, 0.0, -30.0)
SETTINGS = {'index_eqn': 'B1 - B2', 'line_cost': 10, 'target_date': '2014-07-01',
            'label_rules': [{'name': 'gd', 'val': 1, 'change_type': 'GD'}]}


# --change-maps: loss and gain maps over the sorts and filters (the synthetic index spans about
# -200 .. 900)
CHANGE_MAPS = [
    {'name': 'loss', 'delta': 'loss'},
    {'name': 'gain_new', 'delta': 'gain', 'sort': 'newest', 'mag': ['>', 130]},
    {'name': 'loss_steep', 'delta': 'loss', 'sort': 'steepest', 'dur': ['>', 1],
     'preval': ['>=', 600]},
    {'name': 'loss_big', 'delta': 'loss', 'mag': ['>', 480]},
    {'name': 'gain_long', 'delta': 'gain', 'sort': 'longest', 'dur': ['<', 4]},
    {'name': 'loss_90s', 'delta': 'loss', 'sort': 'oldest', 'year': [1990, 1999]},
    {'name': 'gain_small', 'delta': 'gain', 'sort': 'least', 'mag': ['<=', 26.0]},
    {'name': 'loss_short', 'delta': 'loss', 'sort': 'shortest', 'preval': ['<', 0]}]


def make_stack(root, job, rows, cols, years, seed, mask_prob, shift=0, mask_eqn=None,
               qa_band=False, compress='lzw', tiff_tile=None):
    """The job directory: one two-band int16 LZW GeoTIFF per acquisition date (raster order:
    pixel p of the scene at row p // cols, column p % cols) and, with mask_prob > 0, a cloudmask
    raster per date. shift = N > 0: every N-th raster is written with an extent of its own — its
    origin a few pixels off the template's in both axes, a few rows and columns larger or smaller
    (alternating), zeros outside the scene — and with two spare bands behind the two the index
    reads, as a LEDAPS stack's dates differ. mask_eqn / qa_band: every raster gets a third band
    (0 where the scene's mask is, 1 elsewhere); with mask_eqn the key goes into settings.json and
    no cloudmask raster is written. compress / tiff_tile: write_geotiff's compress and tile of
    the rasters and masks. Returns (seconds, bytes written)."""
    import torch
    from land_trendr_amd.raster import write_geotiff
    from land_trendr_amd.synth import make_scene
    t0 = time.time()
    rdir = os.path.join(root, job, 'input', 'rasters')
    os.makedirs(rdir, exist_ok=True)
    with open(os.path.join(root, job, 'input', 'settings.json'), 'w') as f:
        json.dump(dict(SETTINGS, mask_eqn=mask_eqn) if mask_eqn else SETTINGS, f)
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    sc = make_scene(rows * cols, n_years=years, k_min=1, k_max=1, mask_prob=mask_prob, seed=seed,
                    device=dev, with_bands=True)
    sc.values = None
    nbytes = 0
    for k, d in enumerate(sc.dates):
        stem = 'LT5045029_%d_%03d_20120124_104859' % (d.year, d.timetuple().tm_yday)
        img = sc.bands[k].reshape(2, rows, cols).cpu().numpy()
        if mask_eqn or qa_band:
            qa = (np.ones((1, rows, cols), img.dtype) if sc.valid is None else
                  sc.valid[k].reshape(1, rows, cols).cpu().numpy().astype(img.dtype))
            img = np.concatenate([img, qa])
        fn = os.path.join(rdir, stem + '_ledaps.tif')
        gt = GT
        if shift > 0 and k % shift == shift - 1:
            # raster pixel (y, x) is template pixel (y + sy, x + sx)
            sgn = 1 if (k // shift) % 2 == 0 else -1
            sx, sy, h, w = 3 * sgn, -2 * sgn, rows + 5 * sgn, cols - 4 * sgn
            nb = img.shape[0]
            big = np.zeros((nb + 2, h, w), img.dtype)
            y0, y1, x0, x1 = max(0, -sy), min(h, rows - sy), max(0, -sx), min(w, cols - sx)
            big[:nb, y0:y1, x0:x1] = img[:, y0 + sy:y1 + sy, x0 + sx:x1 + sx]
            big[nb:] = 7
            img = big
            gt = (GT[0] + sx * GT[1], GT[1], 0.0, GT[3] + sy * GT[5], 0.0, GT[5])
        write_geotiff(fn, img, geotransform=gt, nodata=None, compress=compress, tile=tiff_tile)
        nbytes += os.path.getsize(fn)
        if sc.valid is not None and not mask_eqn:
            m = sc.valid[k].reshape(rows, cols).cpu().numpy()
            mf = os.path.join(rdir, stem + '_cloudmask.tif')
            write_geotiff(mf, m, geotransform=GT, nodata=None, compress=compress,
                          tile=tiff_tile)
            nbytes += os.path.getsize(mf)
        if k % 5 == 4:
            print('  %d rasters written (%.0f s)' % (k + 1, time.time() - t0), file=sys.stderr,
                  flush=True)
    del sc
    if dev == 'cuda':
        torch.cuda.empty_cache()
    return time.time() - t0, nbytes


def check_sample(j, n, seed=11):
    """A seeded sample of the job's pixels: the oracle on the job's own ingested bands vs every
    output plane. Returns (pixels, {plane: mismatches}). With settings.json mmu the job's matched
    plane is the sieved one: a match the oracle has and the job has not is then what the sieve
    does (counted as 'sieved'), only a match the oracle has not is a mismatch."""
    from golden_io import _bits_equal
    from land_trendr_amd import _abi
    from land_trendr_amd.ingest import host_threads
    from land_trendr_amd.scene import build_scene, parse_date
    from land_trendr_amd.settings import compile_params
    from oracle import oracle
    st = j.stack
    P = st['n_pix']
    cols_s = np.sort(np.random.default_rng(seed).choice(P, min(P, n), replace=False))
    b = st['bands'][:, :, cols_s]
    idx = (b[:, 0].astype(np.int32) - b[:, 1]).astype(np.int16)
    meta = build_scene(st['dates'], parse_date(SETTINGS['target_date']))
    params, _ = compile_params(SETTINGS['line_cost'], SETTINGS['label_rules'])
    valid = np.ascontiguousarray(st['valid'][:, cols_s])
    if j.settings.get('mask_eqn'):  # the numpy evaluation of the mask on the same samples
        from land_trendr_amd.index_eqn import MaskProgram
        keep = MaskProgram(j.settings['mask_eqn'], b.dtype, st['band_numbers']).evaluate(
            np.moveaxis(b, 1, 0))
        valid = np.where(keep, valid, 0).astype(np.uint8)
    exp = oracle.analyze_tile(meta, params, idx.astype(np.float64), valid,
                              n_threads=host_threads())
    bad = np.flatnonzero(exp['status'] & ~_abi.LT_ST_EMPTY)  # on_error='skip'
    exp['matched'][:, bad] = 0
    mism = {}
    for k, a in j.planes.items():
        a = a[..., cols_s]
        e = exp[k][:a.shape[0]] if a.ndim == 2 else exp[k]
        if k == 'winner':
            e = e.copy()
            e[:, bad] = -1
        if k in ('onset_year', 'duration', 'class_val', 'magnitude', 'initial_val'):
            m = exp['matched'][:a.shape[0]].astype(bool)
            a, e = np.where(m, a, 0), np.where(m, e, 0)
        same = _bits_equal(a, e) if a.dtype.kind == 'f' else (a == e)
        if k == 'matched' and getattr(j, 'mmu_stats', None) is not None:
            sieved = (a == 0) & (e != 0)
            j.mmu_sample_sieved = int(sieved.sum())  # reported beside the line's mmu stats
            same = same | sieved
        mism[k] = int((~same).sum())
    return len(cols_s), mism


def diag(j):
    """Where parse and output spend their time: one input raster opened and decoded on 1 and on
    all host threads; output() run again under cProfile (top entries to stderr)."""
    import cProfile
    import io
    import pstats
    from land_trendr_amd.geotiff import GeoTiff
    from land_trendr_amd.ingest import host_threads
    d = {}
    fn = j.rast_fns[1]
    t0 = time.time()
    g = GeoTiff(fn)
    d['open_s'] = round(time.time() - t0, 3)
    for th in (1, host_threads()):
        t0 = time.time()
        a = g.read(threads=th)
        d['decode_%d_threads_s' % th] = round(time.time() - t0, 3)
        d['decode_%d_threads_gb_per_s' % th] = round(a.nbytes / (time.time() - t0) / 1e9, 3)
    pr = cProfile.Profile()
    t0 = time.time()
    pr.enable()
    j.output()
    pr.disable()
    d['output_again_s'] = round(time.time() - t0, 3)
    buf = io.StringIO()
    pstats.Stats(pr, stream=buf).sort_stats('cumulative').print_stats(25)
    print(buf.getvalue(), file=sys.stderr, flush=True)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=7000)
    ap.add_argument('--cols', type=int, default=7000)
    ap.add_argument('--years', type=int, default=30)
    ap.add_argument('--mask', type=float, default=0.0)
    ap.add_argument('--seed', type=int, default=1000)
    ap.add_argument('--tile', type=int, default=1 << 24, help='job tile pixels')
    ap.add_argument('--trendline', action='store_true',
                    help='also the per-year trendline rasters (8 per acquisition date)')
    ap.add_argument('--check', type=int, default=20000, help='oracle sample (0: none)')
    ap.add_argument('--work', default='/tmp/ltjob_bench')
    ap.add_argument('--keep', action='store_true')
    ap.add_argument('--diag', action='store_true',
                    help='after the job: one raster opened / decoded on 1 and all threads, and a '
                         'cProfile of output() run again (stderr)')
    ap.add_argument('--profile', default=None, choices=('setup', 'parse', 'analyze', 'output'),
                    help='run this step under cProfile (top entries by own time to stderr)')
    ap.add_argument('--decode', default='host', choices=('host', 'device'),
                    help="where the rasters' strips are decoded (LocalJob decode=): liblt_io.so on "
                         'the host threads, or the HIP strip decoder on the GPU')
    ap.add_argument('--sample', default='host', choices=('host', 'device'),
                    help='where rasters of another extent or band count and the cloud masks are '
                         'sampled at the grid points (LocalJob sample=): numpy on the host, or the '
                         'HIP sampling kernel on the GPU (needs --decode device)')
    ap.add_argument('--shift', type=int, default=0,
                    help='N > 0: every N-th raster gets an extent of its own (a few pixels off in '
                         'both axes, a few rows and columns larger or smaller) and two spare bands')
    ap.add_argument('--mask-eqn', default=None,
                    help="settings.json mask_eqn over a QA band B3 (0 with the --mask probability) "
                         "that replaces the cloudmask rasters, e.g. 'B3 != 0'")
    ap.add_argument('--qa-cloudmask', action='store_true',
                    help='the three-band rasters of --mask-eqn, masked through cloudmask rasters '
                         'instead (no mask_eqn): the job to compare with')
    ap.add_argument('--encode', default='host', choices=('host', 'device'),
                    help="where the output rasters' strips are encoded (LocalJob encode=): "
                         'liblt_io.so on the host threads, or the HIP strip encoder on the GPU')
    ap.add_argument('--compress', default='lzw', choices=('lzw', 'deflate'),
                    help='compression of the input rasters and masks')
    ap.add_argument('--tiff-tile', type=int, default=0,
                    help='N > 0: the input rasters and masks are N x N tiled GeoTIFFs (a multiple '
                         'of 16), not strips (--tile is the job\'s tile size in pixels)')
    ap.add_argument('--device-formats', default='strips', choices=('strips', 'all'),
                    help="what --decode device offers the GPU (LocalJob device_formats=): 'strips' "
                         "uncompressed / LZW strip files, 'all' tiles and Deflate as well")
    ap.add_argument('--ftv', default=None,
                    help="settings.json ftv_eqns {'ftv': EQN} (e.g. 'B1'): the fit-to-vertex pass "
                         'of one equation in the output step (needs --trendline)')
    ap.add_argument('--vertex-table', nargs='?', const='true', default=None, metavar='CAP',
                    help="settings.json vertex_table: true, or the integer CAP on a pixel's "
                         'vertices (the vertex table and its vertices/ rasters)')
    ap.add_argument('--mmu', type=int, default=None, metavar='N',
                    help='settings.json mmu: the minimum mapping unit of the label rasters, in '
                         'pixels (the sieve pass of the output step)')
    ap.add_argument('--change-maps', nargs='?', const=8, default=None, type=int, metavar='N',
                    help='settings.json change_maps: the first N of eight maps (the change maps '
                         "and their change/ rasters)")
    ap.add_argument('--zonal', nargs='?', const=64, default=None, type=int, metavar='BLOCK',
                    help='settings.json zonal_stats over BLOCK x BLOCK-pixel block zones (the '
                         'per-zone, per-year tables)')
    ap.add_argument('--reuse', action='store_true',
                    help='use the stack an earlier --keep run left in --work (written with the '
                         'same size and format options) instead of writing it again: runs that '
                         'alternate over one stack')
    a = ap.parse_args()
    import torch
    from land_trendr_amd.ingest import host_threads
    from land_trendr_amd.job import LocalJob
    rdir = os.path.join(a.work, 'bench', 'input', 'rasters')
    reuse = a.reuse and os.path.isdir(rdir)
    if reuse:  # everything but the input goes
        for d in (a.work, os.path.join(a.work, 'bench')):
            for name in os.listdir(d):
                if name not in ('bench', 'input'):
                    q = os.path.join(d, name)
                    shutil.rmtree(q) if os.path.isdir(q) else os.remove(q)
    else:
        shutil.rmtree(a.work, ignore_errors=True)
        os.makedirs(a.work)
    try:
        if reuse:
            gen_s = 0.0
            in_bytes = sum(os.path.getsize(os.path.join(rdir, f)) for f in os.listdir(rdir))
        else:
            gen_s, in_bytes = make_stack(a.work, 'bench', a.rows, a.cols, a.years, a.seed, a.mask,
                                            a.shift, a.mask_eqn, a.qa_cloudmask, a.compress,
                                            (a.tiff_tile, a.tiff_tile) if a.tiff_tile else None)
        print('stack written: %.1f s, %.2f GB' % (gen_s, in_bytes / 1e9), file=sys.stderr,
              flush=True)
        spath = os.path.join(a.work, 'bench', 'input', 'settings.json')
        with open(spath) as f:
            settings = json.load(f)
        settings.pop('ftv_eqns', None)  # (a reused stack's settings may carry an earlier run's)
        if a.ftv:
            if not a.trendline:
                ap.error('--ftv needs --trendline')
            settings['ftv_eqns'] = {'ftv': a.ftv}
        settings.pop('vertex_table', None)
        if a.vertex_table:
            settings['vertex_table'] = True if a.vertex_table == 'true' else int(a.vertex_table)
        settings.pop('mmu', None)
        if a.mmu is not None:
            settings['mmu'] = a.mmu
        settings.pop('change_maps', None)
        if a.change_maps is not None:
            if not 1 <= a.change_maps <= len(CHANGE_MAPS):
                ap.error('--change-maps takes 1 to %d' % len(CHANGE_MAPS))
            settings['change_maps'] = CHANGE_MAPS[:a.change_maps]
        settings.pop('zonal_stats', None)
        if a.zonal is not None:
            if a.zonal < 1:
                ap.error('--zonal takes a block size of at least 1')
            from land_trendr_amd.raster import write_geotiff
            nbw = (a.cols + a.zonal - 1) // a.zonal
            zimg = (1 + (np.arange(a.rows, dtype=np.int32)[:, None] // a.zonal) * nbw +
                    np.arange(a.cols, dtype=np.int32)[None, :] // a.zonal)
            write_geotiff(os.path.join(a.work, 'bench', 'input', 'zones.tif'), zimg,
                          geotransform=GT, nodata=0)
            del zimg
            settings['zonal_stats'] = 'zones.tif'
        with open(spath, 'w') as f:
            json.dump(settings, f)
        P = a.rows * a.cols
        j = LocalJob(a.work, 'bench', device=0, tile_pixels=a.tile, trendline=a.trendline,
                     on_error='skip', decode=a.decode, encode=a.encode, sample=a.sample,
                     **({'device_formats': a.device_formats} if a.device_formats != 'strips'
                        else {}))
        t = {}
        files = None
        for step in ('setup', 'parse', 'analyze', 'output'):
            t0 = time.time()
            if step == a.profile:  # this step under cProfile (top entries to stderr)
                import cProfile
                import io
                import pstats
                pr = cProfile.Profile()
                pr.enable()
                res = getattr(j, step)()
                torch.cuda.synchronize()
                pr.disable()
                buf = io.StringIO()
                pstats.Stats(pr, stream=buf).sort_stats('tottime').print_stats(25)
                print(buf.getvalue(), file=sys.stderr, flush=True)
            else:
                res = getattr(j, step)()
            torch.cuda.synchronize()
            t[step] = time.time() - t0
            if step == 'output':
                files = res
            print('%s %.2f s' % (step, t[step]), file=sys.stderr, flush=True)
        total = sum(t.values())
        K = len(j.stack['dates'])
        nb = len(j.stack['band_numbers'])
        decoded = K * nb * P * 2  # the int16 bands ingested per acquisition (two without a mask_eqn)
        out_bytes = sum(os.path.getsize(p) for v in files.values() for p in v)
        res = {'workload': 'job: %d x %d px x %d acquisitions, 2 int16 bands each (%s GeoTIFF, %s), '
                           "index_eqn 'B1 - B2', line_cost 10, one GD rule%s"
                           % (a.rows, a.cols, K, a.compress.upper() if a.compress == 'lzw'
                              else 'Deflate',
                              '%d x %d tiles' % (a.tiff_tile, a.tiff_tile) if a.tiff_tile
                              else 'strips', ', per-year trendline rasters' if a.trendline
                              else ''),
               'pixels': P, 'acquisitions': K, 'host_threads': host_threads(),
               'input_bytes': in_bytes, 'generate_s': round(gen_s, 2),
               'seconds': {k: round(v, 3) for k, v in t.items()},
               'job_s': round(total, 3), 'job_mpx_per_s': round(P / total / 1e6, 3),
               'parse_decoded_gb_per_s': round(decoded / t['parse'] / 1e9, 3),
               'parse_mpx_per_s': round(P / t['parse'] / 1e6, 2),
               'analyze_mpx_per_s': round(P / t['analyze'] / 1e6, 2),
               'output_rasters': len(files), 'output_bytes': out_bytes,
               'raster_order': j._raster_hw is not None,
               'jit': getattr(j, 'jit_stats', None),
               'analyze_parts_s': {k: round(v, 3) for k, v in getattr(j, 'analyze_s', {}).items()},
               'upload': os.environ.get('LT_JOB_UPLOAD', 'whole'),
               'decode': a.decode, 'decode_stats': j.decode_stats,
               'compress': a.compress, 'tiff_tile': a.tiff_tile,
               'device_formats': a.device_formats, 'sample': a.sample, 'shift': a.shift, 'mask': a.mask,
               'sample_stats': j.sample_stats,
               'encode': a.encode, 'encode_stats': j.encode_stats,
               'decode_times_s': {k: round(v, 3)
                                  for k, v in getattr(j, 'decode_times', {}).items()}}
        if a.mask_eqn or a.qa_cloudmask:
            res['mask_eqn'], res['qa_cloudmask'] = a.mask_eqn, a.qa_cloudmask
            res['mask_stats'] = j.mask_stats
            ms = getattr(j, 'analyze_s', {}).get('mask')
            if ms is not None:
                # the pass reads the planes the expression names and the validity bytes, and
                # writes back the validity vectors in which it cleared a byte (counted in full)
                from land_trendr_amd.index_eqn import MaskProgram
                n_slots = len(MaskProgram(a.mask_eqn, np.int16, j.stack['band_numbers']).slots)
                nbytes = K * P * (2 * n_slots + 2)
                res['mask_pass'] = {'ms': round(ms * 1e3, 4), 'bytes': nbytes,
                                    'tb_per_s': round(nbytes / ms / 1e12, 4)}
        if a.ftv:
            res['ftv_eqn'] = a.ftv
            res['ftv_pass_s'] = {k: round(v, 3) for k, v in j.ftv_s.items()}
        if a.vertex_table:
            vfiles = [p for k, v in files.items() if '/vertices/' in '/' + k for p in v]
            vp = j.vertex_planes
            res['vertex_table'] = {
                'setting': settings['vertex_table'], 'max_vertices': int(vp['vertex_year'].shape[0]),
                'vertices_max': int(vp['n_vertices'].max()),
                'vertices_per_pixel': round(float(vp['n_vertices'].sum()) / P, 3),
                'device_bytes': sum(t.numel() * t.element_size() for t in vp.values()),
                'rasters': len(vfiles), 'raster_bytes': sum(os.path.getsize(p) for p in vfiles)}
        if a.mmu is not None:
            res['mmu'] = {'setting': settings['mmu'], 'stats': j.mmu_stats,
                          'pass_s': round(j.mmu_s, 4)}
        if a.change_maps is not None:
            cfiles = [p for k, v in files.items() if k.startswith('change/') for p in v]
            res['change_maps'] = {
                'maps': a.change_maps, 'pass_s': round(j.change_s, 4),
                'stats': {k: {'matched': v['matched'], 'removed': v['removed']}
                          for k, v in j.change_stats.items()},
                'device_bytes': sum(t.numel() * t.element_size()
                                    for t in j.change_planes.values()),
                'rasters': len(cfiles), 'raster_bytes': sum(os.path.getsize(p) for p in cfiles)}
        if a.zonal is not None:
            zs = j.zonal_stats
            res['zonal_stats'] = {
                'block': a.zonal, 'pass_s': round(j.zonal_s, 4),
                'zones': int(len(next(iter(zs.values()))['zone_ids'])), 'tables': sorted(zs),
                'pixels': {k: int(v['pixels'].sum()) for k, v in zs.items()},
                'outside': {k: int(v['pixels'][-1].sum()) for k, v in zs.items()},
                'csv_bytes': sum(os.path.getsize(p) for p in j.zonal_files.values())}
        if a.diag:
            res['diag'] = diag(j)
        if a.check > 0:
            n, mism = check_sample(j, a.check)
            if a.mmu is not None:
                res['mmu']['sieved_in_check_sample'] = j.mmu_sample_sieved
            res['check'] = {'pixels': n, 'mismatches': mism,
                            'checker': 'oracle/lt_oracle.c on the job\'s ingested bands'}
        print(json.dumps(res), flush=True)
        if a.check > 0 and any(res['check']['mismatches'].values()):
            sys.exit(3)
    finally:
        if not a.keep:
            shutil.rmtree(a.work, ignore_errors=True)


if __name__ == '__main__':
    main()
