"""Local job orchestration: MRLandTrendrJob.steps (mr_land_trendr_job.py:154-159)
without mrjob, EMR or S3, over a job directory laid out like the reference's S3 keys
(settings.py:19-25):

    <root>/<job>/input/settings.json             IN_SETTINGS
    <root>/<job>/input/rasters/<...ledaps...>    IN_RASTS (analysis rasters: .tif, .tif.tar.gz, .zip)
    <root>/<job>/input/rasters/<...cloudmask...> optional masks, same name with the trigger swapped
    <root>/<job>/output/pix_grid.csv             OUT_GRID
    <root>/<job>/output/rasters/<key>.tif        OUT_RAST_KEYNAME

Steps, as the reference chains them:
  1. setup    (setup_mapper :20-45)   analysis rasters by RAST_TRIGGER, grid from the first one;
  2. parse    (parse_mapper :47-81)   ingest.ingest_stack: band samples + mask validity per grid
                                      point (index_eqn runs on the GPU in step 3, and so does
                                      the optional settings.json mask_eqn, a boolean expression
                                      over the same bands that drops observations as a mask
                                      raster does: its bands are ingested with index_eqn's);
  3. analysis (analysis_reducer :83-126) the mosaic path of runner.py over pixel tiles on the GPU
                                      (tiles round-robin over the torchrun ranks; the label planes
                                      go to rank 0 over RCCL, the per-year trendline planes stream
                                      to host memory per tile — a file-backed map shared by the
                                      ranks when there are several — never to one GPU);
  4. output   (output_reducer :128-152) raster.label_rasters / trendline_rasters placed by each
                                      grid point's template offsets, written as GeoTIFFs; with
                                      settings.json ftv_eqns ({name: equation}; fit to vertex) also
                                      'ftv/<name>/<date>-<attr>': each equation evaluated as
                                      index_eqn would be and fitted at the analysis's vertices, one
                                      pass per equation, one tile on the GPU at a time (one rank,
                                      trendline=True); with settings.json vertex_table (true or
                                      a cap on the vertices) also 'vertices/n_vertices' and
                                      'vertices/<kk>-year', '<kk>-val_fit', '<kk>-val_raw': each
                                      pixel's vertices, compacted on the GPU per tile (one rank;
                                      trendline=True or False), and 'ftv/<name>/vertices/...' for
                                      every fit-to-vertex equation.

With settings.json mmu (N, or {"min_pixels": N, "connectivity": 4 | 8, "by": "onset_year" |
"match"}) output() first sieves every rule's matches on the GPU (one rank, raster order): patches
of fewer than N connected pixels with one onset year lose their match, so every label raster of
the rule shows NODATA there; the trendline, vertex-table and FTV rasters stay as they are.

With settings.json change_maps (1 to 8 maps: loss or gain, a sort, filters; settings.check_change_maps)
each tile's change maps are evaluated on the GPU during the analysis (one rank; trendline True or
False) into scene-wide device planes; output() clears the dropped pixels' matches, sieves each map
that has an mmu (its own, else the top-level one), counts the pixels per onset year
(LocalJob.change_stats) and writes 'change/<name>-onset_year', '-duration', '-magnitude', '-preval',
'-rate', '-dsnr' for every map with a match, and 'change/rmse'.

With settings.json zonal_stats (a zone raster of integer ids; settings.check_zonal_stats) output()
sums every label rule's and every change map's published planes per zone and onset year on the GPU
(one rank; Engine.zonal_stats) into LocalJob.zonal_stats and 'output/tables/zonal-<name>.csv':
pixels, area, mean magnitude and mean duration per cell. No raster is written or changed.

Multi-rank jobs: rank 0 alone extracts the compressed rasters and writes the grid, then every rank
reads them (a barrier between), so no rank sees a partial extraction or a truncated grid.

Errors follow the reference: a pixel the reference's analysis raises for fails the job with the
same exception type (on_error='raise'); on_error='skip' leaves such pixels NODATA instead.
Grid points with no observation at all never reach the reference's reducer; they stay NODATA.

CLI: python -m land_trendr_amd.job --root DIR --job NAME [--tile-pixels N] [--no-trendline]
     (multi-GPU: torchrun --nproc-per-node N -m land_trendr_amd.job ...)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

from . import _abi
from .geotiff import GeoTiff
from .ingest import (analysis_rasters, grid_axes, grid_coords, grid_offsets, ingest_stack,
                     mask_name, rast2grid, rast_local, read_grid, stack_offset, stack_range)

IN_SETTINGS = '%s/input/settings.json'
IN_RASTS = '%s/input/rasters/'
OUT_GRID = '%s/output/pix_grid.csv'
OUT_RASTS = '%s/output/rasters/'


def zonal_csv(res):
    """One entry of LocalJob.zonal_stats as the text of its 'tables/zonal-<name>.csv': a header,
    then one line per (zone id, onset year) cell with a pixel in it, zones ascending (the row
    outside every zone last, its id 'outside'), years ascending (the column of the onset years
    outside the scene's last, its year 'other'): zone,year,pixels,area,mean_magnitude,
    mean_duration. The numbers are Python's shortest round-trip forms; a cell without a magnitude
    that is not NaN has an empty mean_magnitude."""
    t = res['table']
    rows = [str(int(z)) for z in res['zone_ids']] + ['outside']
    cols = [str(int(y)) for y in res['years']] + ['other']
    lines = ['zone,year,pixels,area,mean_magnitude,mean_duration']
    for r, c in zip(*np.nonzero(t[..., 0])):
        n, dur, q, nv = (int(v) for v in t[r, c])
        lines.append('%s,%s,%d,%r,%s,%r' % (rows[r], cols[c], n, float(n * res['pixel_area']),
                                            repr(q / 16.0 / nv) if nv else '', dur / n))
    return '\n'.join(lines) + '\n'


class _LazyBands(dict):
    """An ingest_stack result whose 'bands' array is completed on first access (LocalJob
    decode='device': the planes of the rasters decoded on the GPU come down from the device
    stack then; the job itself never asks), and, with fill_valid, its 'valid' array the same way
    (sample='device': the validity rows of the rasters sampled on the GPU)."""

    def __init__(self, stack, fill, fill_valid=None):
        super().__init__(stack)
        self._fill = fill
        self._fill_valid = fill_valid

    def _complete(self, key=None):
        if key in (None, 'bands'):
            fill, self._fill = self._fill, None
            if fill is not None:
                fill(dict.__getitem__(self, 'bands'))
        if key in (None, 'valid'):
            fill, self._fill_valid = self._fill_valid, None
            if fill is not None:
                fill(dict.__getitem__(self, 'valid'))

    def __getitem__(self, key):
        if key in ('bands', 'valid'):
            self._complete(key)
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        if key in ('bands', 'valid'):
            self._complete(key)
        return dict.get(self, key, default)

    def items(self):
        self._complete()
        return dict.items(self)

    def values(self):
        self._complete()
        return dict.values(self)


class LocalJob:
    def __init__(self, root, job, device=None, tile_pixels=1 << 22, trendline=True,
                 raster_mode='reference', pre_threshold_mode='reference', on_error='raise',
                 work_dir=None, engine=None, decode=None, encode=None, sample=None,
                 device_formats=None):
        """engine: the analysis engine (default: engine.get_engine of `device`, the HIP library);
        tests pass a CPU double (tests/engine_double.py) to run the multi-rank path over gloo.
        decode: 'host' (default; LT_JOB_DECODE overrides the default) — every raster's strips are
        decoded by liblt_io.so on the host threads; 'device' — parse() builds the device stack up
        front and the rasters the HIP strip decoder takes (GeoTiff.device_eligible, read in
        place: raster order, every band) are decoded on the GPU straight into it, the others on
        the host as before; decode_stats counts both.
        encode: 'host' (default; LT_JOB_ENCODE overrides the default) — output() encodes every
        raster's strips with liblt_io.so on the host threads; 'device' — where output() assembles
        the rasters on the GPU, the HIP strip encoder (Engine.encode_strips) encodes each assembled
        batch there and only the strips come down; elsewhere (a CPU engine, host assembly) the
        host encoder as before; encode_stats counts the rasters by path.
        sample: 'host' (default; LT_JOB_SAMPLE overrides the default) — every raster that is not
        the stack's planes as they are (another extent, spare bands, a rank's tiles of a
        multi-rank job) and every cloud mask is gathered at the grid points on the host
        (ingest.ingest_stack); 'device' (needs decode='device') — in raster order, a raster the
        strip decoder takes is decoded into a scratch raster on the GPU and sampled there
        (Engine.sample_grid) into its plane and validity row of the device stack, whatever its
        extent and band count, and so is its mask (strip-organised, integer samples); the others
        as with 'host'; sample_stats counts the rasters sampled on the device and the masks by
        path.
        device_formats: 'strips' (default; LT_JOB_DEVICE_FORMATS overrides the default) — the
        device decoder is offered the strip-organised uncompressed and LZW files
        (GeoTiff.device_eligible), as before; 'all' (needs decode='device') — every file the HIP
        chunk decoder takes (GeoTiff.device_chunks_eligible: tiles and Deflate as well, through
        GeoTiff.read_device_chunks), in the in-place decode and, with sample='device', for the
        sampled rasters and their masks; decode_stats and sample_stats count as before. As
        measured (DESIGN.md § Tiles and Deflate decoded on the GPU) 'all' pays for Deflate strip
        files only: tiled files decode several times slower on the device than on the host, and
        'all' sends them there all the same."""
        if on_error not in ('raise', 'skip'):
            raise ValueError('on_error must be "raise" or "skip"')
        decode = decode or os.environ.get('LT_JOB_DECODE') or 'host'
        if decode not in ('host', 'device'):
            raise ValueError('decode must be "host" or "device"')
        self.decode = decode
        self.decode_stats = {'device': 0, 'host': 0}  # rasters by the path that decoded them
        encode = encode or os.environ.get('LT_JOB_ENCODE') or 'host'
        if encode not in ('host', 'device'):
            raise ValueError('encode must be "host" or "device"')
        self.encode = encode
        self.encode_stats = {'device': 0, 'host': 0}  # rasters by the path that encoded them
        sample = sample or os.environ.get('LT_JOB_SAMPLE') or 'host'
        if sample not in ('host', 'device'):
            raise ValueError('sample must be "host" or "device"')
        if sample == 'device' and decode != 'device':
            raise ValueError('sample="device" needs decode="device"')
        self.sample = sample
        device_formats = device_formats or os.environ.get('LT_JOB_DEVICE_FORMATS') or 'strips'
        if device_formats not in ('strips', 'all'):
            raise ValueError('device_formats must be "strips" or "all"')
        if device_formats == 'all' and decode != 'device':
            raise ValueError('device_formats="all" needs decode="device"')
        self.device_formats = device_formats
        # rasters sampled on the device (Engine.sample_grid), cloud masks by where they were applied
        self.sample_stats = {'rasters': 0, 'masks_device': 0, 'masks_host': 0}
        # settings.json mask_eqn: {'eqn', 'observations' (valid observation-pixels of this rank's
        # tiles before the mask), 'dropped' (those the mask cleared)} once analyze() has run; None
        # without the key. stack['valid'] keeps the ingest validity (coverage and cloud masks): the
        # mask is ANDed into the planes the analysis reads, not into the stack
        self.mask_stats = None
        self.decode_times = {}  # device mode: thread-seconds of parse() inside the decoder
        self._stack_meta = None  # device mode: (sample type, [K, nb, Q]) of the device stack
        self._dev_keep = None    # device mode: the device stack behind stack['bands']
        self._dev_keep_valid = None  # sample='device': its validity plane behind stack['valid']
        self.root, self.job, self.device = root, job, device
        self.tile_pixels = int(tile_pixels)
        self.trendline = trendline
        self.raster_mode = raster_mode
        self.pre_threshold_mode = pre_threshold_mode
        self.on_error = on_error
        self.work_dir = work_dir or os.path.join(root, job, 'work')
        self.settings_path = os.path.join(root, IN_SETTINGS % job)
        self._grid_fn = os.path.join(root, OUT_GRID % job)
        self._grid_writer = None  # (thread, [exception]) writing the grid CSV beside parse()
        self.out_dir = os.path.join(root, OUT_RASTS % job)
        self.engine = engine
        self._host = None
        self.host_trendline = None
        self._order = None       # grid point of each internal pixel (None: grid order)
        self._raster_hw = None   # (rows, cols) of the raster order, or None
        self.raster_grid = None  # (geotransform, rows, cols) of the raster order, or None
        self._grid_axes = None   # (x of each grid column, y of each grid row) of the raster order
        # settings.json ftv_eqns (fit to vertex): {name: seconds of its pass} once output() ran
        self.ftv_s = {}
        # settings.json vertex_table: the scene-wide vertex table on the analysis's device
        # ({'n_vertices' [P], 'vertex_year' / 'vertex_fit' / 'vertex_raw' [V, P]}: 20 V + 4 bytes
        # a pixel, kept there like the label planes) once analyze() has run; None without the key
        self.vertex_planes = None
        self._ftv_vertex = None  # the same for the fit-to-vertex equation output() is writing
        # settings.json mmu: {rule name: {'matched': pixels matched before the sieve, 'removed':
        # pixels it cleared}} once output() ran; None without the key
        self.mmu_stats = None
        self.mmu_s = 0.0  # seconds of the sieve pass in output(), its count read-back included
        # settings.json change_maps: the scene-wide change-map planes on the analysis's device
        # ({'matched', 'onset_year', 'duration', 'magnitude', 'preval', 'rate', 'dsnr' [M, P],
        # 'rmse', 'n_fit' [P]}: 41 M + 12 bytes a pixel) once analyze() has run; None without the
        # key
        self.change_planes = None
        # {map name: {'matched': pixels matched before the sieve, 'removed': pixels it cleared,
        # 'by_year': {onset year: pixels after the sieve}}} once output() ran; None without the key
        self.change_stats = None
        self.change_s = 0.0  # seconds of the change maps' share of analyze() and output()
        # settings.json zonal_stats: {rule or map name: {'table' int64 [Z + 1, B + 1, 4], 'pixels',
        # 'area', 'mean_magnitude', 'mean_duration' [Z + 1, B + 1], 'zone_ids' [Z], 'years' [B],
        # 'pixel_area'}} once output() ran (the last row: outside every zone; the last column:
        # an onset year outside the scene's); None without the key
        self.zonal_stats = None
        self.zonal_files = None  # {name: path of 'tables/zonal-<name>.csv'}
        self.zonal_s = 0.0  # seconds of the zonal tables in output(), the zone raster included
        self._zones = None  # (zone index of each internal pixel int32 [P], zone ids int64 [Z])
        if os.path.exists(self.settings_path):  # what the job cannot do is said at construction
            try:
                with open(self.settings_path) as f:
                    peek = json.load(f)
            except ValueError:
                peek = None  # (setup() reports a settings.json that does not parse)
            if isinstance(peek, dict):
                self._check_ftv(peek)
                self._check_vertex(peek)
                self._check_mmu(peek)
                self._check_change_maps(peek)
                self._check_zonal(peek)

    def _check_zonal(self, settings):
        """settings.json zonal_stats: validated (settings.check_zonal_stats), and supported by a
        job of one rank; ValueError otherwise."""
        from .settings import check_zonal_stats
        if 'zonal_stats' not in check_zonal_stats(settings):
            return
        if self._dist()[1] > 1:
            raise ValueError('zonal_stats is supported on one rank only (world size %d): the '
                             'zonal tables are not distributed' % self._dist()[1])

    def _check_ftv(self, settings):
        """settings.json ftv_eqns: validated (settings.check_ftv_eqns), and supported by a job of
        one rank that keeps the trendline planes; ValueError otherwise."""
        from .settings import check_ftv_eqns
        if not check_ftv_eqns(settings).get('ftv_eqns'):
            return
        if not self.trendline:
            raise ValueError('ftv_eqns needs trendline=True: the fit-to-vertex pass reads the '
                             "analysis's winner / spike / vertex planes")
        if self._dist()[1] > 1:
            raise ValueError('ftv_eqns is supported on one rank only (world size %d): the '
                             'fit-to-vertex pass is not distributed' % self._dist()[1])

    def _check_vertex(self, settings):
        """settings.json vertex_table: validated (settings.check_vertex_table), and supported by a
        job of one rank; ValueError otherwise."""
        from .settings import check_vertex_table
        if 'vertex_table' not in check_vertex_table(settings):
            return
        if self._dist()[1] > 1:
            raise ValueError('vertex_table is supported on one rank only (world size %d): the '
                             'vertex table is not distributed' % self._dist()[1])

    def _check_mmu(self, settings):
        """settings.json mmu: validated (settings.check_mmu), and supported by a job of one rank;
        ValueError otherwise."""
        from .settings import check_mmu
        if 'mmu' not in check_mmu(settings):
            return
        if self._dist()[1] > 1:
            raise ValueError('mmu is supported on one rank only (world size %d): the sieve '
                             'is not distributed' % self._dist()[1])

    def _check_change_maps(self, settings):
        """settings.json change_maps: validated (settings.check_change_maps), and supported by a
        job of one rank; ValueError otherwise."""
        from .settings import check_change_maps
        if 'change_maps' not in check_change_maps(settings):
            return
        if self._dist()[1] > 1:
            raise ValueError('change_maps is supported on one rank only (world size %d): the '
                             'change maps are not distributed' % self._dist()[1])

    @property
    def grid_fn(self):
        """The grid CSV (the reference's grid file): complete once this returns (a one-rank
        job's setup writes it on a thread of its own while parse runs)."""
        self._join_grid()
        return self._grid_fn

    def _join_grid(self):
        w, self._grid_writer = self._grid_writer, None
        if w is not None:
            w[0].join()
            if w[1]:
                raise w[1][0]

    @property
    def order(self):
        """Grid point of each internal pixel (raster order), None in grid order: pixel (row r,
        column c) is grid point c * rows + r, made on first use (49 M entries at c2 size)."""
        if self._order is None and self._raster_hw is not None:
            H, W = self._raster_hw
            self._order = ((np.arange(W, dtype=np.int64) * H)[None, :] +
                           np.arange(H, dtype=np.int64)[:, None]).ravel()
        return self._order

    def _path(self, key):
        return os.path.join(self.root, key)

    @staticmethod
    def _dist():
        """(torch.distributed or None, world size, rank)."""
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                return dist, dist.get_world_size(), dist.get_rank()
        except ImportError:
            pass
        return None, 1, 0

    # 1. setup_mapper
    def setup(self):
        """Rank 0 extracts the rasters into work_dir and writes the grid (a temporary file moved
        into place); the other ranks wait for it, then list the same files."""
        rdir = os.path.join(self.root, IN_RASTS % self.job)
        names = sorted(os.listdir(rdir)) if os.path.isdir(rdir) else []
        rasts = analysis_rasters(names)
        if not rasts:
            raise Exception('No analysis rasters specified for job %s' % self.job)
        dist, _, rank = self._dist()
        if rank == 0:
            self._locate(rdir, rasts)
            os.makedirs(os.path.dirname(self._grid_fn), exist_ok=True)
            tmp = '%s.tmp%d' % (self._grid_fn, os.getpid())

            def write_grid(err):
                try:
                    rast2grid(self.rast_fns[0], out_csv=tmp)
                    os.replace(tmp, self._grid_fn)
                except BaseException as e:  # re-raised by the first grid_fn access
                    err.append(e)
            self._join_grid()
            err = []
            if dist is None:  # one rank: no other process waits for the file
                import threading
                th = threading.Thread(target=write_grid, args=(err,), daemon=True)
                th.start()
                self._grid_writer = (th, err)
            else:
                write_grid(err)
                if err:
                    raise err[0]
        if dist is not None:
            dist.barrier()
        if rank != 0:
            self._locate(rdir, rasts)  # every archive is extracted by now: only listed
        # the grid's point coordinates, as parsing the CSV being written gives them (raster
        # order: made from the template's axes)
        self._internal_order()
        if self._raster_hw is None:
            self.grid_xy = grid_coords(self.rast_fns[0])
        with open(self.settings_path) as f:
            self.settings = json.load(f)
        self._check_ftv(self.settings)
        self._check_vertex(self.settings)
        self._check_mmu(self.settings)
        self._check_change_maps(self.settings)
        self._check_zonal(self.settings)
        return self.rast_fns

    def _internal_order(self):
        """The job's own pixel order. rast2grid lists the template's pixels column by column
        (utils.py:314-321) while a raster is stored row by row, so gathering every raster at the
        grid points in grid order is a transpose of each band (a random-access gather of 49 M
        samples per band and date). Pixels are independent and the outputs are placed by each
        point's raster offset, so when every grid point lands on its own template pixel (the
        co-registered grid setup() builds from the template) the job runs them in raster order
        instead: internal pixel q is raster pixel q and grid point order[q], and a raster with the
        template's georeferencing is read by slicing (ingest_stack raster_grid). The check is
        pt2val's addressing (grid_offsets' operations) on the grid's distinct coordinates: the
        offsets of a column's points depend on its x alone, a row's on its y. The grid CSV keeps
        the reference's order; grid_wkts() gives the WKTs in the internal order."""
        self._order = self._raster_hw = None
        self.raster_grid = None
        tmpl = GeoTiff(self.rast_fns[0])
        H, W = tmpl.height, tmpl.width
        gt = tmpl.geotransform()
        xv, yv = grid_axes(tmpl)
        xo = np.trunc((xv - gt[0]) * 1.0 / gt[1])
        yo = np.trunc((yv - gt[3]) * 1.0 / gt[5])
        if not (np.array_equal(xo, np.arange(W)) and np.array_equal(yo, np.arange(H))):
            return  # some point not on its own pixel: grid order, offsets per point
        self._raster_hw = (H, W)  # self.order: pixel (row r, column c) is grid point c * H + r
        self.grid_xy = (np.tile(xv, H), np.repeat(yv, W))
        self._grid_axes = (xv, yv)  # grid point (r, c) is (xv[c], yv[r])
        self.raster_grid = (gt, H, W)

    def grid_wkts(self):
        """The grid points' WKTs in the job's internal pixel order (that of the stack and of
        every plane): the grid CSV's order unless _internal_order() chose raster order."""
        w = read_grid(self.grid_fn)
        return w if self.order is None else [w[i] for i in self.order]

    def _locate(self, rdir, rasts):
        os.makedirs(self.work_dir, exist_ok=True)
        self.rast_fns, self.mask_fns = [], []
        for n in rasts:
            self.rast_fns.append(rast_local(os.path.join(rdir, n), self.work_dir))
            m = mask_name(n)
            mp = os.path.join(rdir, m)
            # parse_mapper: a mask that cannot be fetched is ignored (:59-63)
            self.mask_fns.append(rast_local(mp, self.work_dir) if m != n and os.path.exists(mp)
                                 else None)

    # 2. parse_mapper
    def parse(self):
        """Band samples and mask validity of the grid points of this rank's tiles only (the tiles
        of the grid dealt round-robin over the ranks, as analyze runs them): a rank's host planes
        and gathers are 1/N of the job's."""
        from .distributed import Mosaic
        from .index_eqn import parse_eqn_bands
        _, world, rank = self._dist()
        P = len(self.grid_xy[0])
        self.mosaic = Mosaic([P], self.tile_pixels, world, rank, 'round_robin')
        # the planes ingested: the bands of index_eqn and, if set, of mask_eqn (the reference's
        # all_bands, utils.py:459-461) and of every fit-to-vertex equation (ftv_eqns)
        eqn_bands = sorted(set(parse_eqn_bands(self.settings['index_eqn'])) |
                           set(parse_eqn_bands(self.settings.get('mask_eqn') or '')) |
                           {b for e in (self.settings.get('ftv_eqns') or {}).values()
                            for b in parse_eqn_bands(e)})
        # on a GPU (LT_JOB_UPLOAD=whole), each raster's planes cross to the device as soon as they
        # are decoded, on the worker that decoded them, while the other rasters decode: analyze()
        # then starts from the device stack
        self._dev_stack = None
        self._stack_meta = self._dev_keep = self._dev_keep_valid = None
        self.decode_times = {}
        K, Q = len(self.rast_fns), sum(t.n for t in self.mosaic.mine)
        up = self._stack_uploader(K, len(eqn_bands), Q)
        dec = (self._device_decoder(up, K, len(eqn_bands), Q, eqn_bands)
               if self.decode == 'device' else None)
        # sample='device': in raster order the decoder is offered every raster first, with its mask
        smp = dec.sample if (dec is not None and self.sample == 'device' and
                             self.raster_grid is not None) else None
        self.stack = ingest_stack(self.rast_fns, self.grid_xy, self.mask_fns, bands=eqn_bands,
                                  pixels=[(t.p0, t.p1) for t in self.mosaic.mine],
                                  raster_grid=self.raster_grid, on_raster=up,
                                  device_decode=dec, device_sample=smp)
        t_sync = time.perf_counter()
        if up is not None and up.bands is not None:
            import torch
            torch.cuda.synchronize(up.device)
            self._dev_stack = (up.bands, up.valid)
        if dec is not None:  # where a device-decode parse spent its time (thread-seconds)
            self.decode_times = dict(dec.times, sync=time.perf_counter() - t_sync)
        on_dev = (dec.taken | dec.sampled) if dec is not None else set()
        self.decode_stats = {'device': len(on_dev), 'host': K - len(on_dev)}
        n_masks = sum(1 for m in self.mask_fns if m)
        self.sample_stats = {'rasters': len(dec.sampled) if dec is not None else 0,
                             'masks_device': dec.masks if dec is not None else 0,
                             'masks_host': n_masks - (dec.masks if dec is not None else 0)}
        if dec is not None:
            dec.check()
            if on_dev:
                # the job reads the device stack from here on; stack['bands'] and stack['valid']
                # stay usable for callers: the planes of the rasters decoded on the device, and the
                # validity rows of those sampled there, come down on first access
                hb = dict.__getitem__(self.stack, 'bands')
                self._stack_meta = (hb.dtype, tuple(hb.shape))
                self._dev_keep = up.bands
                self._dev_keep_valid = up.valid if dec.sampled else None
                self.stack = _LazyBands(self.stack, self._fill_bands(sorted(on_dev)),
                                        self._fill_valid(sorted(dec.sampled)))
        return self.stack

    def _fill_bands(self, taken):
        def fill(host):
            dev, self._dev_keep = self._dev_keep, None
            for k in taken:
                host[k] = dev[k].cpu().numpy()
        return fill

    def _fill_valid(self, sampled):
        def fill(host):
            dev, self._dev_keep_valid = self._dev_keep_valid, None
            for k in sampled:
                host[k] = dev[k].cpu().numpy()
        return fill if sampled else None

    def device_takes(self, ds):
        """Whether a decode='device' job offers this open GeoTiff to the device decoder: by
        device_formats, GeoTiff.device_eligible ('strips') or device_chunks_eligible ('all')."""
        if self.device_formats == 'all':
            return ds.device_chunks_eligible()
        return ds.device_eligible()

    def _device_decoder(self, up, K, nb, Q, eqn_bands=None):
        """ingest_stack's device_decode of a decode='device' job (None: host decode for the whole
        job — no GPU uploader, or a stack above the 64 GB rule analyze() applies for the whole-stack
        upload). Makes the [K, nb, Q] device stack up front in the first raster's sample type;
        each accepted raster is staged in a pinned buffer of the calling worker thread and decoded
        on one of a few streams (GeoTiff.read_device, or read_device_chunks with
        device_formats='all'; check=False: check() reads every error word once parse has
        synchronised)."""
        import threading
        import torch
        if up is None:
            return None
        first = GeoTiff(self.rast_fns[0])
        dtype = first.dtype.newbyteorder('=')
        if K * nb * Q * dtype.itemsize + K * Q > (64 << 30):
            return None
        if self.engine is None:
            from .engine import get_engine
            self.engine = get_engine(up.device)
        eng = self.engine
        with torch.cuda.device(up.device):
            up.bands = torch.empty((K, nb, Q), dtype=torch.from_numpy(np.empty(0, dtype)).dtype,
                                   device=up.device)
            up.valid = torch.empty((K, Q), dtype=torch.uint8, device=up.device)
            streams = [torch.cuda.Stream(device=up.device) for _ in range(8)]
        tl = threading.local()
        lock = threading.Lock()
        rast_fns, mask_fns = self.rast_fns, self.mask_fns
        # sample='device': the stack's pixel ranges (p0, p1, column of p0), the bands gathered, the
        # grid's axes, and the per-axis offsets on the device per (geotransform, rows, cols)
        spans, q = [], 0
        for t in self.mosaic.mine:
            spans.append((t.p0, t.p1, q))
            q += t.n
        sel = [b - 1 for b in (eqn_bands or [])]
        axes = getattr(self, '_grid_axes', None) if self.raster_grid is not None else None
        offsets = {}
        what = 'strips or tiles' if self.device_formats == 'all' else 'strips'
        # device_formats: which files are offered to the device, and the reader that takes them
        eligible = self.device_takes
        read_device = (GeoTiff.read_device_chunks if self.device_formats == 'all'
                       else GeoTiff.read_device)

        class Dec:
            def __init__(self):
                self.taken, self.errs, self.threads = set(), [], 0
                self.sampled, self.masks = set(), 0
                # seconds summed over the worker threads: waiting for the staging buffer,
                # allocating it, and GeoTiff.read_device (staging copy, H2D and launch calls)
                self.times = {'wait': 0.0, 'alloc': 0.0, 'read': 0.0}

            def _read(self, ds, out):
                """ds decoded into `out` on this worker's stream, through its staging buffer;
                returns the error word and the seconds spent (wait, alloc, read)."""
                if not hasattr(tl, 'stream'):
                    with lock:
                        tl.stream = streams[self.threads % len(streams)]
                        self.threads += 1
                    tl.staging, tl.staged, tl.scratch = None, None, None
                need = ds.staging_bytes()  # (the strip or the tile tags' entries)
                t0 = time.perf_counter()
                if tl.staged is not None:  # the previous raster's bytes have left the buffer
                    tl.staged.synchronize()
                t1 = time.perf_counter()
                if tl.staging is None or tl.staging.numel() < need:
                    tl.staging = torch.empty(need, dtype=torch.uint8, pin_memory=True)
                t2 = time.perf_counter()
                if out is None:  # the worker's scratch raster, grown on demand
                    n = ds.bands * ds.height * ds.width * ds.dtype.itemsize
                    if tl.scratch is None or tl.scratch.numel() < n:
                        with torch.cuda.stream(tl.stream):
                            tl.scratch = None
                            tl.scratch = torch.empty(n, dtype=torch.uint8, device=up.device)
                    tdt = torch.from_numpy(np.empty(0, ds.dtype.newbyteorder('='))).dtype
                    out = tl.scratch[:n].view(tdt).view(ds.bands, ds.height, ds.width)
                _, err = read_device(ds, eng, out=out, stream=tl.stream, check=False,
                                     staging=tl.staging)
                t3 = time.perf_counter()
                tl.staged = ds.staged
                return out, err, (t1 - t0, t2 - t1, t3 - t2)

            def _count(self, dts):
                for key, dt in zip(('wait', 'alloc', 'read'), dts):
                    self.times[key] += dt

            def __call__(self, k, ds):
                if (not eligible(ds) or ds.bands != nb or
                        ds.dtype.newbyteorder('=') != dtype or ds.width * ds.height != Q):
                    return False
                _, err, dts = self._read(ds, up.bands[k].view(ds.bands, ds.height, ds.width))
                with lock:
                    self.taken.add(k)
                    self.errs.append((k, rast_fns[k], err))
                    self._count(dts)
                return True

            def _offsets(self, ds):
                from .ingest import axis_offsets
                key = (ds.geotransform(), ds.height, ds.width)
                with lock:
                    hit = offsets.get(key)
                    if hit is None:
                        xo, yo = axis_offsets(key[0], (ds.height, ds.width), *axes)
                        with torch.cuda.device(up.device):
                            hit = offsets[key] = (torch.from_numpy(xo).to(up.device),
                                                  torch.from_numpy(yo).to(up.device))
                return hit

            def sample(self, k, ds, mds):
                """ingest_stack's device_sample: raster k and its mask decoded into this worker's
                scratch raster and sampled at the stack's pixel ranges (Engine.sample_grid), all on
                the worker's stream."""
                if (axes is None or not sel or not eligible(ds) or
                        ds.dtype.newbyteorder('=') != dtype or ds.bands < max(sel) + 1 or
                        max(ds.height, ds.width) >= 1 << 31):
                    return False
                if mds is not None and not (eligible(mds) and mds.dtype.kind in 'iu' and
                                            max(mds.height, mds.width) < 1 << 31):
                    return False
                for g, mode, name in ((ds, _abi.LT_SAMPLE_BANDS, rast_fns[k]),
                                      (mds, _abi.LT_SAMPLE_MASK, mask_fns[k])):
                    if g is None:
                        continue
                    xo, yo = self._offsets(g)
                    src, err, dts = self._read(g, None)
                    jobs = [dict(src=src, xoff=xo, yoff=yo, p0=p0, n=p1 - p0, mode=mode,
                                 sel=sel if mode == _abi.LT_SAMPLE_BANDS else [0],
                                 out=up.bands[k][:, q0:q0 + p1 - p0],
                                 valid=up.valid[k][q0:q0 + p1 - p0])
                            for p0, p1, q0 in spans]
                    eng.sample_grid(jobs, stream=tl.stream)
                    with lock:
                        self.errs.append((k, name, err))
                        self._count(dts)
                with lock:
                    self.sampled.add(k)
                    self.masks += mds is not None
                return True

            def check(self):
                from .geotiff import TiffError
                for _, name, err in sorted(self.errs, key=lambda e: e[:2]):
                    rc = int(err.item())
                    if rc != 0:
                        raise TiffError('%s: TIFF %s: corrupt or unsupported data (%d)'
                                        % (name, what, rc))
        return Dec()

    def _stack_uploader(self, K, nb, Q):
        """The per-raster H2D of parse() (None when the job does not run on a GPU, or
        LT_JOB_UPLOAD is not 'whole')."""
        import threading
        import torch
        if os.environ.get('LT_JOB_UPLOAD', 'whole') != 'whole' or not torch.cuda.is_available():
            return None
        if self.engine is not None and torch.device(self.engine.device).type != 'cuda':
            return None
        dev = torch.device('cuda', self.device if self.device is not None
                           else torch.cuda.current_device())

        class Up:
            def __init__(self):
                self.device, self.bands, self.valid = dev, None, None
                self.lock = threading.Lock()

            def __call__(self, k, b, v):
                with self.lock:  # the device stack made by the first raster (its sample type)
                    if self.bands is None:
                        self.bands = torch.empty((K, nb, Q), dtype=torch.from_numpy(b[:0]).dtype,
                                                 device=dev)
                        self.valid = torch.empty((K, Q), dtype=torch.uint8, device=dev)
                with torch.cuda.device(dev):
                    if b is not None:  # (None: decoded on the device, already in plane k)
                        self.bands[k].copy_(torch.from_numpy(b))
                    if v is not None:  # (None: sampled on the device, its validity row too)
                        self.valid[k].copy_(torch.from_numpy(v))
        return Up()

    # 3. analysis_reducer, batched over pixel tiles: the mosaic path (runner.py) bench.py runs
    def analyze(self):
        """Tiles of the grid dealt round-robin over the torch.distributed ranks (one when not
        initialised), analysed by runner.MosaicRunner. The label planes (and status / n_years) go
        to rank 0, the writer, through the LabelExchange; the per-year trendline planes leave the
        GPU per tile, while the next tile computes, into host planes [Y, P] (file-backed maps in
        work_dir, shared by the ranks, when there are several), from a ring of three tiles'
        device buffers: no GPU ever holds more than three tiles of trendline. Returns the
        writer's label planes (device), None on the other ranks."""
        import torch
        from .distributed import TrendlineStream
        from .engine import _DTYPE, LABELS, TRENDLINE, get_engine, pack_valid_bits
        from .index_eqn import IndexProgram, MaskProgram
        from .runner import MosaicRunner, TileInput
        from .scene import build_scene, parse_date
        from .settings import change_map_options, compile_params, vertex_cap
        st = self.stack
        P = st['n_pix']
        dist, world, rank = self._dist()
        if self.engine is None:
            self.engine = get_engine(self.device if self.device is not None else
                                     torch.cuda.current_device())
        eng = self.engine
        dev = torch.device(eng.device)
        cuda = dev.type == 'cuda'
        label_fields = LABELS + ('status', 'n_years')
        tl_fields = TRENDLINE if self.trendline else ('winner',)
        self.scene = build_scene(st['dates'], parse_date(self.settings['target_date']))
        params, self.rules = compile_params(self.settings['line_cost'],
                                            self.settings.get('label_rules', ()),
                                            self.pre_threshold_mode)
        numbers = list(st['band_numbers'])
        # the stack's sample type and shape: in device mode from the device stack (the host
        # array's device-decoded planes are only filled when a caller reads stack['bands'])
        meta = getattr(self, '_stack_meta', None)
        b_dtype, b_shape = meta if meta is not None else (st['bands'].dtype, st['bands'].shape)
        prog = IndexProgram(self.settings['index_eqn'], band_dtype=b_dtype,
                            raster_count=max(numbers))
        slots = [numbers.index(b) for b in prog.bands]  # the planes the equation reads
        fn = eng.compile_index(prog)
        # mask_eqn: a boolean expression over the same planes, ANDed into the validity the
        # analysis reads (stack['valid'] keeps the ingest validity). On the GPU one streaming
        # pass (Engine.apply_mask) over the device stack, or over each tile's planes in the
        # 'tile' upload mode; an engine without apply_mask (the tests' CPU double) gets
        # MaskProgram.evaluate's numpy result.
        self.mask_stats = None
        mprog = mfn = None
        m_obs = m_drop = 0  # valid observation-pixels before the mask, and those it dropped
        m_events = []
        if self.settings.get('mask_eqn'):
            mprog = MaskProgram(self.settings['mask_eqn'], b_dtype, numbers,
                                raster_count=max(numbers))
            if hasattr(eng, 'apply_mask'):
                mfn = eng.compile_mask(mprog)
                m_drop = torch.zeros(1, dtype=torch.int64, device=dev)

        def mask_device(bands, valid):  # valid &= mask on device planes, in place
            nonlocal m_obs
            m_obs = m_obs + valid.count_nonzero()
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record(torch.cuda.current_stream(dev))
            eng.apply_mask(mfn, bands, valid, dropped=m_drop)
            ev[1].record(torch.cuda.current_stream(dev))
            m_events.append(ev)
        m = self.mosaic
        if (m.world, m.rank, m.scene_pixels) != (world, rank, [P]):
            raise RuntimeError('parse() ran under another process group')
        K, Y = self.scene.n_obs, self.scene.n_years
        t_in = time.perf_counter()
        # LT_JOB_UPLOAD 'whole' (default on a GPU): the rank's gathered stack (its tiles' pixel
        # ranges) crosses to the device in one copy per array and each tile's inputs are made from
        # device views of it; 'tile': each tile's bands gathered into a host copy first (a 2 GB
        # single-threaded copy per 16.8 Mpx tile, most of round 6's job analysis time)
        b_nbytes = int(np.prod(b_shape)) * np.dtype(b_dtype).itemsize
        # (device mode: the [K, Q] uint8 validity plane's size from the stack's shape as well; its
        # device-sampled rows are only filled when a caller reads stack['valid'])
        v_nbytes = b_shape[0] * b_shape[2] if meta is not None else st['valid'].nbytes
        whole = (cuda and os.environ.get('LT_JOB_UPLOAD', 'whole') == 'whole' and
                 (meta is not None or (st['bands'].flags.c_contiguous and
                                       st['valid'].flags.c_contiguous)) and
                 b_nbytes + v_nbytes <= (64 << 30))
        if whole:
            ds = getattr(self, '_dev_stack', None)
            if ds is not None and ds[0].device == dev and tuple(ds[0].shape) == tuple(b_shape):
                w_bands, w_valid = ds  # uploaded raster by raster during parse()
            else:
                w_bands = torch.from_numpy(st['bands']).to(dev)
                w_valid = torch.from_numpy(st['valid']).to(dev)
            self._dev_stack = None
            if mfn is not None:
                if w_valid is getattr(self, '_dev_keep_valid', None):
                    w_valid = w_valid.clone()  # (stack['valid'] comes down from that tensor)
                mask_device(w_bands, w_valid)
            if slots == list(range(slots[0], slots[0] + len(slots))):
                # (a run of planes of a stack that also holds mask_eqn's: a view, no copy)
                w_bands = w_bands[:, slots[0]:slots[0] + len(slots)]
            elif slots != list(range(b_shape[1])):
                w_bands = w_bands[:, slots]
        items = []
        for t in m.mine:
            if whole:
                q = stack_offset(st, t.p0, t.p1)
                bands = w_bands[:, :, q:q + t.n]
                valid = w_valid[:, q:q + t.n]
            else:
                t_bands, t_valid = stack_range(st, t.p0, t.p1)
                if mprog is not None and mfn is None:  # no HIP engine: the numpy evaluation
                    keep = mprog.evaluate(np.moveaxis(t_bands, 1, 0))
                    m_obs += int(np.count_nonzero(t_valid))
                    m_drop += int(np.count_nonzero((t_valid != 0) & ~keep))
                    t_valid = np.where(keep, t_valid, 0).astype(np.uint8)
                valid = torch.from_numpy(np.ascontiguousarray(t_valid)).to(dev)
                if mfn is not None:  # the mask reads every plane of the tile
                    bands = torch.from_numpy(np.ascontiguousarray(t_bands)).to(dev)
                    mask_device(bands, valid)
                    if slots != list(range(b_shape[1])):
                        bands = bands[:, slots].contiguous()
                else:
                    bands = torch.from_numpy(np.ascontiguousarray(t_bands[:, slots])).to(dev)
            if cuda and fn.lin is not None and len(slots) == 2 and bands.dtype == torch.int16:
                # the fused load stage reads a pixel's two int16 bands as one 32-bit word
                inter = torch.empty((K, t.n, 2), dtype=bands.dtype, device=dev).permute(0, 2, 1)
                inter.copy_(bands)
                bands = inter
            elif whole:
                bands = bands.contiguous()
            if whole:
                valid = valid.contiguous()
            if cuda:  # the winner pick reads the mask as bit planes (one word per 32 obs)
                valid = pack_valid_bits(valid)
            # the index raster: allocated by the runner only if the load kernel writes it (the
            # fused load stage never does)
            items.append(TileInput(t, self.scene, None, valid, bands))
        if whole:
            del w_bands, w_valid  # every tile holds its own copies
        if cuda:
            torch.cuda.synchronize(dev)
        self.analyze_s = {'inputs': time.perf_counter() - t_in}
        if mprog is not None:
            self.mask_stats = {'eqn': mprog.eqn, 'observations': int(m_obs),
                               'dropped': int(m_drop)}
            if m_events:  # the mask kernels' time on the device
                self.analyze_s['mask'] = sum(a.elapsed_time(b) for a, b in m_events) * 1e-3
        host = self.host_trendline = self._trendline_planes(tl_fields, Y, P, dist, world, rank)
        # settings.json vertex_table: the tile's device planes gain what the table is made from
        # (not streamed to the host unless the trendline is), and each tile's vertices are
        # compacted (Engine.vertex_table) straight into scene-wide device planes [V, P] at the
        # tile's offset: 20 V + 4 bytes a pixel that stay on the device like the label planes
        V = vertex_cap(self.settings, Y)
        vt_fields = tuple(f for f in ('val_raw', 'val_fit', 'vertex')
                          if f not in tl_fields) if V is not None else ()
        self.vertex_planes = vt = None
        if V is not None:
            if not hasattr(eng, 'vertex_table'):
                raise RuntimeError('vertex_table needs the HIP engine (no CPU path exists)')
            vt = self.vertex_planes = {
                'n_vertices': torch.empty(P, dtype=torch.int32, device=dev),
                'vertex_year': torch.empty((V, P), dtype=torch.int32, device=dev),
                'vertex_fit': torch.empty((V, P), dtype=torch.float64, device=dev),
                'vertex_raw': torch.empty((V, P), dtype=torch.float64, device=dev)}

        # settings.json change_maps: likewise the tile's device planes gain what the maps are made
        # from, and each tile's maps are evaluated (Engine.change_maps, all of them in one pass)
        # straight into scene-wide device planes at the tile's offset
        self._change_opts = cm_opts = change_map_options(self.settings)
        cm_fields = tuple(f for f in ('val_fit', 'vertex', 'val_raw', 'spike')
                          if f not in tl_fields + vt_fields) if cm_opts is not None else ()
        self.change_planes = cm = None
        self.change_stats = None
        self.change_s = 0.0
        if cm_opts is not None:
            if not hasattr(eng, 'change_maps'):
                raise RuntimeError('change_maps needs the HIP engine (no CPU path exists)')
            M = len(cm_opts)
            cm = self.change_planes = {
                f: torch.empty((M, P), dtype=getattr(torch, d), device=dev)
                for f, d in _abi.CHANGE_MAP_FIELDS}
            cm.update({f: torch.empty(P, dtype=getattr(torch, d), device=dev)
                       for f, d in _abi.CHANGE_PIX_FIELDS})

        def changes(k):  # tile k's change maps, on the current stream, behind its last stage
            t, o = items[k].tile, runner.outs[k]
            eng.change_maps(self.scene.years, cm_opts, o['val_fit'][:, :t.n],
                            o['vertex'][:, :t.n], winner=o['winner'][:, :t.n],
                            val_raw=o['val_raw'][:, :t.n], spike=o['spike'][:, :t.n],
                            out={f: a[..., t.p0:t.p1] for f, a in cm.items()})

        def vertices(k):  # tile k's vertices, on the current stream, behind the tile's last stage
            t, o = items[k].tile, runner.outs[k]
            eng.vertex_table(self.scene.years, o['val_fit'][:, :t.n], o['vertex'][:, :t.n],
                             winner=o['winner'][:, :t.n], val_raw=o['val_raw'][:, :t.n],
                             max_vertices=V, out={f: a[..., t.p0:t.p1] for f, a in vt.items()})
        # the trendline planes: a ring of three tiles' buffers on the GPU (tile k reuses tile
        # k-3's once its rows have reached the host), so a rank's HBM never holds all its tiles'
        # trendlines
        # LT_JOB_JIT: 'off' (default) — the precompiled kernels (a linear index_eqn fused into
        # them, any other through the load kernel): a scene's analysis is ~1 % of a job's time
        # (tools/job_bench.py: 49 Mpx in ~20 ms of kernels against seconds of decode and IO),
        # while a hiprtc compile takes ~10 s of host time and, left running on its worker thread
        # past the analysis, slowed the output step 13x (profiles/r06_run6d); 'async' — the module
        # compiles on a worker thread while the first tiles run precompiled (same results);
        # 'sync' — compile first (a disk-cached module loads at once)
        jit_mode = os.environ.get('LT_JOB_JIT', 'sync' if os.environ.get('LT_JOB_JIT_SYNC') == '1'
                                  else 'off')
        runner = MosaicRunner(eng, m, params, items, label_fields + tl_fields + vt_fields + cm_fields,
                              fn,
                              dist, exchange_fields=label_fields, ring=3 if cuda else 0,
                              jit=jit_mode != 'off')
        jit_async = cuda and runner.jit is not None and jit_mode == 'async'
        if jit_async:
            eng.set_jit_mode(True)
            runner.prepare_jit(wait=False)

        # a completed year row of tile t, copied from its pinned ring buffer into the host plane
        # in pieces on a pool of host threads (numpy releases the GIL for the copy): one thread
        # copied ~10 GB/s, the bound of a trendline job's analysis (profiles/r06_run33); the ring
        # buffer is reused only after sink() returns
        from concurrent.futures import ThreadPoolExecutor
        from .ingest import host_threads
        n_cp = max(1, min(8, host_threads()))
        pool = ThreadPoolExecutor(n_cp) if cuda and n_cp > 1 else None

        def sink(f, row, view, t):  # one completed year row of tile t
            src = view.numpy().view(host[f].dtype)
            dst = host[f][row, t.p0:t.p1]
            n = src.shape[0]
            if pool is None or n < (1 << 20):
                dst[...] = src
                return
            step = -(-n // n_cp)

            def piece(a):
                dst[a:a + step] = src[a:a + step]
            list(pool.map(piece, range(0, n, step)))

        # the ring's rows sized for the widest plane streamed (the labels-only job's winner rows
        # are 4 bytes a pixel: half the pinned memory to allocate)
        row_b = max(torch.empty(0, dtype=_DTYPE[f]).element_size() for f in tl_fields)
        tls = TrendlineStream(m.tile * row_b, dev, depth=16, sink=sink) if cuda else None
        copied = {}  # tile -> event after its rows' D2H copies

        def push(k):
            t = items[k].tile
            copied[k] = tls.push({f: runner.outs[k][f] for f in tl_fields}, t.n, t)

        # tile k-1's rows are queued behind tile k's kernels, so the copies overlap them; tile k's
        # vertex table and change maps are queued first, behind its last stage (the step's calls are joined to the
        # stream at one rank) and ahead of the event that reports its ring buffer free (recorded
        # by push(k), after everything queued here)
        def after(k):
            if vt is not None:
                vertices(k)
            if cm is not None:
                changes(k)
            if k > 0:
                push(k - 1)

        t_st = time.perf_counter()
        try:
            runner.step(after_tile=after if cuda else None,
                        slab_free=copied.get if cuda else None)
        finally:
            # the engine is cached per device (get_engine): a failed step must not leave later
            # jobs of this process in async-JIT mode
            if jit_async:
                eng.set_jit_mode(False)
        if jit_async:
            self.jit_stats = eng.jit_stats()
        if cuda:
            if items:
                push(len(items) - 1)
            torch.cuda.synchronize(dev)
            self.analyze_s['steps'] = time.perf_counter() - t_st
            t_dr = time.perf_counter()
            tls.drain()
            self.analyze_s['drain'] = time.perf_counter() - t_dr
        if pool is not None:
            pool.shutdown()
        else:  # a CPU engine (tests): its planes are host tensors already
            for o, it in zip(runner.outs, items):
                for f in tl_fields:
                    host[f][:, it.tile.p0:it.tile.p1] = o[f][:, :it.tile.n].numpy()
            if vt is not None:
                for k in range(len(items)):
                    vertices(k)
            if cm is not None:
                t_cm = time.perf_counter()
                for k in range(len(items)):
                    changes(k)
                self.change_s += time.perf_counter() - t_cm
        for a in host.values():
            if isinstance(a, np.memmap):
                a.flush()
        if dist is not None:
            dist.barrier()  # every rank's trendline rows are in the shared maps
        self._host = None
        if not runner.exchange.is_writer:
            self.dev_planes = None
            return None
        # the writer's label planes stay on the device: the output step assembles each raster
        self.dev_planes = {f: runner.exchange.raster(f) for f in label_fields}
        del runner
        self._check_errors()
        return self.dev_planes

    def _trendline_planes(self, fields, Y, P, dist, world, rank):
        """Host [Y, P] planes the trendline rows stream into: in memory for one rank, else
        file-backed maps in work_dir that rank 0 creates and every rank fills with its tiles."""
        from .engine import _DTYPE
        np_dt = {f: np.dtype(str(_DTYPE[f]).replace('torch.', '')) for f in fields}
        if world == 1:
            return {f: np.empty((Y, P), np_dt[f]) for f in fields}
        d = os.path.join(self.work_dir, 'trendline')
        path = {f: os.path.join(d, f + '.bin') for f in fields}
        if rank == 0:
            os.makedirs(d, exist_ok=True)
            for f in fields:
                np.memmap(path[f], np_dt[f], 'w+', shape=(Y, P)).flush()
        dist.barrier()
        return {f: np.memmap(path[f], np_dt[f], 'r+', shape=(Y, P)) for f in fields}

    @property
    def planes(self):
        """Host copies of the writer's output planes (made on first use): the label planes and
        the trendline planes."""
        if self._host is None and self.dev_planes is not None:
            self._host = {f: t.cpu().numpy() for f, t in self.dev_planes.items()}
            self._host.update({f: np.asarray(a) for f, a in self.host_trendline.items()})
        return self._host

    def _check_errors(self):
        import torch
        from .utils import _raise_for_status
        status = self.dev_planes['status'].cpu().numpy()
        bad = np.flatnonzero(status & ~_abi.LT_ST_EMPTY)
        if len(bad) == 0:
            return
        if self.on_error == 'raise':
            p = int(bad[0])
            wkt = self.grid_wkts()[p]
            s = int(status[p])
            if s & _abi.LT_ST_PRE_THRESHOLD_ATTR:
                raise AttributeError("LabelRule instance has no attribute 'threshold' (pixel %s)"
                                     % wkt)
            try:
                _raise_for_status(s, None)
            except Exception as e:
                raise type(e)('%s (pixel %s)' % (e, wkt)) from e
        else:  # skip: the failing pixels emit nothing
            idx = torch.from_numpy(bad).to(self.dev_planes['matched'].device)
            self.dev_planes['matched'][:, idx] = 0
            self.host_trendline['winner'][:, bad] = -1  # no trendline key either
            if self.vertex_planes is not None:  # nor a vertex
                self.vertex_planes['n_vertices'][idx.to(
                    self.vertex_planes['n_vertices'].device)] = 0
            self._host = None

    def _sieve(self, rows, cols):
        """settings.json mmu: each rule's matched row of the scene-wide label planes sieved in
        place on their device (Engine.sieve; the key is the rule's onset_year row, or none with
        by 'match'), after the EMPTY and rejected pixels' matches are cleared and before any
        raster is assembled, so every label raster of a rule shows NODATA on a removed patch.
        The trendline, vertex-table and FTV rasters are not touched. Needs the raster order (the
        planes are then the rasters, pixel for pixel) and an engine with a sieve: there is no CPU
        path."""
        from .settings import mmu_options
        opt = mmu_options(self.settings)
        self.mmu_stats = None
        if opt is None:
            return
        if self._raster_hw is None:
            raise RuntimeError('mmu needs the raster order (every grid point on its own template '
                               'pixel): the label planes of this job are in grid order')
        if not hasattr(self.engine, 'sieve'):
            raise RuntimeError('mmu needs the HIP engine (no CPU path exists)')
        t0 = time.perf_counter()
        dp = self.dev_planes
        before = dp['matched'].ne(0).sum(dim=1)
        for r in range(len(self.rules)):
            self.engine.sieve(dp['matched'][r], dp['onset_year'][r] if opt['by'] == 'onset_year'
                              else None, (rows, cols), opt['min_pixels'], opt['connectivity'])
        after = dp['matched'].ne(0).sum(dim=1)
        counts = zip(before.cpu().tolist(), after.cpu().tolist())  # the one read-back: 2 R counts
        self.mmu_stats = {rule.name: {'matched': b, 'removed': b - a}
                          for rule, (b, a) in zip(self.rules, counts)}
        self.mmu_s = time.perf_counter() - t0
        self._host = None

    def _change_output(self, rows, cols):
        """settings.json change_maps, between the analysis and the rasters: on the planes'
        device, `matched` is cleared on the pixels the job drops (EMPTY, and under
        on_error='skip' the rejected ones: self._change_keep is the mask of the others), each map
        that has an mmu above 1 is sieved in place (Engine.sieve; the key is the map's onset_year
        row, or none with by 'match'; needs the raster order, as _sieve does), and every map is
        counted per onset year before and after the sieve (Engine.label_counts) into
        self.change_stats; the two [M, Y + 1] count tables are the only read-back."""
        cm, opts = self.change_planes, self._change_opts
        self._change_keep = None
        if cm is None:
            return
        import torch
        t0 = time.perf_counter()
        eng = self.engine
        for need in ('change_maps', 'label_counts'):
            if not hasattr(eng, need):
                raise RuntimeError('change_maps needs the HIP engine (no CPU path exists)')
        keep = self._change_keep = (self.dev_planes['status'] == 0).to(cm['matched'].device)
        cm['matched'].masked_fill_(~keep[None, :], 0)
        years = [int(y) for y in self.scene.years]
        lo = min(years)
        n_bins = min(max(years) - lo + 1, 256)
        M = len(opts)
        counts = torch.zeros((2, M, n_bins + 1), dtype=torch.int64, device=cm['matched'].device)
        for m, opt in enumerate(opts):
            eng.label_counts(cm['matched'][m], cm['onset_year'][m], lo, n_bins, out=counts[0, m])
            mmu = opt['mmu']
            if mmu is not None and mmu['min_pixels'] > 1:
                if self._raster_hw is None:
                    raise RuntimeError('change_maps: mmu needs the raster order (every grid '
                                       'point on its own template pixel): the planes of this '
                                       'job are in grid order')
                if not hasattr(eng, 'sieve'):
                    raise RuntimeError('change_maps: mmu needs the HIP engine (no CPU path '
                                       'exists)')
                eng.sieve(cm['matched'][m], cm['onset_year'][m] if mmu['by'] == 'onset_year'
                          else None, (rows, cols), mmu['min_pixels'], mmu['connectivity'])
            eng.label_counts(cm['matched'][m], cm['onset_year'][m], lo, n_bins, out=counts[1, m])
        c = counts.cpu().numpy()  # the one read-back
        self.change_stats = {}
        for m, opt in enumerate(opts):
            before, after = int(c[0, m].sum()), int(c[1, m].sum())
            self.change_stats[opt['name']] = {
                'matched': before, 'removed': before - after,
                'by_year': {y: int(c[1, m, y - lo]) for y in sorted(set(years))
                            if y - lo < n_bins}}
        self._change_live = [int(c[1, m].sum()) > 0 for m in range(M)]
        self.change_s += time.perf_counter() - t0

    def _zone_index(self, opt):
        """settings.json zonal_stats, once per job: the zone raster sampled at the grid points on
        the host as every other raster is (GeoTiff.read and grid_offsets: pt2val's truncation, but
        not its wrap of a negative offset). -> (zone index of each internal pixel, int32 [P]; the
        zone ids, int64 [Z] ascending): index k is the k-th smallest id; a grid point off the
        raster, on its GDAL_NODATA value or on an ignored id has index -1."""
        if self._zones is not None:
            return self._zones
        fn = opt['zones']
        if not os.path.isabs(fn):
            fn = os.path.join(self.root, self.job, 'input', fn)
        if not os.path.exists(fn):
            raise ValueError('zonal_stats: no zone raster %s' % fn)
        zt = GeoTiff(fn)
        if zt.dtype.kind not in 'iu':
            raise ValueError('zonal_stats: the zone raster %s holds %s samples; integer zone ids '
                             'are required' % (fn, zt.dtype.newbyteorder('=')))
        if opt['band'] > zt.bands:
            raise ValueError('zonal_stats: band %d of a zone raster with %d band(s)'
                             % (opt['band'], zt.bands))
        lng, lat = self.grid_xy
        zgt = zt.geotransform()
        lng, lat = np.asarray(lng), np.asarray(lat)
        at, ok = grid_offsets(zgt, (zt.height, zt.width), lng, lat)
        # a zone is a place: a point whose offset truncates below zero is off the raster (pt2val's
        # numpy indexing would wrap it to the far side; the analysis rasters keep that); an offset
        # in (-1, 0) truncates to zero, as pt2val's does, and reads the first row or column
        ok = ok & (np.trunc((lng - zgt[0]) * 1.0 / zgt[1]) >= 0) & \
            (np.trunc((lat - zgt[3]) * 1.0 / zgt[5]) >= 0)
        band = zt.read()[opt['band'] - 1].reshape(-1)
        ids = band[at]
        if ids.dtype.kind == 'u' and ids.dtype.itemsize == 8:
            if ids.max(initial=0) >= 2 ** 63:
                raise ValueError('zonal_stats: zone ids of 2^63 and above are not supported')
        ids = ids.astype(np.int64)
        live = np.asarray(ok, bool).copy()
        drop = list(opt['ignore'])
        if zt.nodata is not None and float(zt.nodata).is_integer():
            drop.append(int(zt.nodata))
        if drop:
            live &= ~np.isin(ids, np.array(drop, np.int64))
        zone_ids, dense = np.unique(ids[live], return_inverse=True)
        if len(zone_ids) > _abi.LT_MAX_ZONES:
            raise ValueError('zonal_stats: %d distinct zone ids, more than LT_MAX_ZONES (%d)'
                             % (len(zone_ids), _abi.LT_MAX_ZONES))
        index = np.full(len(ids), -1, np.int32)
        index[live] = dense.astype(np.int32)
        self._zones = (index, zone_ids.astype(np.int64))
        return self._zones

    def _zonal_output(self, tmpl):
        """settings.json zonal_stats, after the sieve and the change maps' output pass and before
        any raster is assembled: every label rule's and every change map's published planes
        (matched, onset_year, duration, magnitude: EMPTY and rejected pixels cleared, the MMU
        applied) summed per zone and onset year on their device (Engine.zonal_stats), all tables
        read back in one copy, into self.zonal_stats and 'output/tables/zonal-<name>.csv'. No
        raster is written or changed."""
        from .settings import zonal_stats_options
        opt = zonal_stats_options(self.settings)
        self.zonal_stats = self.zonal_files = None
        if opt is None:
            return
        import torch
        eng = self.engine
        if not hasattr(eng, 'zonal_stats'):
            raise RuntimeError('zonal_stats needs the HIP engine (no CPU path exists)')
        t0 = time.perf_counter()
        index, zone_ids = self._zone_index(opt)
        Z = len(zone_ids)
        nz = max(Z, 1)  # (no zone at all: one row that stays empty, dropped below)
        years = [int(y) for y in self.scene.years]
        lo = min(years)
        n_bins = min(max(years) - lo + 1, 256)
        jobs = []  # (name, the four plane rows)
        if 'labels' in opt['of']:
            dp = self.dev_planes
            jobs += [(rule.name, [dp[f][r] for f in ('matched', 'onset_year', 'duration',
                                                      'magnitude')])
                     for r, rule in enumerate(self.rules)]
        if 'change_maps' in opt['of'] and self.change_planes is not None:
            cm = self.change_planes
            jobs += [(o['name'], [cm[f][m] for f in ('matched', 'onset_year', 'duration',
                                                      'magnitude')])
                     for m, o in enumerate(self._change_opts)]
        gt = tmpl.geotransform()
        pixel_area = abs(gt[1] * gt[5])
        self.zonal_stats, self.zonal_files = {}, {}
        if jobs:
            dev = jobs[0][1][0].device
            zone = torch.from_numpy(index).to(dev)
            tables = torch.zeros((len(jobs), nz + 1, n_bins + 1, 4), dtype=torch.int64, device=dev)
            for i, (_, (mt, on, du, mg)) in enumerate(jobs):
                eng.zonal_stats(mt, zone.to(mt.device), on, lo, n_bins, nz, duration=du, value=mg,
                                out=tables[i])
            host = tables.cpu().numpy()  # the one read-back
            keep_rows = list(range(Z)) + [nz]
            tdir = os.path.join(self.root, self.job, 'output', 'tables')
            os.makedirs(tdir, exist_ok=True)
            bin_years = np.arange(lo, lo + n_bins, dtype=np.int32)
            for (name, _), full in zip(jobs, host):
                t = np.ascontiguousarray(full[keep_rows])
                with np.errstate(invalid='ignore', divide='ignore'):
                    res = {'table': t, 'pixels': t[..., 0].copy(),
                           'area': t[..., 0] * pixel_area,
                           'mean_magnitude': np.where(t[..., 3] > 0,
                                                      t[..., 2] / 16.0 / t[..., 3], np.nan),
                           'mean_duration': np.where(t[..., 0] > 0,
                                                     t[..., 1] / t[..., 0].astype(np.float64),
                                                     np.nan),
                           'zone_ids': zone_ids, 'years': bin_years, 'pixel_area': pixel_area}
                self.zonal_stats[name] = res
                path = os.path.join(tdir, 'zonal-%s.csv' % name)
                with open(path, 'w', newline='') as fh:
                    fh.write(zonal_csv(res))
                self.zonal_files[name] = path
        self.zonal_s = time.perf_counter() - t0

    # 4. output_reducer
    def output(self):
        """Every output key's raster, written as LZW GeoTIFF with the template's georeferencing.
        With one grid point per raster pixel (the co-registered grid setup builds) the rasters
        are assembled on the GPU (lt_raster_assemble) and each one reaches the host only as its
        finished GDT_Byte (or typed) array, written at once; a grid that maps two points to one
        pixel (the reference's loop: the last one wins) is assembled on the host."""
        import torch
        from .raster import (FTV_ATTRS, _np_dtype, _strip_rows, device_encodable, label_rasters,
                             label_rasters_device, output_reducer, raster_path,
                             change_rasters, change_rasters_device,
                             trendline_rasters, trendline_rasters_device, vertex_rasters,
                             vertex_rasters_device, write_tiff_strips)
        tmpl = GeoTiff(self.rast_fns[0])
        rows, cols = tmpl.height, tmpl.width
        lng, lat = self.grid_xy
        if self._raster_hw is not None:  # raster order: internal pixel q is template pixel q
            dest, ok = np.arange(rows * cols, dtype=np.int64), np.ones(rows * cols, bool)
        else:
            dest, ok = grid_offsets(tmpl.geotransform(), (rows, cols), lng, lat)
        if not ok.all():
            # data2raster assigns holder[y_off, x_off]: an off-template point raises there
            raise IndexError('grid point %s is off the template raster'
                             % self.grid_wkts()[int(np.flatnonzero(~ok)[0])])
        tdt = tmpl.dtype.newbyteorder('=')
        dp = self.dev_planes
        # an EMPTY pixel never reaches the reference's reducer: it emits nothing
        empty = (dp['status'] & _abi.LT_ST_EMPTY) != 0
        dp['matched'].masked_fill_(empty[None, :], 0)
        self._host = None
        self._sieve(rows, cols)
        self._change_output(rows, cols)
        self._zonal_output(tmpl)
        names = [d.strftime('%Y-%m-%d') for d in self.scene.dates]
        cuda = torch.device(self.engine.device).type == 'cuda'
        distinct = self._raster_hw is not None or np.bincount(dest, minlength=rows * cols).max() <= 1
        if cuda and distinct and len(set(names)) == len(names):
            ddest = torch.from_numpy(np.ascontiguousarray(dest, np.int64)).to(dp['status'].device)
            out = {}
            # each raster is encoded and written on a writer thread (its LZW strips on the native
            # pool) while the next one is assembled on the GPU and copied back: at most three in
            # flight; written in key order, the first error re-raised
            from collections import deque
            from concurrent.futures import ThreadPoolExecutor
            writer = ThreadPoolExecutor(1)
            inflight = deque()

            def settle(keep):
                while len(inflight) > keep:
                    out.update(inflight.popleft().result())

            stats = {'device': 0, 'host': 0}

            def write(key, arr):  # each raster to its file as soon as it is on the host
                stats['host'] += 1
                inflight.append(writer.submit(
                    lambda r: dict(output_reducer(r, tmpl, self.root, self.job)), {key: arr}))
                settle(2)

            # encode='device': each assembled batch (a rule set's rasters, one date's attributes)
            # is encoded by the HIP strip encoder on the same stream, every raster with its own
            # sample type and rows per strip (raster_mode 'typed' mixes int32, float64 and uint8);
            # the sizes and totals of the batch come down in one copy, then per raster exactly
            # `total` bytes into one of three pinned buffers, and the writer thread only lays out
            # the header and writes. A raster the encoder does not take goes through write().
            ring = [None] * 3
            turn = [0]

            def put(path, buf, n, sizes, dtype, rps, ev, keep):
                ev.synchronize()
                write_tiff_strips(path, buf[:n].numpy(), sizes, (1, rows, cols), dtype, 5, 1,
                                  rps, tmpl)
                return {keep[0]: [path]}

            def encode_batch(batch):
                plan = []  # per raster: (numpy sample type, rows per strip) or None (host)
                for _, t in batch:
                    ndt = _np_dtype(t)
                    plan.append((ndt, _strip_rows(rows, cols, ndt.itemsize))
                                if device_encodable(ndt, (rows, cols)) else None)
                took = [i for i, p in enumerate(plan) if p is not None]
                enc = self.engine.encode_strips(
                    [{'data': batch[i][1], 'rows_per_strip': plan[i][1], 'compression': 5,
                      'predictor': 1} for i in took]) if took else []
                # one copy for the sizes and totals of the whole batch
                flat = (torch.cat([x for _, sizes, total in enc for x in (sizes, total)])
                        .cpu().numpy() if took else None)
                metas, o = {}, 0
                for i, (_, sizes, _) in zip(took, enc):
                    metas[i] = flat[o:o + sizes.numel() + 1]
                    o += sizes.numel() + 1
                    if int(metas[i][-1]) < 0:
                        raise ValueError('TIFF strips: device encode failed (%d)'
                                         % int(metas[i][-1]))
                need = max([1 << 20] + [int(m[-1]) for m in metas.values()])
                eouts = {i: e[0] for i, e in zip(took, enc)}
                for i, (key, t) in enumerate(batch):
                    if plan[i] is None:
                        write(key, t.cpu().numpy())
                        continue
                    ndt, rps = plan[i]
                    n = int(metas[i][-1])
                    settle(2)  # the buffer of three rasters ago is written out
                    k = turn[0] % 3
                    turn[0] += 1
                    if ring[k] is None or ring[k].numel() < need:
                        ring[k] = torch.empty(need, dtype=torch.uint8).pin_memory()
                    ring[k][:n].copy_(eouts[i][:n], non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(self.engine.device))
                    stats['device'] += 1
                    inflight.append(writer.submit(
                        put, raster_path(self.root, self.job, key), ring[k], n, metas[i][:-1],
                        ndt, rps, ev, (key, eouts[i])))

            dsink = encode_batch if self.encode == 'device' else None
            try:
                for k, a in label_rasters_device(self.engine, dp, self.rules, (rows, cols), ddest,
                                                 tdt, self.raster_mode,
                                                 device_sink=dsink).items():
                    write(k, a)
                if self.vertex_planes is not None:
                    vertex_rasters_device(self.engine, self.vertex_planes, (rows, cols), ddest,
                                          tdt, self.raster_mode, sink=write, device_sink=dsink)
                if self.change_planes is not None:
                    t_cm = time.perf_counter()
                    change_rasters_device(self.engine, self.change_planes, self._change_opts,
                                          (rows, cols), ddest, tdt, self.raster_mode,
                                          keep=self._change_keep, sink=write, device_sink=dsink,
                                          live=self._change_live)
                    self.change_s += time.perf_counter() - t_cm
                if self.trendline:
                    rows_dev = _DeviceRows(self.host_trendline, dp['status'].device)
                    trendline_rasters_device(self.engine, rows_dev, self.scene, self.scene.dates,
                                             (rows, cols), ddest, tdt, self.raster_mode,
                                             sink=write, device_sink=dsink)
                    # fit to vertex: one equation's planes at a time (the host planes are reused)
                    for name, fhost in self._ftv_passes():
                        trendline_rasters_device(
                            self.engine, _DeviceRows(fhost, dp['status'].device, rows_dev.winner),
                            self.scene, self.scene.dates, (rows, cols), ddest, tdt,
                            self.raster_mode, attrs=FTV_ATTRS, sink=write, device_sink=dsink,
                            prefix='ftv/%s/' % name)
                        if self._ftv_vertex is not None:
                            vertex_rasters_device(self.engine, self._ftv_vertex, (rows, cols),
                                                  ddest, tdt, self.raster_mode, sink=write,
                                                  device_sink=dsink,
                                                  prefix='ftv/%s/vertices/' % name)
                        settle(0)  # every raster of the equation is written: its planes are free
                settle(0)
            finally:
                writer.shutdown(wait=True)
            self.encode_stats = stats
            self._join_grid()  # the grid CSV, the job's other output, in place too
            return out
        n = rows * cols
        placed = {}
        for k, a in self.planes.items():
            fill = -1 if k == 'winner' else 0
            b = np.full(a.shape[:-1] + (n,), fill, a.dtype)
            b[..., dest] = a  # repeated offsets: the last grid point wins, as in the loop
            placed[k] = b
        rasters = label_rasters(placed, self.rules, (rows, cols), tdt, self.raster_mode)

        def place_table(table):  # a vertex table's planes in raster order (no vertex elsewhere)
            res = {}
            for k, t in table.items():
                a = t.cpu().numpy()
                b = np.zeros(a.shape[:-1] + (n,), a.dtype)
                b[..., dest] = a
                res[k] = b
            return res
        if self.vertex_planes is not None:
            rasters.update(vertex_rasters(place_table(self.vertex_planes), (rows, cols), tdt,
                                          self.raster_mode))
        if self.change_planes is not None:
            t_cm = time.perf_counter()
            kept = place_table({'keep': self._change_keep})['keep']
            rasters.update(change_rasters(place_table(self.change_planes), self._change_opts,
                                          (rows, cols), tdt, self.raster_mode, keep=kept))
            self.change_s += time.perf_counter() - t_cm
        if self.trendline:
            rasters.update(trendline_rasters(placed, self.scene, self.scene.dates, (rows, cols),
                                             tdt, self.raster_mode))
        res = dict(output_reducer(rasters, tmpl, self.root, self.job))
        if self.trendline:
            for name, fhost in self._ftv_passes():
                fplaced = {'winner': placed['winner']}
                for k, a in fhost.items():
                    b = np.zeros(a.shape[:-1] + (n,), a.dtype)
                    b[..., dest] = a
                    fplaced[k] = b
                res.update(output_reducer(
                    trendline_rasters(fplaced, self.scene, self.scene.dates, (rows, cols), tdt,
                                      self.raster_mode, attrs=FTV_ATTRS, prefix='ftv/%s/' % name),
                    tmpl, self.root, self.job))
                if self._ftv_vertex is not None:
                    res.update(output_reducer(
                        vertex_rasters(place_table(self._ftv_vertex), (rows, cols), tdt,
                                       self.raster_mode, prefix='ftv/%s/vertices/' % name),
                        tmpl, self.root, self.job))
        self.encode_stats = {'device': 0, 'host': len(res)}
        self._join_grid()
        return res

    def _ftv_passes(self):
        """settings.json ftv_eqns after the analysis: for each equation in turn, yields (name, its
        host planes {field: [Y, P] float64}): the equation evaluated as index_eqn would be
        (Engine.index_tile) and fitted to the analysis's vertices (Engine.ftv_tile), the tiles one
        at a time — a tile's winner / spike / vertex rows go up from the host trendline planes, its
        six planes come down — so the device never holds more than one tile of FTV planes. The
        host planes are reused by the next equation: the caller is done with them before it asks
        for the next. A pixel the analysis rejected has no winner there (_check_errors), so it gets
        no FTV raster either. With settings.json vertex_table, self._ftv_vertex holds the
        equation's vertex table while the caller has its planes (its val_fit / val_raw at the
        analysis's vertices, compacted per tile like the analysis's own; device planes [V, P],
        dropped before the next equation's are made), else None."""
        self._ftv_vertex = None
        eqns = self.settings.get('ftv_eqns') or {}
        if not eqns:
            return
        import torch
        from .engine import FTV_FIELDS
        from .index_eqn import IndexProgram
        eng = self.engine
        if not hasattr(eng, 'ftv_tile'):
            raise RuntimeError('ftv_eqns needs the HIP engine (no CPU path exists)')
        dev = torch.device(eng.device)
        st, tl = self.stack, self.host_trendline
        numbers = list(st['band_numbers'])
        b_dtype = self._stack_meta[0] if self._stack_meta is not None else st['bands'].dtype
        Y, P = self.scene.n_years, st['n_pix']
        host = {f: np.empty((Y, P), np.float64) for f in FTV_FIELDS}
        nmax = max([t.n for t in self.mosaic.mine] + [1])
        buf = torch.empty((len(FTV_FIELDS), Y, nmax), dtype=torch.float64, device=dev)
        from .settings import vertex_cap
        V = vertex_cap(self.settings, Y)
        if V is not None:  # the flags in rows of the FTV planes' stride (Engine.vertex_table)
            wbuf = torch.empty((Y, nmax), dtype=torch.int16, device=dev)
            xbuf = torch.empty((Y, nmax), dtype=torch.uint8, device=dev)
        for name, eqn in eqns.items():
            t0 = time.perf_counter()
            self._ftv_vertex = vt = None
            if V is not None:
                vt = self._ftv_vertex = {
                    'n_vertices': torch.empty(P, dtype=torch.int32, device=dev),
                    'vertex_year': torch.empty((V, P), dtype=torch.int32, device=dev),
                    'vertex_fit': torch.empty((V, P), dtype=torch.float64, device=dev),
                    'vertex_raw': torch.empty((V, P), dtype=torch.float64, device=dev)}
            prog = IndexProgram(eqn, band_dtype=b_dtype, raster_count=max(numbers))
            slots = [numbers.index(b) for b in prog.bands]  # the planes the equation reads
            fn = eng.compile_index(prog)
            for t in self.mosaic.mine:
                flags = [torch.from_numpy(np.ascontiguousarray(tl[f][:, t.p0:t.p1])).to(dev)
                         for f in ('winner', 'spike', 'vertex')]
                t_bands, _ = stack_range(st, t.p0, t.p1)
                bands = torch.from_numpy(np.ascontiguousarray(t_bands[:, slots])).to(dev)
                out = {f: buf[i, :, :t.n] for i, f in enumerate(FTV_FIELDS)}
                eng.ftv_tile(self.scene, *flags, eng.index_tile(fn, bands), out=out)
                if vt is not None:
                    wbuf[:, :t.n].copy_(flags[0])
                    xbuf[:, :t.n].copy_(flags[2])
                    eng.vertex_table(self.scene.years, out['val_fit'], xbuf[:, :t.n],
                                     winner=wbuf[:, :t.n], val_raw=out['val_raw'], max_vertices=V,
                                     out={f: a[..., t.p0:t.p1] for f, a in vt.items()})
                for f, o in out.items():
                    host[f][:, t.p0:t.p1] = o.cpu().numpy()
            self.ftv_s[name] = time.perf_counter() - t0
            yield name, host
        self._ftv_vertex = None

    def run(self):
        """Every rank runs setup/parse/analysis; the writer (rank 0) also writes the rasters.
        Returns {key: [path]} on the writer, None on the other ranks."""
        self.setup()
        self.parse()
        if self.analyze() is None:
            self._join_grid()
            return None
        out = self.output()
        self._join_grid()
        return out


class _DeviceRows:
    """The host trendline planes as raster.trendline_rasters_device reads them: 'winner' whole on
    the device (it selects the pixels of every key), every other plane one year row at a time,
    uploaded into a buffer of its own when the row is asked for (the rows of one date's rasters
    are assembled together, then the next date's rows overwrite them in stream order)."""

    def __init__(self, host, device, winner=None):
        import torch
        self.host, self.device = host, device
        # (winner: the device plane another _DeviceRows of the same analysis already holds)
        self.winner = winner if winner is not None else torch.from_numpy(
            np.ascontiguousarray(host['winner'])).to(device)
        self.buf = {}

    def __getitem__(self, field):
        if field == 'winner':
            return self.winner
        return _Rows(self, field)


class _Rows:
    def __init__(self, owner, field):
        self.owner, self.field = owner, field

    def __getitem__(self, y):
        import torch
        o = self.owner
        row = torch.from_numpy(np.ascontiguousarray(o.host[self.field][y]))
        b = o.buf.get(self.field)
        if b is None:
            b = o.buf[self.field] = torch.empty(row.shape, dtype=row.dtype, device=o.device)
        b.copy_(row)
        return b


def main(argv=None):
    ap = argparse.ArgumentParser(description='LandTrendr job on the local GPU (steps of '
                                 'MRLandTrendrJob without mrjob/S3)')
    ap.add_argument('--root', required=True, help='directory holding <job>/input/...')
    ap.add_argument('--job', required=True)
    ap.add_argument('--device', type=int, default=None)
    ap.add_argument('--tile-pixels', type=int, default=1 << 22)
    ap.add_argument('--no-trendline', action='store_true')
    ap.add_argument('--raster-mode', choices=('reference', 'typed'), default='reference')
    ap.add_argument('--pre-threshold-mode', choices=('reference', 'documented'),
                    default='reference')
    ap.add_argument('--on-error', choices=('raise', 'skip'), default='raise')
    a = ap.parse_args(argv)
    dist = None
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        import torch
        import torch.distributed as dist
        local = int(os.environ.get('LOCAL_RANK', '0'))
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
        if a.device is None:
            a.device = local
    j = LocalJob(a.root, a.job, a.device, a.tile_pixels, not a.no_trendline, a.raster_mode,
                 a.pre_threshold_mode, a.on_error)
    res = j.run()
    for key in sorted(res or {}):
        print('%s\t%s' % (key, res[key][0]))
    if dist is not None:
        dist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
