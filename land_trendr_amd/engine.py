"""Tile engine: torch device tensors in, lt_analyze_tile (HIP) on the current stream, tensors out.

One Engine per GPU (per process). torch provides device memory and the stream only; all compute
happens in land_trendr_amd/liblt_hip.so. There is no CPU path.
"""
import ctypes
import threading

import torch

from . import _abi

TRENDLINE = tuple(f for f, _ in _abi.YEAR_FIELDS)
LABELS = tuple(f for f, _ in _abi.RULE_FIELDS)
ALL_FIELDS = TRENDLINE + LABELS + ('status', 'n_years')
LABEL_FIELDS = ('status', 'matched', 'class_val', 'onset_year', 'duration', 'magnitude')
FTV_FIELDS = _abi.FTV_FIELDS  # the planes ftv_tile writes (besides status)

_DT = {'int16': torch.int16, 'int32': torch.int32, 'uint8': torch.uint8,
       'float64': torch.float64}
# raster element types a tile may carry (index rasters, band planes): torch dtype -> LT_T_*
_LT_T = {torch.float64: _abi.LT_T_F64, torch.int16: _abi.LT_T_I16, torch.uint16: _abi.LT_T_U16,
         torch.int32: _abi.LT_T_I32, torch.float32: _abi.LT_T_F32, torch.uint8: _abi.LT_T_U8,
         torch.uint32: _abi.LT_T_U32, torch.int8: _abi.LT_T_I8, torch.int64: _abi.LT_T_I64}
_TORCH_OF_LT = {v: k for k, v in _LT_T.items()}
_SHAPE_KIND = {**{f: 'year' for f, _ in _abi.YEAR_FIELDS},
               **{f: 'rule' for f, _ in _abi.RULE_FIELDS},
               **{f: 'pix' for f, _ in _abi.PIX_FIELDS}}
_DTYPE = {f: _DT[d] for f, d in _abi.YEAR_FIELDS + _abi.RULE_FIELDS + _abi.PIX_FIELDS}


class LtError(RuntimeError):
    pass


class Engine:
    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise LtError('land_trendr_amd needs a HIP device (no CPU fallback)')
        self.lib = _abi.load_lib()
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None
                                   else int(device))
        ctx = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.lt_ctx_create(self.device.index, ctypes.byref(ctx))
        if rc != 0:
            raise LtError('lt_ctx_create failed (%d)' % rc)
        self.ctx = ctx
        self._decode_lock = threading.Lock()
        self._encode_lock = threading.Lock()
        self._sample_lock = threading.Lock()

    def close(self):
        if self.ctx:
            self.lib.lt_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise LtError('%s failed (%d): %s' % (what, rc,
                                                  self.lib.lt_last_error(self.ctx).decode()))

    def alloc_outputs(self, n_years, n_rules, n_pix, fields=ALL_FIELDS):
        out = {}
        for f in fields:
            kind = _SHAPE_KIND[f]
            shape = {'year': (n_years, n_pix), 'rule': (max(n_rules, 1), n_pix),
                     'pix': (n_pix,)}[kind]
            out[f] = torch.empty(shape, dtype=_DTYPE[f], device=self.device)
        return out

    def analyze_tile(self, scene, params, values, valid=None, fields=ALL_FIELDS, out=None,
                     stream=None, lin=None, index=None):
        """values: [K, P] observation values — float64, or an index raster in its stored type
        (int16, uint16, int32, float32, uint8, ...: what index_tile writes) — valid: uint8 [K, P]
        or None. With lin (an IndexFn's linear form, fn.lin): values are the [K, NB, P] band
        planes and the kernel evaluates the index of each winner itself (the fused load stage).
        With index (an IndexFn of any program): the same, with the program inlined into JIT
        analyze / resolve kernels (lt_jit.h; compiled on first use, cached).
        Returns the dict of output tensors ([Y, P], [R, P], [P]); asynchronous on `stream`."""
        tin, tout, out = self._tile_structs(scene, params, values, valid, fields, out, lin, index)
        sc = scene.to_c()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        rc = self.lib.lt_analyze_tile(self.ctx, ctypes.byref(sc), ctypes.byref(params),
                                      ctypes.byref(tin), ctypes.byref(tout),
                                      ctypes.c_void_p(st.cuda_stream))
        self._check(rc, 'lt_analyze_tile')
        return out

    def analyze_tiles(self, scene, params, tiles, fields=ALL_FIELDS, outs=None, stream=None,
                      ready=None, lin=None, index=None, done=None, join=True):
        """analyze_tile over a list of (values, valid) tiles of one scene in one call
        (lt_analyze_tiles: tile t's resolve stage overlaps tile t+1's analyze stage). ready: None
        or one recorded torch.cuda.Event (or None) per tile, which that tile's analyze kernel
        waits on (lt_analyze_tiles_after: the load stage of later tiles may still be running on
        another stream). lin / index: as analyze_tile (every tile's values are then band planes).
        done: None or one torch.cuda.Event (or None) per tile, recorded once every output of that
        tile is complete; join=False: `stream` does not wait for the tiles' last stages
        (lt_analyze_tiles_ev: the caller orders later work on the done events).
        Returns the list of output dicts; asynchronous on `stream`."""
        n = len(tiles)
        tins = (_abi.LtTileIn * max(n, 1))()
        touts = (_abi.LtTileOut * max(n, 1))()
        res = []
        for t, (values, valid) in enumerate(tiles):
            tin, tout, o = self._tile_structs(scene, params, values, valid, fields,
                                              outs[t] if outs is not None else None, lin, index)
            tins[t] = tin
            touts[t] = tout
            res.append(o)
        sc = scene.to_c()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if done is not None or not join:
            if done is not None and len(done) != n:
                raise LtError('done needs one event (or None) per tile')
            if ready is not None and len(ready) != n:
                raise LtError('ready needs one event (or None) per tile')
            evr = (ctypes.c_void_p * max(n, 1))(
                *[e.cuda_event if e is not None else None for e in (ready or [None] * n)])
            evd = (ctypes.c_void_p * max(n, 1))(
                *[e.cuda_event if e is not None else None for e in (done or [None] * n)])
            rc = self.lib.lt_analyze_tiles_ev(self.ctx, ctypes.byref(sc), ctypes.byref(params), n,
                                              tins, touts, evr, evd, 1 if join else 0,
                                              ctypes.c_void_p(st.cuda_stream))
        elif ready is None:
            rc = self.lib.lt_analyze_tiles(self.ctx, ctypes.byref(sc), ctypes.byref(params), n,
                                           tins, touts, ctypes.c_void_p(st.cuda_stream))
        else:
            if len(ready) != n:
                raise LtError('ready needs one event (or None) per tile')
            evs = (ctypes.c_void_p * max(n, 1))(
                *[e.cuda_event if e is not None else None for e in ready])
            rc = self.lib.lt_analyze_tiles_after(self.ctx, ctypes.byref(sc), ctypes.byref(params),
                                                 n, tins, touts, evs,
                                                 ctypes.c_void_p(st.cuda_stream))
        self._check(rc, 'lt_analyze_tiles')
        return res

    def _tile_structs(self, scene, params, values, valid, fields, out, lin=None, index=None):
        if index is not None:  # any program, JIT kernels: its band type and band count
            nb = len(index.program.bands)
            want = _TORCH_OF_LT[_LT_T_OF_NP(index.program.band_dtype)]
        elif lin is not None:
            nb, want = lin.n_bands, _TORCH_OF_LT.get(lin.band_type)
        if lin is not None or index is not None:  # the fused load stage: [K, NB, P] band planes
            planar = values.dim() == 3 and values.stride(2) == 1
            inter = values.dim() == 3 and values.stride(1) == 1 and values.stride(2) == nb
            if (values.dtype != want or values.device != self.device or values.dim() != 3 or
                    values.shape[1] != nb or not (planar or inter)):
                raise LtError('bands must be a %s [K, %d, P] tensor on %s, planar (unit pixel '
                              'stride) or pixel-interleaved (unit band stride)'
                              % (want, nb, self.device))
            K, _, P = values.shape
        else:
            if values.dtype not in _LT_T or values.device != self.device or values.dim() != 2:
                raise LtError('values must be a [K, P] raster tensor on %s' % self.device)
            if values.stride(1) != 1:
                raise LtError('values must have unit pixel stride')
            K, P = values.shape
        if K != scene.n_obs:
            raise LtError('values has %d obs rows, scene has %d' % (K, scene.n_obs))
        if valid is not None and valid.dtype == torch.int32:  # mask bit planes
            W = (K + 31) // 32
            if (tuple(valid.shape) != (W, P) or valid.stride(1) != 1 or
                    valid.device != self.device):
                raise LtError('valid bit planes must be an int32 [%d, P] tensor with unit pixel '
                              'stride' % W)
            if lin is None and index is None and W > 1 and valid.stride(0) != values.stride(0):
                raise LtError('valid bit planes must share the row stride of values')
        elif valid is not None:
            if lin is not None or index is not None:
                if (valid.dtype != torch.uint8 or tuple(valid.shape) != (K, P) or
                        valid.stride(1) != 1 or valid.device != self.device):
                    raise LtError('valid must be a uint8 [K, P] tensor with unit pixel stride')
            elif (valid.dtype != torch.uint8 or valid.shape != values.shape or
                    valid.stride() != values.stride() or valid.device != self.device):
                raise LtError('valid must be uint8 with the shape/strides of values')
        if out is None:
            out = self.alloc_outputs(scene.n_years, params.n_rules, P, fields)
        ostride = None
        for f, t in out.items():
            kind = _SHAPE_KIND[f]
            if t.device != self.device or t.dtype != _DTYPE[f] or t.shape[-1] < P:
                raise LtError('output %s has wrong device/dtype/shape' % f)
            if kind != 'pix':
                need = scene.n_years if kind == 'year' else params.n_rules
                if t.shape[0] < need or t.stride(1) != 1:
                    raise LtError('output %s too small' % f)
                s = t.stride(0)
                if ostride is None:
                    ostride = s
                elif s != ostride:
                    raise LtError('all [Y|R, P] outputs must share one row stride')
        tin = _abi.LtTileIn()
        tin.n_pix = P
        if lin is not None or index is not None:
            tin.stride = valid.stride(0) if valid is not None and valid.shape[0] > 1 else P
            tin.obs_bands = values.data_ptr()
            tin.band_obs_stride = values.stride(0)
            tin.band_stride = values.stride(1)
            tin.band_pix_stride = values.stride(2)
            if index is not None:
                tin.index = index.handle
            else:
                tin.lin = lin
        elif values.dtype == torch.float64:
            tin.stride = values.stride(0)
            tin.obs_val = ctypes.cast(values.data_ptr(), _abi.c_f64p)
        else:
            tin.stride = values.stride(0)
            tin.obs_index = values.data_ptr()
            tin.index_type = _LT_T[values.dtype]
        if valid is not None and valid.dtype == torch.int32:
            tin.obs_valid_bits = valid.data_ptr()
        else:
            tin.obs_valid = (ctypes.cast(valid.data_ptr(), _abi.c_u8p) if valid is not None
                             else None)
        tout = _abi.LtTileOut()
        tout.stride = ostride if ostride is not None else P
        for f, t in out.items():
            setattr(tout, f, ctypes.cast(t.data_ptr(), type(getattr(tout, f))))
        return tin, tout, out

    # --- fit to vertex: an analysis's segments on a second index (lt_ftv_tile, lt_ftv.hip) ---
    def ftv_tile(self, scene, winner, spike, vertex, values, fields=FTV_FIELDS, out=None,
                 stream=None):
        """The spikes and vertices of an analysis applied to a second index (vertices2eqns +
        eqns2fitted_points on given planes). winner int16 / spike uint8 / vertex uint8: [Y, P]
        tensors as analyze_tile wrote them, unit pixel stride, one shared row stride >= P.
        values: [K, P] float64, or an index raster in its stored type (what index_tile writes).
        Returns the dict of device tensors: the requested `fields` of FTV_FIELDS ([Y, P]
        float64) and 'status' ([P] int32); asynchronous on `stream`. out: tensors to fill instead
        (exactly the planes to write: [Y, >= P] float64 sharing one row stride, 'status' [>= P])."""
        Y, K = scene.n_years, scene.n_obs
        if (not isinstance(winner, torch.Tensor) or winner.dim() != 2 or
                winner.dtype != torch.int16 or winner.device != self.device or
                winner.shape[0] != Y or (winner.shape[1] > 1 and winner.stride(1) != 1)):
            raise LtError('winner must be an int16 [%d, P] tensor on %s with unit pixel stride'
                          % (Y, self.device))
        P = winner.shape[1]
        istride = winner.stride(0) if Y > 1 else max(P, 1)
        if istride < P:
            raise LtError('winner rows must not overlap')
        for name, t in (('spike', spike), ('vertex', vertex)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or
                    t.device != self.device or t.shape != winner.shape or
                    (P > 1 and t.stride(1) != 1) or (Y > 1 and t.stride(0) != istride)):
                raise LtError('%s must be uint8 with the shape and row stride of winner' % name)
        if (not isinstance(values, torch.Tensor) or values.dtype not in _LT_T or
                values.device != self.device or values.dim() != 2 or
                tuple(values.shape) != (K, P) or (P > 1 and values.stride(1) != 1)):
            raise LtError('values must be a [%d, %d] raster tensor on %s with unit pixel stride'
                          % (K, P, self.device))
        vstride = values.stride(0) if K > 1 else max(P, 1)
        if vstride < P:
            raise LtError('values rows must not overlap')
        if out is None:
            bad = [f for f in fields if f not in FTV_FIELDS]
            if bad:
                raise LtError('ftv_tile writes %s, not %s' % (', '.join(FTV_FIELDS), bad))
            out = self.alloc_outputs(Y, 0, P, tuple(fields) + ('status',))
        ostride = None
        for f, t in out.items():
            if f not in FTV_FIELDS and f != 'status':
                raise LtError('ftv_tile writes %s and status, not %s' % (', '.join(FTV_FIELDS), f))
            if (not isinstance(t, torch.Tensor) or t.device != self.device or
                    t.dtype != _DTYPE[f] or t.shape[-1] < P):
                raise LtError('output %s has wrong device/dtype/shape' % f)
            if f == 'status':
                if t.dim() != 1 or (t.numel() > 1 and t.stride(0) != 1):
                    raise LtError('output status must be a [P] tensor with unit stride')
                continue
            if t.dim() != 2 or t.shape[0] < Y or (t.shape[1] > 1 and t.stride(1) != 1):
                raise LtError('output %s too small' % f)
            s = t.stride(0) if t.shape[0] > 1 else max(P, 1)
            if s < P:
                raise LtError('output %s rows must not overlap' % f)
            if ostride is None:
                ostride = s
            elif s != ostride:
                raise LtError('all [Y, P] outputs must share one row stride')
        fin = _abi.LtFtvIn()
        fin.n_pix, fin.stride, fin.obs_stride = P, istride, vstride
        fin.winner = ctypes.cast(winner.data_ptr(), _abi.c_i16p)
        fin.spike = ctypes.cast(spike.data_ptr(), _abi.c_u8p)
        fin.vertex = ctypes.cast(vertex.data_ptr(), _abi.c_u8p)
        if values.dtype == torch.float64:
            fin.obs_val = ctypes.cast(values.data_ptr(), _abi.c_f64p)
        else:
            fin.obs_index = values.data_ptr()
            fin.index_type = _LT_T[values.dtype]
        tout = _abi.LtTileOut()
        tout.stride = ostride if ostride is not None else max(P, 1)
        for f, t in out.items():
            setattr(tout, f, ctypes.cast(t.data_ptr(), type(getattr(tout, f))))
        sc = scene.to_c()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        rc = self.lib.lt_ftv_tile(self.ctx, ctypes.byref(sc), ctypes.byref(fin),
                                  ctypes.byref(tout), ctypes.c_void_p(st.cuda_stream))
        self._check(rc, 'lt_ftv_tile')
        return out

    # --- vertex table: a trendline as one row per vertex (lt_vertex_table, lt_vertex.hip) ---
    def vertex_table(self, years, val_fit, vertex, present=None, winner=None, val_raw=None,
                     max_vertices=None, out=None, stream=None):
        """Each pixel's vertices compacted from its per-year planes. years: the calendar year of
        each of the Y slots. val_fit float64 / vertex uint8: [Y, P] device tensors with unit
        pixel stride and one shared row stride >= P; val_raw (float64), present (uint8, 0 = no
        point in the slot) and winner (int16, a point iff >= 0) likewise, each optional, at most
        one of present / winner. The first slot that holds a point is vertex 0, every later
        flagged one the next. Returns the dict of device tensors: 'n_vertices' [P] int32 (the full
        count), 'vertex_year' [V, P] int32, 'vertex_fit' [V, P] float64 and, with val_raw,
        'vertex_raw' [V, P] float64, LT_NODATA from a pixel's count on; V = max_vertices
        (default Y). out: tensors to fill instead (exactly the planes to write: [>= V, >= P]
        sharing one row stride, of which V rows are written; 'n_vertices' [>= P]). Asynchronous
        on `stream`."""
        import numpy as np
        if (not isinstance(val_fit, torch.Tensor) or val_fit.dim() != 2 or
                val_fit.dtype != torch.float64 or val_fit.device != self.device or
                (val_fit.shape[1] > 1 and val_fit.stride(1) != 1)):
            raise LtError('val_fit must be a float64 [Y, P] tensor on %s with unit pixel stride'
                          % self.device)
        Y, P = val_fit.shape
        istride = val_fit.stride(0) if Y > 1 else max(P, 1)
        if istride < P:
            raise LtError('val_fit rows must not overlap')
        if present is not None and winner is not None:
            raise LtError('at most one of present / winner')
        for name, t, dt in (('vertex', vertex, torch.uint8), ('present', present, torch.uint8),
                            ('winner', winner, torch.int16), ('val_raw', val_raw, torch.float64)):
            if t is None and name != 'vertex':
                continue
            if (not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != self.device or
                    t.shape != val_fit.shape or (P > 1 and t.stride(1) != 1) or
                    (Y > 1 and t.stride(0) != istride)):
                raise LtError('%s must be %s with the shape and row stride of val_fit'
                              % (name, str(dt).split('.')[-1]))
        yrs = np.ascontiguousarray(np.asarray(years, np.int32))
        if yrs.ndim != 1 or len(yrs) != Y:
            raise LtError('years must have one entry per slot')
        if Y > _abi.LT_MAX_YEARS:
            raise LtError('more than %d year slots' % _abi.LT_MAX_YEARS)
        V = Y if max_vertices is None else int(max_vertices)
        if not 1 <= V <= _abi.LT_MAX_YEARS:
            raise LtError('max_vertices must be in [1, %d]' % _abi.LT_MAX_YEARS)
        dts = {f: _DT[d] for f, d in _abi.VERTEX_FIELDS}
        if out is None:
            out = {f: torch.empty((P,) if f == 'n_vertices' else (V, P), dtype=dt,
                                  device=self.device)
                   for f, dt in dts.items() if f != 'vertex_raw' or val_raw is not None}
        ostride = None
        for f, t in out.items():
            if f not in dts:
                raise LtError('vertex_table writes %s, not %s' % (', '.join(dts), f))
            if f == 'vertex_raw' and val_raw is None:
                raise LtError('vertex_raw needs val_raw')
            if (not isinstance(t, torch.Tensor) or t.device != self.device or
                    t.dtype != dts[f] or t.shape[-1] < P):
                raise LtError('output %s has wrong device/dtype/shape' % f)
            if f == 'n_vertices':
                if t.dim() != 1 or (t.numel() > 1 and t.stride(0) != 1):
                    raise LtError('output n_vertices must be a [P] tensor with unit stride')
                continue
            if t.dim() != 2 or t.shape[0] < V or (t.shape[1] > 1 and t.stride(1) != 1):
                raise LtError('output %s too small' % f)
            s = t.stride(0) if t.shape[0] > 1 else max(P, 1)
            if s < P:
                raise LtError('output %s rows must not overlap' % f)
            if ostride is None:
                ostride = s
            elif s != ostride:
                raise LtError('all [V, P] outputs must share one row stride')
        vin = _abi.LtVertexIn()
        vin.n_pix, vin.stride, vin.n_years = P, istride, Y
        vin.year = yrs.ctypes.data_as(_abi.c_i32p)
        for f, t in (('val_fit', val_fit), ('vertex', vertex), ('val_raw', val_raw),
                     ('present', present), ('winner', winner)):
            if t is not None:
                setattr(vin, f, ctypes.cast(t.data_ptr(), type(getattr(vin, f))))
        vout = _abi.LtVertexOut()
        vout.stride = ostride if ostride is not None else max(P, 1)
        vout.max_vertices = V
        for f, t in out.items():
            setattr(vout, f, ctypes.cast(t.data_ptr(), type(getattr(vout, f))))
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        rc = self.lib.lt_vertex_table(self.ctx, ctypes.byref(vin), ctypes.byref(vout),
                                      ctypes.c_void_p(st.cuda_stream))
        self._check(rc, 'lt_vertex_table')
        return out

    # --- change maps: loss / gain maps of a trendline (lt_change_maps, lt_change.hip) ---
    def change_maps(self, years, rules, val_fit, vertex, present=None, winner=None, val_raw=None,
                    spike=None, out=None, stream=None):
        """The change maps of every pixel, all of them in one pass over its per-year planes.
        years: the calendar year of each of the Y slots. rules: 1 to 8 maps, each a dict as
        settings.change_map_options gives it ('delta', and optionally 'sort', 'index_sign',
        'year', 'mag', 'dur', 'preval') or an _abi.LtChangeRule. val_fit float64 / vertex uint8:
        [Y, P] device tensors with unit pixel stride and one shared row stride >= P; present
        (uint8), winner (int16), val_raw (float64) and spike (uint8) likewise, each optional, at
        most one of present / winner. Returns the dict of device tensors: 'matched' uint8,
        'onset_year' / 'duration' int32, 'magnitude' / 'preval' / 'rate' float64, all [M, P] and
        LT_NODATA (matched 0) where no segment was kept, and, with val_raw and spike, 'dsnr'
        [M, P], 'rmse' [P] float64 and 'n_fit' [P] int32. out: tensors to fill instead (exactly
        the planes to write: the [M, P] ones [>= M, >= P] sharing one row stride, 'rmse' and
        'n_fit' [>= P]). Asynchronous on `stream`."""
        import numpy as np
        if (not isinstance(val_fit, torch.Tensor) or val_fit.dim() != 2 or
                val_fit.dtype != torch.float64 or val_fit.device != self.device or
                (val_fit.shape[1] > 1 and val_fit.stride(1) != 1)):
            raise LtError('val_fit must be a float64 [Y, P] tensor on %s with unit pixel stride'
                          % self.device)
        Y, P = val_fit.shape
        istride = val_fit.stride(0) if Y > 1 else max(P, 1)
        if istride < P:
            raise LtError('val_fit rows must not overlap')
        if present is not None and winner is not None:
            raise LtError('at most one of present / winner')
        for name, t, dt in (('vertex', vertex, torch.uint8), ('present', present, torch.uint8),
                            ('winner', winner, torch.int16), ('val_raw', val_raw, torch.float64),
                            ('spike', spike, torch.uint8)):
            if t is None and name != 'vertex':
                continue
            if (not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != self.device or
                    t.shape != val_fit.shape or (P > 1 and t.stride(1) != 1) or
                    (Y > 1 and t.stride(0) != istride)):
                raise LtError('%s must be %s with the shape and row stride of val_fit'
                              % (name, str(dt).split('.')[-1]))
        yrs = np.ascontiguousarray(np.asarray(years, np.int32))
        if yrs.ndim != 1 or len(yrs) != Y:
            raise LtError('years must have one entry per slot')
        if Y > _abi.LT_MAX_YEARS:
            raise LtError('more than %d year slots' % _abi.LT_MAX_YEARS)
        rules = list(rules)
        M = len(rules)
        if not 1 <= M <= _abi.LT_MAX_CHANGE_MAPS:
            raise LtError('1 to %d change maps' % _abi.LT_MAX_CHANGE_MAPS)
        try:
            crules = (_abi.LtChangeRule * M)(*[
                r if isinstance(r, _abi.LtChangeRule) else _abi.change_rule(r) for r in rules])
        except (KeyError, TypeError, IndexError, ValueError) as e:
            raise LtError('bad change map rule: %r' % (e,))
        fit = val_raw is not None and spike is not None
        map_dt = {f: _DT[d] for f, d in _abi.CHANGE_MAP_FIELDS}
        pix_dt = {f: _DT[d] for f, d in _abi.CHANGE_PIX_FIELDS}
        if out is None:
            out = {f: torch.empty((M, P), dtype=dt, device=self.device)
                   for f, dt in map_dt.items() if f != 'dsnr' or fit}
            if fit:
                out.update({f: torch.empty(P, dtype=dt, device=self.device)
                            for f, dt in pix_dt.items()})
        ostride = None
        for f, t in out.items():
            if f not in map_dt and f not in pix_dt:
                raise LtError('change_maps writes %s, not %s'
                              % (', '.join(list(map_dt) + list(pix_dt)), f))
            if f in ('dsnr', 'rmse', 'n_fit') and not fit:
                raise LtError('%s needs val_raw and spike' % f)
            dt = map_dt.get(f, pix_dt.get(f))
            if (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != dt or
                    t.shape[-1] < P):
                raise LtError('output %s has wrong device/dtype/shape' % f)
            if f in pix_dt:
                if t.dim() != 1 or (t.numel() > 1 and t.stride(0) != 1):
                    raise LtError('output %s must be a [P] tensor with unit stride' % f)
                continue
            if t.dim() != 2 or t.shape[0] < M or (t.shape[1] > 1 and t.stride(1) != 1):
                raise LtError('output %s too small' % f)
            s = t.stride(0) if t.shape[0] > 1 else max(P, 1)
            if s < P:
                raise LtError('output %s rows must not overlap' % f)
            if ostride is None:
                ostride = s
            elif s != ostride:
                raise LtError('all [M, P] outputs must share one row stride')
        cin = _abi.LtChangeIn()
        cin.n_pix, cin.stride, cin.n_years = P, istride, Y
        cin.year = yrs.ctypes.data_as(_abi.c_i32p)
        for f, t in (('val_fit', val_fit), ('vertex', vertex), ('val_raw', val_raw),
                     ('present', present), ('winner', winner), ('spike', spike)):
            if t is not None:
                setattr(cin, f, ctypes.cast(t.data_ptr(), type(getattr(cin, f))))
        cout = _abi.LtChangeOut()
        cout.stride = ostride if ostride is not None else max(P, 1)
        for f, t in out.items():
            setattr(cout, f, ctypes.cast(t.data_ptr(), type(getattr(cout, f))))
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        rc = self.lib.lt_change_maps(self.ctx, ctypes.byref(cin), M, crules, ctypes.byref(cout),
                                     ctypes.c_void_p(st.cuda_stream))
        self._check(rc, 'lt_change_maps')
        return out

    def label_counts(self, matched, key, key_lo, n_bins, out=None):
        """A label plane counted per key: matched uint8 [P] and key int32 [P], device tensors
        with unit stride. Returns an int64 [n_bins + 1] device tensor: element k the pixels with
        matched != 0 and key == key_lo + k, the last element the matched pixels whose key is
        outside [key_lo, key_lo + n_bins). n_bins is in [1, 256]. out: an int64 [n_bins + 1]
        tensor the counts are added to (the caller zeroes it). Runs on the current stream and
        does not synchronise."""
        for name, v in (('key_lo', key_lo), ('n_bins', n_bins)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise LtError('%s must be an integer' % name)
        if not 1 <= n_bins <= 256:
            raise LtError('n_bins must be in [1, 256]')
        if not -2 ** 31 <= key_lo <= 2 ** 31 - 1:
            raise LtError('key_lo must be an int32')
        if (not isinstance(matched, torch.Tensor) or matched.dtype != torch.uint8 or
                matched.device != self.device or matched.dim() != 1 or
                (matched.numel() > 1 and matched.stride(0) != 1)):
            raise LtError('matched must be a uint8 [P] tensor on %s with unit stride'
                          % self.device)
        P = matched.numel()
        if (not isinstance(key, torch.Tensor) or key.dtype != torch.int32 or
                key.device != self.device or key.dim() != 1 or key.numel() != P or
                (P > 1 and key.stride(0) != 1)):
            raise LtError('key must be an int32 [%d] tensor on %s with unit stride'
                          % (P, self.device))
        if out is None:
            out = torch.zeros(n_bins + 1, dtype=torch.int64, device=self.device)
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or
                out.device != self.device or out.dim() != 1 or out.numel() != n_bins + 1 or
                out.stride(0) != 1):
            raise LtError('out must be an int64 [n_bins + 1] tensor on %s' % self.device)
        if P == 0:
            return out
        st = torch.cuda.current_stream(self.device)
        rc = self.lib.lt_label_counts(self.ctx, matched.data_ptr(), key.data_ptr(), P, key_lo,
                                      n_bins, out.data_ptr(), ctypes.c_void_p(st.cuda_stream))
        self._check(rc, 'lt_label_counts')
        return out

    # --- zonal table: a label plane summed per zone and key (lt_zonal_stats, lt_zonal.hip) ---
    def zonal_stats(self, matched, zone, key, key_lo, n_bins, n_zones, duration=None, value=None,
                    out=None, _path=0):
        """A label plane summed per zone and key: matched uint8 [P], zone int32 [P] (a dense zone
        index), key int32 [P] and, optionally, duration int32 [P] and value float64 [P], device
        tensors with unit stride. Returns an int64 [n_zones + 1, n_bins + 1, 4] device tensor: for
        the pixels with matched != 0, row zone (the last row for an index outside [0, n_zones)),
        column key - key_lo (the last column for a key outside [key_lo, key_lo + n_bins)), the
        four words hold the pixel count, the sum of duration, the sum of rint(clamp(value, -2^30,
        2^30) * 16) over the values that are not NaN, and the count of those (a mean magnitude is
        word 2 / 16 / word 3). n_bins is in [1, 256], n_zones in [1, 65536]. Without duration /
        value their words are left as they are. out: an int64 [n_zones + 1, n_bins + 1, 4] tensor
        the sums are added to (the caller zeroes it). Integer sums: the table is a function of
        the input alone. Runs on the current stream and does not synchronise."""
        for name, v in (('key_lo', key_lo), ('n_bins', n_bins), ('n_zones', n_zones),
                        ('_path', _path)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise LtError('%s must be an integer' % name)
        if not 1 <= n_bins <= 256:
            raise LtError('n_bins must be in [1, 256]')
        if not 1 <= n_zones <= _abi.LT_MAX_ZONES:
            raise LtError('n_zones must be in [1, %d]' % _abi.LT_MAX_ZONES)
        if not -2 ** 31 <= key_lo <= 2 ** 31 - 1:
            raise LtError('key_lo must be an int32')
        if _path not in (0, 1, 2):
            raise LtError('_path must be 0, 1 or 2')
        if (not isinstance(matched, torch.Tensor) or matched.dtype != torch.uint8 or
                matched.device != self.device or matched.dim() != 1 or
                (matched.numel() > 1 and matched.stride(0) != 1)):
            raise LtError('matched must be a uint8 [P] tensor on %s with unit stride'
                          % self.device)
        P = matched.numel()
        for name, t, dt, need in (('zone', zone, torch.int32, True), ('key', key, torch.int32, True),
                                  ('duration', duration, torch.int32, False),
                                  ('value', value, torch.float64, False)):
            if t is None and not need:
                continue
            if (not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != self.device or
                    t.dim() != 1 or t.numel() != P or (P > 1 and t.stride(0) != 1)):
                raise LtError('%s must be a [%d] tensor of %s on %s with unit stride'
                              % (name, P, str(dt).replace('torch.', ''), self.device))
        shape = (n_zones + 1, n_bins + 1, 4)
        if out is None:
            out = torch.zeros(shape, dtype=torch.int64, device=self.device)
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or
                out.device != self.device or tuple(out.shape) != shape or not out.is_contiguous()):
            raise LtError('out must be a contiguous int64 [n_zones + 1, n_bins + 1, 4] tensor on %s'
                          % self.device)
        if P == 0:
            return out
        st = torch.cuda.current_stream(self.device)
        rc = self.lib.lt_zonal_stats(
            self.ctx, matched.data_ptr(), zone.data_ptr(), key.data_ptr(),
            duration.data_ptr() if duration is not None else None,
            value.data_ptr() if value is not None else None, P, key_lo, n_bins, n_zones, _path,
            out.data_ptr(), ctypes.c_void_p(st.cuda_stream))
        self._check(rc, 'lt_zonal_stats')
        return out

    # --- MMU sieve: patches of a label plane below a minimum size (lt_sieve_labels) ---
    def sieve(self, matched, key, shape, min_pixels, connectivity=8, apply=True, out=None,
              _phases=None):
        """Connected-component labelling of one label plane and the minimum mapping unit.
        matched: uint8 [P] device tensor with unit stride over a shape = (rows, cols) raster
        (P = rows * cols, row-major); key: int32 [P] likewise, or None (one key for all). A patch
        is a maximal 4- or 8-connected set of pixels with matched != 0 and one key. Returns
        {'root', 'size'}: int32 [P] device tensors, the smallest raster index of the pixel's patch
        (-1 where unmatched) and its pixel count (0 where unmatched); with apply, matched is
        cleared in place wherever 0 < size < min_pixels (a patch of exactly min_pixels stays).
        key is never written. out: {'root', 'size'} tensors to fill instead. Runs on the current
        stream and does not synchronise; the workspace (8 bytes a pixel) is allocated per call on
        that stream."""
        try:
            rows, cols = (int(v) for v in shape)
        except (TypeError, ValueError):
            raise LtError('shape must be (rows, cols)')
        if rows < 0 or cols < 0:
            raise LtError('shape must not be negative')
        P = rows * cols

        def plane(name, t, dt):
            if (not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != self.device or
                    t.dim() != 1 or t.numel() != P or (P > 1 and t.stride(0) != 1)):
                raise LtError('%s must be a %s [%d] tensor on %s with unit stride'
                              % (name, str(dt).split('.')[-1], P, self.device))
        plane('matched', matched, torch.uint8)
        if key is not None:
            plane('key', key, torch.int32)
        for name, v in (('min_pixels', min_pixels), ('connectivity', connectivity)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise LtError('%s must be an integer' % name)
        if connectivity not in (4, 8):
            raise LtError('connectivity must be 4 or 8')
        if not 1 <= min_pixels <= 2 ** 31 - 1:
            raise LtError('min_pixels must be in [1, 2^31 - 1]')
        if out is None:
            out = {f: torch.empty(P, dtype=torch.int32, device=self.device)
                   for f in ('root', 'size')}
        if set(out) != {'root', 'size'}:
            raise LtError('sieve writes root and size, not %s' % ', '.join(sorted(out)))
        for f, t in out.items():
            plane('output ' + f, t, torch.int32)
        if P == 0:
            return out
        nbytes = self.lib.lt_sieve_workspace_bytes(rows, cols)
        if nbytes < 0:
            raise LtError('raster of %d x %d pixels is above the limit' % (rows, cols))
        if _phases is None:
            work, phases = torch.empty(nbytes // 4, dtype=torch.int32, device=self.device), 0
        else:  # tools/sieve_rate.py: (a workspace kept between calls, the launches to run)
            work, phases = _phases
        sin = _abi.LtSieveIn()
        sin.rows, sin.cols = rows, cols
        sin.matched = ctypes.cast(matched.data_ptr(), _abi.c_u8p)
        if key is not None:
            sin.key = ctypes.cast(key.data_ptr(), _abi.c_i32p)
        sin.connectivity, sin.min_pixels, sin.apply = connectivity, min_pixels, int(bool(apply))
        sin.phases = phases
        sout = _abi.LtSieveOut()
        sout.root = ctypes.cast(out['root'].data_ptr(), _abi.c_i32p)
        sout.size = ctypes.cast(out['size'].data_ptr(), _abi.c_i32p)
        sout.workspace, sout.workspace_bytes = work.data_ptr(), nbytes
        st = torch.cuda.current_stream(self.device)
        rc = self.lib.lt_sieve_labels(self.ctx, ctypes.byref(sin), ctypes.byref(sout),
                                      ctypes.c_void_p(st.cuda_stream))
        self._check(rc, 'lt_sieve_labels')
        return out

    # --- load stage: index_eqn (rast_algebra, utils.py:447-484) ---
    def compile_index(self, program):
        """hiprtc-compile an index_eqn.IndexProgram for this device (cached per program). A
        program with an integer linear form is evaluated inside the analyze kernels, so its load
        kernel is compiled only when something asks for an index raster (IndexFn.handle): a
        job's analysis did not need the ~0.1 s."""
        def build():
            fn = ctypes.c_void_p()
            prog = program.to_c()
            with torch.cuda.device(self.device):
                self._check(self.lib.lt_index_compile(self.ctx, ctypes.byref(prog),
                                                      ctypes.byref(fn)), 'lt_index_compile')
            return fn
        lin = linear_form(program)
        if lin is not None:
            return IndexFn(None, program, lin, build=build)
        return IndexFn(build(), program, lin)

    def index_tile(self, fn, bands, out=None, stream=None):
        """bands: [K, NB, P] band planes (NB = the program's band slots; unit pixel stride, or
        pixel-interleaved: band stride 1, pixel stride NB) in the program's band type; returns the
        [K, P] index raster in the program's output type."""
        prog = fn.program
        want = _TORCH_OF_LT[_LT_T_OF_NP(prog.band_dtype)]
        if bands.dim() != 3 or bands.dtype != want or bands.device != self.device:
            raise LtError('bands must be a %s [K, %d, P] tensor on %s' % (want, len(prog.bands),
                                                                         self.device))
        K, NB, P = bands.shape
        if NB != len(prog.bands):
            raise LtError('bands must have %d band planes' % len(prog.bands))
        # planar ([K, NB, P], unit pixel stride) or pixel-interleaved (band stride 1, pixel stride
        # NB: lt_index_kernel4i reads a 4-pixel group's bands with NB vector loads)
        inter = bands.stride(1) == 1 and bands.stride(2) == NB and NB > 1
        if bands.stride(2) != 1 and not inter:
            bands = bands.contiguous()
        odt = _TORCH_OF_LT[_LT_T_OF_NP(prog.out_dtype)]
        if out is None:
            out = torch.empty((K, P), dtype=odt, device=self.device)
        if out.dtype != odt or out.shape[0] < K or out.shape[1] < P or out.stride(1) != 1:
            raise LtError('out must be a %s [K, P] tensor' % odt)
        io = _abi.LtIndexIO()
        io.n_pix, io.n_obs = P, K
        # (one band plane: its band stride is never used; the obs stride stands in)
        io.obs_stride = bands.stride(0)
        io.band_stride = bands.stride(1) if NB > 1 else bands.stride(0)
        io.band_pix_stride = bands.stride(2)
        io.out_stride = out.stride(0)
        io.bands, io.out = bands.data_ptr(), out.data_ptr()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._check(self.lib.lt_index_apply(self.ctx, fn.handle, ctypes.byref(io),
                                            ctypes.c_void_p(st.cuda_stream)), 'lt_index_apply')
        return out

    # --- mask stage: mask_eqn (rast_algebra's mask_eqn, utils.py:447-484; lt_mask.h) ---
    def compile_mask(self, program):
        """hiprtc-compile an index_eqn.MaskProgram for this device (cached per program)."""
        fn = ctypes.c_void_p()
        prog = program.to_c()
        with torch.cuda.device(self.device):
            self._check(self.lib.lt_mask_compile(self.ctx, ctypes.byref(prog), ctypes.byref(fn)),
                        'lt_mask_compile')
        return MaskFn(fn, program)

    def apply_mask(self, fn, bands, valid, dropped=None, stream=None):
        """valid[k, p] &= mask_eqn on the bands of obs k at pixel p, in place. bands: [K, NB, P]
        planes in the program's band type (NB = len(program.band_numbers); any strides: a view of
        a larger stack, pixel-interleaved, ...); valid: uint8 [K, P] with unit pixel stride (its
        row stride may exceed P). dropped: an int64 [1] device tensor the number of bytes cleared
        is added to. Asynchronous on `stream`; returns valid."""
        prog = fn.program
        want = _TORCH_OF_LT[_LT_T_OF_NP(prog.band_dtype)]
        NB = len(prog.band_numbers)
        if (bands.dim() != 3 or bands.dtype != want or bands.device != self.device or
                bands.shape[1] != NB):
            raise LtError('bands must be a %s [K, %d, P] tensor on %s' % (want, NB, self.device))
        K, _, P = bands.shape
        if (valid.dim() != 2 or valid.dtype != torch.uint8 or valid.device != self.device or
                tuple(valid.shape) != (K, P) or (P > 1 and valid.stride(1) != 1) or
                (K > 1 and valid.stride(0) < P)):
            raise LtError('valid must be a uint8 [%d, %d] tensor on %s with unit pixel stride'
                          % (K, P, self.device))
        if K > 65535:
            raise LtError('at most 65535 observations')
        if dropped is not None and (dropped.dtype != torch.int64 or dropped.numel() != 1 or
                                    dropped.device != self.device):
            raise LtError('dropped must be an int64 tensor of one element on %s' % self.device)
        if K == 0 or P == 0:
            return valid
        io = _abi.LtMaskIO()
        io.n_pix, io.n_obs = P, K
        io.obs_stride, io.band_stride = bands.stride(0), bands.stride(1)
        io.band_pix_stride = bands.stride(2) if P > 1 else 1
        io.bands, io.valid = bands.data_ptr(), valid.data_ptr()
        io.valid_stride = valid.stride(0) if K > 1 else P
        io.dropped = dropped.data_ptr() if dropped is not None else None
        if min(io.obs_stride, io.band_stride) < 0 or io.band_pix_stride < 1:
            raise LtError('bands must have positive pixel stride and non-negative strides')
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._check(self.lib.lt_mask_apply(self.ctx, fn.handle, ctypes.byref(io),
                                           ctypes.c_void_p(st.cuda_stream)), 'lt_mask_apply')
        return valid

    # --- output raster assembly (output_reducer -> data2raster, lt_raster_assemble) ---
    def raster_assemble(self, jobs, stream=None):
        """jobs: a list of _abi.LtRasterJob (device pointers of this engine's tensors, which the
        caller keeps alive until the stream has run them)."""
        if not jobs:
            return
        arr = (_abi.LtRasterJob * len(jobs))(*jobs)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._check(self.lib.lt_raster_assemble(self.ctx, arr, len(jobs),
                                                ctypes.c_void_p(st.cuda_stream)),
                    'lt_raster_assemble')

    # --- ingest: TIFF strips decoded on the device (lt_tiff_decode_strips_dev, lt_chunks.hip) ---
    def decode_strips(self, jobs, stream=None):
        """Every strip of len(jobs) strip-organised TIFF images whose compressed bytes are in
        device memory, decoded by the HIP strip decoder in one call. A job is a dict:
          file      uint8 device tensor: the bytes that hold every strip (the file or a slice);
          offsets, counts  int64 (or uint64) device tensors [n_strips], offsets relative to file;
          compression (1 or 5), predictor (1 or 2), planar (1 or 2), rows_per_strip;
          dtype     the numpy sample type as stored (its byte order is the file's);
          width, height, bands;
          out       optional contiguous [bands, height, width] device tensor to fill.
        Returns (the list of [bands, height, width] tensors, native byte order; the int32 error
        words, one per job: 0, or the LT_IO_ERR_* of a failing strip once the stream has run).
        Asynchronous on `stream`; the caller keeps the input tensors alive until it has run."""
        def fill(a, j, n_strips):
            a.n_strips, a.compression = n_strips, int(j['compression'])
            a.rows_per_strip = int(j['rows_per_strip'])
        return self._decode_jobs('decode_strips', _abi.LtStripsJob, fill,
                                 'lt_tiff_decode_strips_dev', jobs, stream)

    # --- ingest: TIFF tiles and Deflate decoded on the device (lt_tiff_decode_chunks_dev) ---
    def decode_chunks(self, jobs, stream=None):
        """decode_strips for strips or tiles, uncompressed, LZW or Deflate (the HIP chunk decoder,
        lt_chunks.hip). A job is decode_strips's dict with, instead of rows_per_strip:
          compression  1, 5, 8 or 32946 (Deflate);
          chunk_w, chunk_h  the tile size, or the image's width and the rows per strip;
          tiled        whether the offsets are tiles (all full size) or strips.
        Same return, same error words (one per job), same asynchrony and lifetime rules."""
        def fill(a, j, n_chunks):
            comp = int(j['compression'])
            a.n_chunks, a.compression = n_chunks, 8 if comp == 32946 else comp
            a.chunk_w, a.chunk_h = int(j['chunk_w']), int(j['chunk_h'])
            a.tiled = 1 if j['tiled'] else 0
        return self._decode_jobs('decode_chunks', _abi.LtChunksJob, fill,
                                 'lt_tiff_decode_chunks_dev', jobs, stream)

    def _decode_jobs(self, what, struct, fill, entry, jobs, stream):
        """decode_strips's and decode_chunks's common part: the outputs and error words made on
        the stream, the checks of out / file / offsets / counts, the fields the two job structs
        share, fill(a, j) for the others, then the library call `entry` under the decode lock."""
        import numpy as np
        n = len(jobs)
        arr = (struct * max(n, 1))()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):  # (tensors made here belong to the stream that fills them)
            err = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)  # zeroed by the call
            made = [torch.empty((int(j['bands']), int(j['height']), int(j['width'])),
                                dtype=torch.from_numpy(
                                    np.empty(0, np.dtype(j['dtype']).newbyteorder('='))).dtype,
                                device=self.device) if j.get('out') is None else None
                    for j in jobs]
        outs = []
        for k, j in enumerate(jobs):
            dt = np.dtype(j['dtype'])
            tdt = torch.from_numpy(np.empty(0, dt.newbyteorder('='))).dtype
            shape = (int(j['bands']), int(j['height']), int(j['width']))
            out = j.get('out') if j.get('out') is not None else made[k]
            if (tuple(out.shape) != shape or out.dtype != tdt or out.device != self.device or
                    not out.is_contiguous()):
                raise LtError('%s: out must be a contiguous %s %s tensor on %s'
                              % (what, tdt, shape, self.device))
            f, offs, cnts = j['file'], j['offsets'], j['counts']
            if (f.dtype != torch.uint8 or f.dim() != 1 or not f.is_contiguous() or
                    f.device != self.device):
                raise LtError('%s: file must be a contiguous uint8 tensor on %s'
                              % (what, self.device))
            for t in (offs, cnts):
                if (t.dtype not in (torch.int64, torch.uint64) or t.dim() != 1 or
                        not t.is_contiguous() or t.device != self.device or
                        t.shape != offs.shape):
                    raise LtError('%s: offsets / counts must be contiguous 64-bit [n] tensors '
                                  'on %s' % (what, self.device))
            a = arr[k]
            a.file, a.file_size = f.data_ptr(), f.numel()
            a.offsets, a.counts = offs.data_ptr(), cnts.data_ptr()
            a.predictor = int(j['predictor'])
            a.bps = dt.itemsize
            a.big_endian = 1 if (dt.byteorder == '>' or
                                 (dt.byteorder == '=' and np.little_endian is False)) else 0
            a.width, a.height, a.bands = shape[2], shape[1], shape[0]
            a.planar = int(j['planar'])
            a.out = out.data_ptr()
            a.err = err.data_ptr() + 4 * k
            fill(a, j, offs.numel())
            outs.append(out)
        with self._decode_lock:  # one context: one caller at a time (ingest decodes on threads)
            self._check(getattr(self.lib, entry)(self.ctx, arr, n,
                                                 ctypes.c_void_p(st.cuda_stream)), entry)
        return outs, err[:n]

    # --- output: TIFF strips encoded on the device (lt_tiff_encode_strips_dev, lt_encode.hip) ---
    def encode_strips(self, jobs, stream=None):
        """The LZW / uncompressed strips of len(jobs) rasters in device memory, encoded by the HIP
        strip encoder in one call: tiffcodec.encode_strips's bytes and sizes. A job is a dict:
          data      contiguous device tensor [bands, rows, cols] or [rows, cols] (1, 2, 4 or 8
                    byte samples; never written);
          rows_per_strip, compression (1 or 5), predictor (1 or 2; 2 for integer samples);
          out       optional uint8 device tensor to fill (default: the worst case);
          cap       optional: only the first cap bytes of out are offered.
        Returns, per job, (out uint8 tensor, strip_sizes int64 tensor, total int64 tensor of one
        element: the bytes in out, or a negative LT_IO_ERR_*, LT_IO_ERR_SPACE when cap is too
        small). Asynchronous on `stream`; the caller keeps `data` alive until it has run."""
        n = len(jobs)
        arr = (_abi.LtEncodeJob * max(n, 1))()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        res = []
        for k, j in enumerate(jobs):
            d = j['data']
            if (not isinstance(d, torch.Tensor) or d.device != self.device or
                    d.dim() not in (2, 3) or not d.is_contiguous() or d.numel() == 0 or
                    d.is_complex() or d.element_size() not in (1, 2, 4, 8)):
                raise LtError('encode_strips: data must be a contiguous [bands, rows, cols] or '
                              '[rows, cols] tensor of 1, 2, 4 or 8 byte samples on %s'
                              % self.device)
            nb, rows, cols = (1,) + tuple(d.shape) if d.dim() == 2 else tuple(d.shape)
            rps, comp, pred = (int(j['rows_per_strip']), int(j['compression']),
                               int(j.get('predictor', 1)))
            if rps <= 0 or comp not in (1, 5) or pred not in (1, 2):
                raise LtError('encode_strips: rows_per_strip > 0, compression 1 or 5, '
                              'predictor 1 or 2')
            if pred == 2 and d.is_floating_point():
                raise LtError('encode_strips: predictor 2 is for integer samples')
            ns = nb * (-(-rows // rps))
            raw = nb * rows * cols * d.element_size()
            out = j.get('out')
            with torch.cuda.stream(st):  # (tensors made here belong to the stream that fills them)
                if out is None:
                    out = torch.empty(raw * 3 // 2 + 16 * ns + 16 if comp == 5 else raw,
                                      dtype=torch.uint8, device=self.device)
                meta = torch.empty(ns + 1, dtype=torch.int64, device=self.device)
            if (out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or
                    out.device != self.device):
                raise LtError('encode_strips: out must be a contiguous uint8 tensor on %s'
                              % self.device)
            cap = int(j['cap']) if j.get('cap') is not None else out.numel()
            if cap < 0 or cap > out.numel():
                raise LtError('encode_strips: cap must be within out')
            a = arr[k]
            a.in_, a.bands, a.bps = d.data_ptr(), nb, d.element_size()
            a.rows, a.cols, a.rows_per_strip = rows, cols, rps
            a.compression, a.predictor = comp, pred
            a.out, a.cap = out.data_ptr(), cap
            a.strip_sizes, a.total = meta.data_ptr(), meta.data_ptr() + 8 * ns
            res.append((out, meta[:ns], meta[ns:]))
        with self._encode_lock:  # one context: one caller at a time
            self._check(self.lib.lt_tiff_encode_strips_dev(self.ctx, arr, n,
                                                           ctypes.c_void_p(st.cuda_stream)),
                        'lt_tiff_encode_strips_dev')
        return res

    # --- ingest: rasters sampled at the grid points on the device (lt_grid_sample_dev) ---
    def sample_grid(self, jobs, stream=None):
        """Rasters in device memory sampled at ranges of a raster-order grid by the HIP sampling
        kernel (lt_sample.hip), the jobs of one call in order: what ingest_stack's np.take at
        grid_offsets' indices, the zeroing off the raster and the mask rule give. A job is a dict:
          src       contiguous device tensor [bands, rows, cols] (1, 2, 4 or 8 byte samples);
          xoff, yoff  the per-axis offsets (ingest.axis_offsets): host int32 arrays, checked
                    against src's shape and uploaded here, or int32 device tensors [grid cols],
                    [grid rows] (the caller's to have checked; the kernel reads nothing outside
                    src either way);
          p0, n     the grid pixels p0 .. p0 + n - 1 (pixel p: row p // cols, column p % cols);
          mode      _abi.LT_SAMPLE_BANDS (default) or _abi.LT_SAMPLE_MASK;
          sel       the source band of each output plane (default [0]; MASK reads sel[0]);
          out       BANDS: device tensor [len(sel), >= n] of src's type, unit pixel stride: plane
                    b gets band sel[b], zero off the raster;
          valid     uint8 device tensor [>= n], unit stride: BANDS writes whether the pixel is on
                    the raster, MASK clears it where the sample of band sel[0] is zero.
        Raises LtError, with nothing launched, for what lt_grid_sample_dev rejects. Asynchronous
        on `stream`; the caller keeps the tensors alive until it has run."""
        import numpy as np
        n_jobs = len(jobs)
        arr = (_abi.LtSampleJob * max(n_jobs, 1))()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        keep = []

        def bad(msg):
            raise LtError('sample_grid: ' + msg)

        for k, j in enumerate(jobs):
            src = j['src']
            if (not isinstance(src, torch.Tensor) or src.device != self.device or src.dim() != 3 or
                    not src.is_contiguous() or src.is_complex() or
                    src.element_size() not in (1, 2, 4, 8)):
                bad('src must be a contiguous [bands, rows, cols] tensor of 1, 2, 4 or 8 byte '
                    'samples on %s' % self.device)
            nb, sh, sw = src.shape
            mode = int(j.get('mode', _abi.LT_SAMPLE_BANDS))
            if mode not in (_abi.LT_SAMPLE_BANDS, _abi.LT_SAMPLE_MASK):
                bad('mode must be LT_SAMPLE_BANDS or LT_SAMPLE_MASK')
            if mode == _abi.LT_SAMPLE_MASK and src.is_floating_point():
                bad('floating-point masks are not taken (-0.0 == 0)')
            sel = [int(b) for b in j.get('sel', [0])]
            if not 1 <= len(sel) <= 16 or any(not 0 <= b < nb for b in sel):
                bad('sel must name 1..16 of the source\'s %d bands' % nb)
            p0, n = int(j['p0']), int(j['n'])
            offs = []
            for name, lim in (('xoff', sw), ('yoff', sh)):
                o = j[name]
                if isinstance(o, torch.Tensor):
                    if (o.dtype != torch.int32 or o.dim() != 1 or not o.is_contiguous() or
                            o.device != self.device):
                        bad('%s must be a contiguous int32 tensor on %s' % (name, self.device))
                else:
                    h = np.asarray(o)
                    if h.dtype != np.int32 or h.ndim != 1:
                        bad('%s must be a one-dimensional int32 array' % name)
                    if h.size and (int(h.min()) < -1 or int(h.max()) >= lim):
                        bad('%s outside the source raster' % name)
                    with torch.cuda.stream(st):
                        o = torch.from_numpy(np.ascontiguousarray(h)).to(self.device)
                    keep.append(o)
                offs.append(o)
            gw, gh = offs[0].numel(), offs[1].numel()
            if p0 < 0 or n < 0 or p0 + n > gw * gh:
                bad('p0 + n outside the grid of %d x %d' % (gh, gw))
            valid = j['valid']
            if (not isinstance(valid, torch.Tensor) or valid.dtype != torch.uint8 or
                    valid.dim() != 1 or valid.device != self.device or valid.numel() < n or
                    (valid.numel() > 1 and valid.stride(0) != 1)):
                bad('valid must be a uint8 [>= n] tensor with unit stride on %s' % self.device)
            a = arr[k]
            out = j.get('out')
            if mode == _abi.LT_SAMPLE_BANDS:
                if (not isinstance(out, torch.Tensor) or out.dtype != src.dtype or
                        out.device != self.device or out.dim() != 2 or
                        out.shape[0] != len(sel) or out.shape[1] < n or
                        (out.shape[1] > 1 and out.stride(1) != 1) or
                        (len(sel) > 1 and out.stride(0) < n)):
                    bad('out must be a %s [%d, >= n] tensor with unit pixel stride on %s'
                        % (src.dtype, len(sel), self.device))
                a.out = out.data_ptr()
                a.out_stride = out.stride(0) if len(sel) > 1 else max(n, out.stride(0))
            a.src, a.bps, a.src_bands, a.src_h, a.src_w = src.data_ptr(), src.element_size(), nb, sh, sw
            a.xoff, a.yoff, a.grid_w, a.grid_h = offs[0].data_ptr(), offs[1].data_ptr(), gw, gh
            a.p0, a.n, a.n_sel = p0, n, len(sel)
            for b, s in enumerate(sel):
                a.sel[b] = s
            a.valid, a.mode = valid.data_ptr(), mode
        with self._sample_lock:  # one context: one caller at a time (its error text)
            self._check(self.lib.lt_grid_sample_dev(self.ctx, arr, n_jobs,
                                                    ctypes.c_void_p(st.cuda_stream)),
                        'lt_grid_sample_dev')

    # --- JIT kernels of tiles carrying a program (lt_jit.h; lt_ctx_set_jit_mode, lt_jit_prepare) ---
    def set_jit_mode(self, asynchronous):
        """False (default): a launch needing a JIT module compiles it first. True: modules compile
        on worker threads and tiles launched before theirs is ready run on the precompiled kernels
        (same results; counted in jit_stats()['fallback_tiles'])."""
        self._check(self.lib.lt_ctx_set_jit_mode(
            self.ctx, _abi.LT_JIT_ASYNC if asynchronous else _abi.LT_JIT_SYNC), 'set_jit_mode')

    def jit_prepare(self, scene, params, bands, valid, fields, index, wait=True):
        """Compile (wait) or start compiling the JIT module lt_analyze_tiles would use for a tile
        of these band planes, mask and output fields, carrying `index` (an IndexFn). Raises
        LtError when a waited-for compile fails (the launches would then fall back)."""
        P = bands.shape[-1]
        tin, _, _ = self._tile_structs(scene, params, bands, valid, (), {}, None, index)
        tout = _abi.LtTileOut()
        tout.stride = P
        for f in fields:  # which planes are requested is all the module depends on (never read)
            setattr(tout, f, ctypes.cast(ctypes.c_void_p(16), type(getattr(tout, f))))
        sc = scene.to_c()
        with torch.cuda.device(self.device):
            self._check(self.lib.lt_jit_prepare(self.ctx, ctypes.byref(sc), ctypes.byref(params),
                                                ctypes.byref(tin), ctypes.byref(tout),
                                                1 if wait else 0), 'lt_jit_prepare')

    def jit_stats(self):
        """The context's JIT counters (lt_jit_stats) and its last JIT failure message."""
        st = _abi.LtJitStats()
        msg = ctypes.create_string_buffer(2048)
        self._check(self.lib.lt_ctx_jit_stats(self.ctx, ctypes.byref(st), msg, len(msg)),
                    'jit_stats')
        d = {f: getattr(st, f) for f, _ in _abi.LtJitStats._fields_}
        d['last_error'] = msg.value.decode(errors='replace')
        return d

    # --- stage timing (HIP events recorded around every launch on the launch stream) ---
    def set_timing(self, enable):
        self._check(self.lib.lt_ctx_set_timing(self.ctx, 1 if enable else 0), 'set_timing')

    def stage_ms(self):
        ms = (ctypes.c_double * 3)()
        n = ctypes.c_int64()
        self._check(self.lib.lt_ctx_stage_ms(self.ctx, ms, 3, ctypes.byref(n)), 'stage_ms')
        return {'analyze': ms[0], 'resolve': ms[1], 'expand': ms[2], 'launches': n.value}

    def last_deferred(self):
        n = ctypes.c_int64()
        self._check(self.lib.lt_ctx_last_deferred(self.ctx, ctypes.byref(n)), 'last_deferred')
        return n.value


def pack_valid_bits(valid):
    """A [K, P] cloud mask (nonzero = valid, utils.py:353) as the bit planes the analyze kernel
    reads (lt_tile_in.obs_valid_bits): int32 [ceil(K/32), P], bit k % 32 of plane k // 32."""
    K, P = valid.shape
    acc = torch.zeros(((K + 31) // 32, P), dtype=torch.int64, device=valid.device)
    for k in range(K):
        acc[k // 32] |= (valid[k] != 0).to(torch.int64) << (k % 32)
    return acc.to(torch.int32)


def valid_bytes(valid, n_obs):
    """The [K, P] uint8 mask of either form (bytes, or pack_valid_bits planes)."""
    if valid is None or valid.dtype == torch.uint8:
        return valid
    return torch.stack([((valid[k // 32] >> (k % 32)) & 1).to(torch.uint8)
                        for k in range(n_obs)])


class IndexFn:
    """A compiled load-stage kernel (owned by the engine's context). lin: the program's integer
    linear form (_abi.LtIndexLin) when it has one: the analyze kernel then evaluates the index of
    each winner from the band planes itself (analyze_tile(..., lin=fn.lin)), and the load kernel
    is needed only to materialise an index raster."""

    def __init__(self, handle, program, lin=None, build=None):
        self._handle = handle
        self._build = build  # makes the handle on first use (Engine.compile_index)
        self.program = program
        self.lin = lin

    @property
    def handle(self):
        if self._handle is None and self._build is not None:
            self._handle, self._build = self._build(), None
        return self._handle


class MaskFn:
    """A compiled mask_eqn kernel (owned by the engine's context)."""

    def __init__(self, handle, program):
        self.handle = handle
        self.program = program


def linear_form(program):
    """lt_index_linearize of an index_eqn.IndexProgram: its _abi.LtIndexLin, or None when the
    program is not an integer linear form (divisions, float nodes, products of band terms, mixed
    node types, more than LT_LIN_MAX_BANDS bands). Host-only: needs the library, not a GPU."""
    lib = _abi.load_lib()
    lin = _abi.LtIndexLin()
    prog = program.to_c()
    if lib.lt_index_linearize(ctypes.byref(prog), ctypes.byref(lin)) != 0:
        return None
    return lin


def _LT_T_OF_NP(np_dtype):
    from .index_eqn import DTYPES
    return DTYPES[np_dtype]


_ENGINES = {}


def get_engine(device=None):
    if isinstance(device, torch.device):
        device = device.index
    idx = torch.cuda.current_device() if device is None else int(device)
    eng = _ENGINES.get(idx)
    if eng is None:
        eng = _ENGINES[idx] = Engine(idx)
    return eng


def label_tile(engine, years, params, val_fit, vertex, present=None, out=None, stream=None):
    """change_labeling alone on trendlines in device memory: val_fit float64 [Y, P],
    vertex / present uint8 [Y, P] (same strides). Returns the rule-plane dict + status."""
    import numpy as np
    # the C ABI reads val_fit, vertex and present with the one lin.stride: check every plane the
    # way _tile_structs checks a tile (a mismatch would be an out-of-bounds device read)
    if (not isinstance(val_fit, torch.Tensor) or val_fit.dim() != 2 or
            val_fit.dtype != torch.float64 or val_fit.device != engine.device or
            val_fit.stride(1) != 1):
        raise LtError('val_fit must be a float64 [Y, P] tensor on %s with unit pixel stride'
                      % engine.device)
    for name, t in (('vertex', vertex), ('present', present)):
        if t is None and name == 'present':
            continue
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or
                t.device != engine.device or t.shape != val_fit.shape or
                t.stride() != val_fit.stride()):
            raise LtError('%s must be uint8 with the shape and strides of val_fit' % name)
    Y, P = val_fit.shape
    yrs = np.ascontiguousarray(np.asarray(years, np.int32))
    if len(yrs) != Y:
        raise LtError('years must have one entry per slot')
    if out is None:
        out = engine.alloc_outputs(Y, params.n_rules, P, LABELS + ('status',))
    need = set(LABELS) | {'status'}
    if not need <= set(out):
        raise LtError('out lacks %s' % sorted(need - set(out)))
    rstride = None
    for f, t in out.items():
        kind = _SHAPE_KIND.get(f)
        if kind is None or t.device != engine.device or t.dtype != _DTYPE[f] or t.shape[-1] < P:
            raise LtError('output %s has wrong device/dtype/shape' % f)
        if kind == 'rule':
            if t.dim() != 2 or t.shape[0] < max(params.n_rules, 1) or t.stride(1) != 1:
                raise LtError('output %s too small' % f)
            if rstride is not None and t.stride(0) != rstride:
                raise LtError('all [R, P] outputs must share one row stride')
            rstride = t.stride(0)
        elif kind == 'pix' and t.stride(0) != 1:
            raise LtError('output %s must have unit pixel stride' % f)
    lin = _abi.LtLabelIn()
    lin.n_pix = P
    lin.stride = val_fit.stride(0)
    lin.n_years = Y
    lin.year = yrs.ctypes.data_as(_abi.c_i32p)
    lin.val_fit = ctypes.cast(val_fit.data_ptr(), _abi.c_f64p)
    lin.vertex = ctypes.cast(vertex.data_ptr(), _abi.c_u8p)
    lin.present = ctypes.cast(present.data_ptr(), _abi.c_u8p) if present is not None else None
    tout = _abi.LtTileOut()
    tout.stride = rstride
    for f, t in out.items():
        setattr(tout, f, ctypes.cast(t.data_ptr(), type(getattr(tout, f))))
    st = stream if stream is not None else torch.cuda.current_stream(engine.device)
    rc = engine.lib.lt_label_tile(engine.ctx, ctypes.byref(lin), ctypes.byref(params),
                                  ctypes.byref(tout), ctypes.c_void_p(st.cuda_stream))
    engine._check(rc, 'lt_label_tile')
    return out
