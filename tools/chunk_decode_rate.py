"""The device decoders' rate alone, in GB/s of decoded bytes, for one raster of each kind: LZW
strips through the strips entry (GeoTiff.read_device; the row still named "strip decoder") and
through the chunks entry (read_device_chunks), which share one kernel; Deflate strips, Deflate tiles. The raster is two int16 bands of a synthetic
scene (tools/job_bench.py's rasters). kernel_ms: the decode call between two events on its
stream, the file's bytes already on the device; read_call_ms: the whole read_device /
read_device_chunks call with check=True (staging copy, H2D, kernel, synchronise). Best of --reps.

  python tools/chunk_decode_rate.py --rows 7000 --cols 7000 --tiles 256 512
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=7000)
    ap.add_argument('--cols', type=int, default=7000)
    ap.add_argument('--tiles', type=int, nargs='*', default=[256, 512])
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    import torch
    from land_trendr_amd.engine import get_engine
    from land_trendr_amd.geotiff import GeoTiff
    from land_trendr_amd.raster import write_geotiff
    from land_trendr_amd.synth import make_scene
    eng = get_engine(0)
    sc = make_scene(a.rows * a.cols, n_years=1, k_min=1, k_max=1, mask_prob=0.0, seed=1000,
                    device='cuda', with_bands=True)
    img = sc.bands[0].reshape(2, a.rows, a.cols).cpu().numpy()
    del sc
    kinds = [('lzw strips (strip decoder)', dict(compress='lzw'), 'strips'),
             ('lzw strips', dict(compress='lzw'), 'chunks'),
             ('deflate strips', dict(compress='deflate'), 'chunks')]
    kinds += [('deflate tiles %d' % t, dict(compress='deflate', tile=(t, t)), 'chunks')
              for t in a.tiles]
    kinds += [('lzw tiles %d' % t, dict(compress='lzw', tile=(t, t)), 'chunks')
              for t in a.tiles[:1]]
    res = []
    with tempfile.TemporaryDirectory() as d:
        for name, kw, path in kinds:
            p = os.path.join(d, 'r.tif')
            t0 = time.time()
            write_geotiff(p, img, nodata=None, **kw)
            wrote = time.time() - t0
            g = GeoTiff(p)
            want = g.read()
            out = torch.empty(want.shape, dtype=torch.int16, device=eng.device)
            best = None
            for _ in range(a.reps):
                read = g.read_device if path == 'strips' else g.read_device_chunks
                t0 = time.perf_counter()
                got, err = read(eng, out=out, check=True)
                whole = time.perf_counter() - t0
                best = whole if best is None else min(best, whole)
            same = bool(np.array_equal(got.cpu().numpy(), want))
            # the kernel alone: the file's bytes on the device first, then the engine call
            lay = g.chunk_layout()
            offs = torch.tensor(np.asarray(g.tags[lay[0]], np.int64), device=eng.device)
            cnts = torch.tensor(np.asarray(g.tags[lay[1]], np.int64), device=eng.device)
            data = torch.from_numpy(np.frombuffer(g._d, np.uint8).copy()).to(eng.device)
            job = dict(file=data, offsets=offs, counts=cnts, compression=g.compression,
                       predictor=g.predictor, dtype=g.dtype, width=g.width, height=g.height,
                       bands=g.bands, planar=g.planar, out=out)
            kern = None
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if path == 'strips':
                    eng.decode_strips([dict(job, rows_per_strip=lay[3])])
                else:
                    eng.decode_chunks([dict(job, chunk_w=lay[2], chunk_h=lay[3], tiled=lay[4])])
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1)
                kern = ms if kern is None else min(kern, ms)
            same = same and bool(np.array_equal(out.cpu().numpy(), want))
            row = {'kind': name, 'file_MB': round(os.path.getsize(p) / 1e6, 1),
                   'decoded_MB': round(want.nbytes / 1e6, 1), 'chunks': int(lay[5]),
                   'kernel_ms': round(kern, 2), 'kernel_GBps': round(want.nbytes / kern / 1e6, 2),
                   'read_call_ms': round(best * 1e3, 1), 'same_as_host': same,
                   'write_s': round(wrote, 1)}
            print(json.dumps(row), flush=True)
            res.append(row)
            del g
    print(json.dumps({'rows': a.rows, 'cols': a.cols, 'results': res}))


if __name__ == '__main__':
    main()
