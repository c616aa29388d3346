"""Encoder throughput: every encode_strips call of a device-encode job's output() timed with a
synchronise on both sides (raw bytes, encoded bytes = the D2H copy), and one call on a near-random
int16 raster of the same size. One JSON line to stdout."""
import json
import os
import shutil
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import job_bench  # noqa: E402
from land_trendr_amd.job import LocalJob  # noqa: E402

rows = cols = int(sys.argv[1]) if len(sys.argv) > 1 else 7000
work = '/tmp/ltjob_encthr'
shutil.rmtree(work, ignore_errors=True)
os.makedirs(work)
res = {'rows': rows, 'cols': cols}
try:
    job_bench.make_stack(work, 'bench', rows, cols, 30, 1000, 0.0)
    j = LocalJob(work, 'bench', device=0, tile_pixels=1 << 24, trendline=True, on_error='skip',
                 encode='device')
    j.setup(); j.parse(); j.analyze()
    torch.cuda.synchronize()
    eng = j.engine
    real = eng.encode_strips
    calls = []

    def timed(jobs, stream=None):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = real(jobs, stream)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        raw = sum(x['data'].numel() * x['data'].element_size() for x in jobs)
        enc = sum(int(t.item()) for _, _, t in r)
        calls.append({'rasters': len(jobs), 'raw': raw, 'encoded': enc, 's': dt})
        return r
    eng.encode_strips = timed
    t0 = time.perf_counter()
    j.output()
    res['output_s_with_syncs'] = round(time.perf_counter() - t0, 3)
    eng.encode_strips = real
    res['encode_stats'] = j.encode_stats
    tl = [c for c in calls if c['rasters'] == 8]
    res['trendline_calls'] = len(tl)
    gbs = sorted(c['raw'] / c['s'] / 1e9 for c in tl[1:])  # (the first call grows the scratch)
    res['trendline_date_gb_per_s'] = {'min': round(gbs[0], 3), 'median': round(gbs[len(gbs) // 2], 3),
                                      'max': round(gbs[-1], 3), 'first_call': round(tl[0]['raw'] / tl[0]['s'] / 1e9, 3)}
    res['trendline_date_raw_bytes'] = tl[1]['raw']
    res['trendline_date_encoded_bytes'] = sorted(c['encoded'] for c in tl)[len(tl) // 2]
    res['all_calls_raw'] = sum(c['raw'] for c in calls)
    res['all_calls_encoded'] = sum(c['encoded'] for c in calls)
    res['all_calls_s'] = round(sum(c['s'] for c in calls), 3)
    res['label_call'] = [c for c in calls if c['rasters'] != 8]
    del j
    torch.cuda.empty_cache()
    a = torch.randint(-3000, 3000, (1, rows, cols), dtype=torch.int16, device=eng.device)
    job = [{'data': a, 'rows_per_strip': 1, 'compression': 5, 'predictor': 1}]
    rr = []
    for k in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        (o, s, t), = real(job)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rr.append(round(a.numel() * 2 / dt / 1e9, 3))
        enc = int(t.item())
    res['random_int16_gb_per_s'] = rr
    res['random_int16_raw_bytes'] = a.numel() * 2
    res['random_int16_encoded_bytes'] = enc
    # the host encoder on the same raster, for the ratio on this box
    from land_trendr_amd import tiffcodec
    from land_trendr_amd.ingest import host_threads
    h = a.cpu().numpy()
    t0 = time.perf_counter()
    w, ws = tiffcodec.encode_strips(h, 1, 5, 1, host_threads())
    res['random_int16_host_gb_per_s'] = round(h.nbytes / (time.perf_counter() - t0) / 1e9, 3)
    res['random_int16_same_bytes'] = bool(len(w) == enc and
                                          o[:enc].cpu().numpy().tobytes() == w.tobytes())
    res['host_threads'] = host_threads()
finally:
    shutil.rmtree(work, ignore_errors=True)
print(json.dumps(res), flush=True)
