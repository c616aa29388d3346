"""One encode_strips call on 8 near-random int16 rasters of 7000 x 7000 (56000 strips: as many
lanes as one trendline date), and on one (7000 strips), GB/s of raw bytes."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from land_trendr_amd.engine import get_engine

eng = get_engine(0)
res = {}
for n in (1, 8):
    a = [torch.randint(-3000, 3000, (1, 7000, 7000), dtype=torch.int16, device=eng.device)
         for _ in range(n)]
    jobs = [{'data': t, 'rows_per_strip': 1, 'compression': 5, 'predictor': 1} for t in a]
    r = []
    for k in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.encode_strips(jobs)
        torch.cuda.synchronize()
        r.append(round(n * 98e6 / (time.perf_counter() - t0) / 1e9, 3))
        del out
    res['random_int16_x%d_gb_per_s' % n] = r
    del a, jobs
    torch.cuda.empty_cache()
print(json.dumps(res), flush=True)
