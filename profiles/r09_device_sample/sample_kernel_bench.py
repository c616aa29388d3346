"""The sampling kernel alone at the c2 size: two int16 bands of a four-band source of another extent
into a 7000 x 7000 grid, then an 8-bit mask; HIP events around 20 calls. LT_HIP_LIB selects the build."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from land_trendr_amd import _abi, ingest
from land_trendr_amd.engine import get_engine

eng = get_engine(0)
H = W = 7000
GT = (500000.0, 30.0, 0.0, 4200000.0, 0.0, -30.0)
xv = GT[0] + (np.arange(W) + 0.5) * GT[1]
yv = GT[3] + (np.arange(H) + 0.5) * GT[5]
res = {'lib': os.environ.get('LT_HIP_LIB', 'default')}
for name, (sh, sw, dy, dx) in (('shifted', (7005, 6996, -2, 3)), ('aligned', (7000, 7000, 0, 0))):
    gt = (GT[0] - dx * GT[1], GT[1], 0.0, GT[3] - dy * GT[5], 0.0, GT[5])
    xo, yo = ingest.axis_offsets(gt, (sh, sw), xv, yv)
    dxo, dyo = torch.from_numpy(xo).cuda(), torch.from_numpy(yo).cuda()
    src = torch.randint(-3000, 3000, (4, sh, sw), dtype=torch.int16, device='cuda')
    mask = (torch.rand((1, sh, sw), device='cuda') < 0.8).to(torch.uint8)
    out = torch.empty((2, H * W), dtype=torch.int16, device='cuda')
    valid = torch.empty(H * W, dtype=torch.uint8, device='cuda')
    jb = dict(src=src, xoff=dxo, yoff=dyo, p0=0, n=H * W, sel=[0, 1], out=out, valid=valid)
    jm = dict(src=mask, xoff=dxo, yoff=dyo, p0=0, n=H * W, valid=valid, mode=_abi.LT_SAMPLE_MASK)
    on = float(((xo >= 0).sum() * (yo >= 0).sum())) / (H * W)
    for label, job, nbytes in (('bands', jb, H * W * (2 * 2 * on + 2 * 2 + 1)),
                               ('mask', jm, H * W * (1 * on + 2))):
        for _ in range(3):
            eng.sample_grid([job])
        torch.cuda.synchronize()
        ms = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.sample_grid([job])
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        ms.sort()
        res['%s_%s' % (name, label)] = {'ms_median': round(ms[10], 4), 'ms_min': round(ms[0], 4),
                                        'bytes': int(nbytes),
                                        'gb_per_s_median': round(nbytes / ms[10] / 1e6, 1)}
print(json.dumps(res))
