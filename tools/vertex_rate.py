"""The vertex-table kernel's rate alone (lt_vertex_table, land_trendr_amd/csrc/lt_vertex.hip), beside
lt_label_tile with one GD rule on the same planes: the kernel of the library that reads the same
val_fit / vertex rows in full.

Input: a --rows x --cols tile (default 4096 x 4096) of the seeded synthetic scene, --years years,
one int16 observation a year (no cloud mask). Its winner / val_fit / val_raw / vertex planes come
from one analyze launch per --line-costs entry (default 10 and 1: few and many vertices). Timed:
lt_vertex_table with V = the year count writing all four outputs, and lt_label_tile, alternating
in this process, warmed up, HIP events around --launches launches, --reps times (the spread).
Reported per line cost: ms per launch, the algorithmic bytes (computed here from the shapes and the
counted vertices: the flag and winner rows read, 16 B read per stored vertex, (20 V + 4) B written
per pixel), those bytes over the time and their share of 8 TB/s; the same for the label kernel
(its rows read in full, its rule planes written). The timed launch is also checked: a second
launch must give the same bits in every plane, and a seeded --check sample of pixels must equal
the kernel's per-pixel code run on the host (exit 3 otherwise). Prints one JSON line.

  python tools/vertex_rate.py [--rows 4096 --cols 4096 --years 30 --launches 20 --reps 3]
                              [--check 20000] [--line-costs 10,1]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TB_S = 8.0  # the MI355X's HBM3E peak


def timed(fn, launches, torch):
    """ms per launch of fn(), HIP events around `launches` launches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches


def rate(ms, nbytes):
    tb = nbytes / (min(ms) * 1e-3) / 1e12
    return {'ms': [round(v, 4) for v in ms], 'ms_best': round(min(ms), 4), 'bytes': int(nbytes),
            'tb_per_s': round(tb, 3), 'share_of_8_tb_per_s': round(tb / PEAK_TB_S, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=4096)
    ap.add_argument('--cols', type=int, default=4096)
    ap.add_argument('--years', type=int, default=30)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--seed', type=int, default=1000)
    ap.add_argument('--check', type=int, default=20000, help='host-checked pixel sample (0: none)')
    ap.add_argument('--line-costs', default='10,1')
    a = ap.parse_args()
    P = a.rows * a.cols
    import torch
    from land_trendr_amd.engine import LABELS, get_engine, label_tile
    from land_trendr_amd.scene import build_scene, parse_date
    from land_trendr_amd.settings import compile_params
    from land_trendr_amd.synth import make_scene
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import vertexfixture as vx
    eng = get_engine(0)
    sc = make_scene(P, n_years=a.years, k_min=1, k_max=1, mask_prob=0.0, seed=a.seed,
                    device='cuda')
    meta = build_scene(sc.dates, parse_date('2014-07-01'))
    index = sc.values.to(torch.int16)  # the synthetic index values are int16 integers
    assert bool((index.to(torch.float64) == sc.values).all())
    del sc
    Y = V = meta.n_years
    fields = ('winner', 'val_raw', 'val_fit', 'vertex', 'status')
    aout = eng.alloc_outputs(Y, 1, P, fields)
    vout = {'n_vertices': torch.empty(P, dtype=torch.int32, device='cuda'),
            'vertex_year': torch.empty((V, P), dtype=torch.int32, device='cuda'),
            'vertex_fit': torch.empty((V, P), dtype=torch.float64, device='cuda'),
            'vertex_raw': torch.empty((V, P), dtype=torch.float64, device='cuda')}
    res = {'tool': 'vertex_rate', 'pixels': P, 'years': Y, 'max_vertices': V,
           'launches': a.launches, 'runs': []}
    bad = False
    for lc in [float(x) for x in a.line_costs.split(',')]:
        params, _ = compile_params(lc, [{'name': 'gd', 'val': 1, 'change_type': 'GD'}])
        eng.analyze_tile(meta, params, index, None, fields, out=aout)
        torch.cuda.synchronize()
        present = (aout['winner'] >= 0).to(torch.uint8)
        lout = eng.alloc_outputs(Y, 1, P, LABELS + ('status',))
        run_v = lambda: eng.vertex_table(meta.years, aout['val_fit'], aout['vertex'],
                                         winner=aout['winner'], val_raw=aout['val_raw'],
                                         max_vertices=V, out=vout)
        run_l = lambda: label_tile(eng, meta.years, params, aout['val_fit'], aout['vertex'],
                                   present, out=lout)
        for _ in range(3):
            run_v()
            run_l()
        torch.cuda.synchronize()
        v_ms, l_ms = [], []
        for _ in range(a.reps):  # alternating, so that both see the same state of the device
            v_ms.append(timed(run_v, a.launches, torch))
            l_ms.append(timed(run_l, a.launches, torch))
        n = vout['n_vertices']
        stored = int(torch.clamp(n, max=V).sum())
        # flag rows (1 B) and winner rows (2 B) in full, both values of every stored vertex, and
        # every element of the four outputs once
        v_bytes = Y * P * 3 + 16 * stored + (20 * V + 4) * P
        # val_fit (8 B), vertex and present rows in full; matched + class_val + onset_year +
        # duration + magnitude + initial_val of one rule and the status
        l_bytes = Y * P * 10 + (1 + 4 + 4 + 4 + 8 + 8 + 4) * P
        run = {'line_cost': lc, 'vertices_per_pixel': round(float(n.sum()) / P, 3),
               'vertex_table': rate(v_ms, v_bytes), 'label_tile': rate(l_ms, l_bytes)}
        run['vertex_table']['mpx_per_s'] = round(P / min(v_ms) / 1e3, 1)
        # the launch at full occupancy, checked: a second launch gives the same bits in every
        # plane, and a seeded sample of pixels equals the kernel's per-pixel code run on the host
        # (tests/native/vertex_host_check.hip, the checker here, never a producer)
        differing = {}
        for f in vout:
            first = vout[f].clone()
            run_v()
            torch.cuda.synchronize()
            a_, b_ = (t.view(torch.int64) if t.dtype == torch.float64 else t
                      for t in (first, vout[f]))
            differing[f] = int((a_ != b_).sum())
            del first
        run['second_launch_differing'] = differing
        if a.check > 0:
            gen = torch.Generator().manual_seed(a.seed + 2)
            idx = torch.randperm(P, generator=gen)[:a.check].sort().values.cuda()
            host = vx.run_host(vx.load_host(), meta.years, *(
                aout[f][:, idx].cpu().numpy() for f in ('val_fit', 'vertex')),
                winner=aout['winner'][:, idx].cpu().numpy(),
                val_raw=aout['val_raw'][:, idx].cpu().numpy(), V=V)
            run['check'] = {'pixels': int(idx.numel()), 'checker': "the kernel's per-pixel code "
                            'on the host (liblt_vertexcheck.so)',
                            'mismatches': {f: int((~vx.same(vout[f][..., idx].cpu().numpy(),
                                                            host[f])).sum()) for f in vout}}
            bad = bad or any(run['check']['mismatches'].values())
        bad = bad or any(differing.values())
        res['runs'].append(run)
        del lout, present
    print(json.dumps(res), flush=True)
    if bad:
        sys.exit(3)


if __name__ == '__main__':
    main()
