"""The change-map kernel's rate alone (lt_change_maps, land_trendr_amd/csrc/lt_change.hip), beside
lt_vertex_table on the same planes: the kernel of the library that reads a subset of the same
rows.

Input: a --rows x --cols tile (default 4096 x 4096) of the seeded synthetic scene, --years years,
one int16 observation a year (no cloud mask). Its winner / val_fit / val_raw / vertex / spike planes
come from one analyze launch at --line-cost (default 10). Timed: lt_change_maps with 1 and with 8
maps, each with the fit-noise inputs (val_raw and spike: rmse, n_fit and dsnr written) and without
(six planes a map), and lt_vertex_table with V = the year count, alternating in this process,
warmed up, HIP events around --launches launches, --reps times (all values shown, the best used).
Reported per variant: ms per launch, the algorithmic bytes (computed here from the shapes and the
counted points: the flag, winner and spike rows read in full, 8 B of val_fit per vertex or 16 B
per fitted point, 33 or 41 B written per map and pixel plus 12 B per pixel), those bytes over the
time and their share of 8 TB/s. The timed launch is also checked: a second launch must give the
same bits in every plane, and a seeded --check sample of pixels must equal the kernel's per-pixel
code run on the host (exit 3 otherwise). Prints one JSON line.

  python tools/change_rate.py [--rows 4096 --cols 4096 --years 30 --launches 20 --reps 3]
                              [--check 20000] [--line-cost 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TB_S = 8.0  # the MI355X's HBM3E peak

MAPS = [{'delta': 'loss'}, {'delta': 'gain', 'sort': 'newest', 'mag': ['>', 130]},
        {'delta': 'loss', 'sort': 'steepest', 'dur': ['>', 1], 'preval': ['>=', 600]},
        {'delta': 'loss', 'mag': ['>', 480]}, {'delta': 'gain', 'sort': 'longest', 'dur': ['<', 4]},
        {'delta': 'loss', 'sort': 'oldest', 'year': [1990, 1999]},
        {'delta': 'gain', 'sort': 'least', 'mag': ['<=', 26.0]},
        {'delta': 'loss', 'sort': 'shortest', 'preval': ['<', 0]}]


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
    ap.add_argument('--line-cost', type=float, default=10.0)
    a = ap.parse_args()
    P = a.rows * a.cols
    import torch
    from land_trendr_amd import _abi
    from land_trendr_amd.engine import get_engine
    from land_trendr_amd.scene import build_scene, parse_date
    from land_trendr_amd.settings import compile_params
    from land_trendr_amd.synth import make_scene
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import changefixture as cx
    eng = get_engine(0)
    sc = make_scene(P, n_years=a.years, k_min=1, k_max=1, mask_prob=0.0, seed=a.seed,
                    device='cuda')
    meta = build_scene(sc.dates, parse_date('2014-07-01'))
    index = sc.values.to(torch.int16)  # the synthetic index values are int16 integers
    assert bool((index.to(torch.float64) == sc.values).all())
    del sc
    Y = V = meta.n_years
    fields = ('winner', 'val_raw', 'val_fit', 'vertex', 'spike', 'status')
    aout = eng.alloc_outputs(Y, 1, P, fields)
    params, _ = compile_params(a.line_cost, [{'name': 'gd', 'val': 1, 'change_type': 'GD'}])
    eng.analyze_tile(meta, params, index, None, fields, out=aout)
    torch.cuda.synchronize()
    del index
    vout = {'n_vertices': torch.empty(P, dtype=torch.int32, device='cuda'),
            'vertex_year': torch.empty((V, P), dtype=torch.int32, device='cuda'),
            'vertex_fit': torch.empty((V, P), dtype=torch.float64, device='cuda'),
            'vertex_raw': torch.empty((V, P), dtype=torch.float64, device='cuda')}
    dts = {f: getattr(torch, d) for f, d in _abi.CHANGE_MAP_FIELDS + _abi.CHANGE_PIX_FIELDS}
    pix = tuple(f for f, _ in _abi.CHANGE_PIX_FIELDS)
    cout = {f: torch.empty((P,) if f in pix else (8, P), dtype=dt, device='cuda')
            for f, dt in dts.items()}

    def change(M, fit):
        out = {f: (t if f in pix else t[:M]) for f, t in cout.items()
               if fit or f not in ('dsnr', 'rmse', 'n_fit')}
        kw = dict(val_raw=aout['val_raw'], spike=aout['spike']) if fit else {}
        return out, lambda: eng.change_maps(meta.years, MAPS[:M], aout['val_fit'], aout['vertex'],
                                            winner=aout['winner'], out=out, **kw)
    run_v = lambda: eng.vertex_table(meta.years, aout['val_fit'], aout['vertex'],
                                     winner=aout['winner'], val_raw=aout['val_raw'],
                                     max_vertices=V, out=vout)
    variants = [(M, fit) + change(M, fit) for M in (1, 8) for fit in (False, True)]
    for _ in range(3):
        run_v()
        for v in variants:
            v[3]()
    torch.cuda.synchronize()
    v_ms, c_ms = [], [[] for _ in variants]
    for _ in range(a.reps):  # alternating, so that all see the same state of the device
        v_ms.append(timed(run_v, a.launches, torch))
        for ms, v in zip(c_ms, variants):
            ms.append(timed(v[3], a.launches, torch))
    n = vout['n_vertices']
    stored = int(n.sum())
    fitted = int(((aout['winner'] >= 0) & (aout['spike'] == 0)).sum())
    res = {'tool': 'change_rate', 'pixels': P, 'years': Y, 'launches': a.launches,
           'line_cost': a.line_cost, 'vertices_per_pixel': round(stored / P, 3),
           'fitted_points_per_pixel': round(fitted / P, 3),
           # flag rows (1 B) and winner rows (2 B) in full, both values of every vertex, and every
           # element of the four outputs once
           'vertex_table': rate(v_ms, Y * P * 3 + 16 * stored + (20 * V + 4) * P), 'runs': []}
    bad = False
    for ms, (M, fit, out, run) in zip(c_ms, variants):
        # flag and winner rows in full; without the fit inputs val_fit at every vertex, with them
        # the spike rows in full and val_fit and val_raw at every fitted point (a vertex is one)
        nbytes = Y * P * 3 + (Y * P + 16 * fitted + 41 * M * P + 12 * P if fit
                              else 8 * stored + 33 * M * P)
        r = dict(rate(ms, nbytes), maps=M, fit_inputs=fit)
        r['mpx_per_s'] = round(P / min(ms) / 1e3, 1)
        r['times_vertex_table'] = round(min(ms) / min(v_ms), 3)
        differing = {}
        run()
        torch.cuda.synchronize()
        first = {f: t.clone() for f, t in out.items()}
        run()
        torch.cuda.synchronize()
        for f, t in out.items():
            a_, b_ = (x.view(torch.int64) if x.dtype == torch.float64 else x
                      for x in (first[f], t))
            differing[f] = int((a_ != b_).sum())
        del first
        r['second_launch_differing'] = differing
        if a.check > 0:
            gen = torch.Generator().manual_seed(a.seed + 2)
            idx = torch.randperm(P, generator=gen)[:a.check].sort().values.cuda()
            kw = {f: aout[f][:, idx].cpu().numpy() for f in ('val_fit', 'vertex', 'winner')}
            if fit:
                kw.update({f: aout[f][:, idx].cpu().numpy() for f in ('val_raw', 'spike')})
            host = cx.run_host(cx.load_host(), MAPS[:M], meta.years, **kw)
            r['check'] = {'pixels': int(idx.numel()), 'checker': "the kernel's per-pixel code on "
                          'the host (liblt_changecheck.so)',
                          'mismatches': {f: int((~cx.same(out[f][..., idx].cpu().numpy(),
                                                          host[f])).sum()) for f in out}}
            bad = bad or any(r['check']['mismatches'].values())
        bad = bad or any(differing.values())
        r['matched_share'] = [round(float(x), 4) for x in
                              (out['matched'].ne(0).sum(dim=1).cpu().numpy() / P)]
        res['runs'].append(r)
    print(json.dumps(res), flush=True)
    if bad:
        sys.exit(3)


if __name__ == '__main__':
    main()
