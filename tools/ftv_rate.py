"""The fit-to-vertex kernel's rate alone (lt_ftv_tile, land_trendr_amd/csrc/lt_ftv.hip), beside the
store-only ceiling of its plane layout and the analyze launch that made its flags.

Input: a --rows x --cols tile (default 4096 x 4096) of the seeded synthetic scene, --years years,
one int16 observation a year (no cloud mask). Its winner / spike / vertex planes come from one
analyze launch of the same data at line_cost 1 (c5-like vertex counts); the second index is a
seeded int16 raster. Timed: lt_ftv_tile writing all six planes, warmed up, HIP events around
--launches launches, --reps times (the spread); the analyze launch with every per-year plane the
same way. Reported: ms per launch, Mpx/s, written TB/s (48 B x present pixel-years over the time),
and build/bin/store_pattern's rates for the same pixels, years and six binary64 planes (a child
process, before this one allocates), with the ratio to its one-wave-per-64-pixels nontemporal
pattern. The timed launch is also checked: a second launch must give the same bits in every plane,
and a seeded --check sample of pixels must equal the kernel's per-pixel code run on the host
(exit 3 otherwise). Prints one JSON line.

  python tools/ftv_rate.py [--rows 4096 --cols 4096 --years 30 --launches 20 --reps 3]
                           [--check 20000] [--float64]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, launches, reps, torch):
    """ms per launch of fn(), HIP events around `launches` launches, `reps` times."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / launches)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=4096)
    ap.add_argument('--cols', type=int, default=4096)
    ap.add_argument('--years', type=int, default=30)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--seed', type=int, default=1000)
    ap.add_argument('--check', type=int, default=20000, help='host-checked pixel sample (0: none)')
    ap.add_argument('--float64', action='store_true',
                    help='the second index as binary64 values (obs_val) instead of int16')
    a = ap.parse_args()
    P = a.rows * a.cols
    store = None
    sp = os.path.join(ROOT, 'build', 'bin', 'store_pattern')
    if os.path.exists(sp):  # the store-only ceiling of this layout, same box, same visit
        r = subprocess.run([sp, str(P), str(a.years), '6', '0'], capture_output=True, text=True,
                           timeout=300)
        if r.returncode == 0:
            store = json.loads(r.stdout.strip().splitlines()[-1])
        else:
            print('store_pattern failed (%d): %s' % (r.returncode, r.stderr[-400:]),
                  file=sys.stderr)
    import torch
    from land_trendr_amd.engine import FTV_FIELDS, TRENDLINE, get_engine
    from land_trendr_amd.scene import build_scene, parse_date
    from land_trendr_amd.settings import compile_params
    from land_trendr_amd.synth import make_scene
    eng = get_engine(0)
    sc = make_scene(P, n_years=a.years, k_min=1, k_max=1, mask_prob=0.0, seed=a.seed,
                    device='cuda')
    meta = build_scene(sc.dates, parse_date('2014-07-01'))
    params, _ = compile_params(1.0, [{'name': 'gd', 'val': 1, 'change_type': 'GD'}])
    index = sc.values.to(torch.int16)  # the synthetic index values are int16 integers
    assert bool((index.to(torch.float64) == sc.values).all())
    del sc
    fields = TRENDLINE + ('status',)
    aout = eng.alloc_outputs(meta.n_years, 1, P, fields)
    run_a = lambda: eng.analyze_tile(meta, params, index, None, fields, out=aout)
    for _ in range(2):
        run_a()
    torch.cuda.synchronize()
    an_ms = timed(run_a, max(1, a.launches // 4), a.reps, torch)
    winner, spike, vertex = aout['winner'], aout['spike'], aout['vertex']
    present = int((winner >= 0).sum())
    n_vertex = int(vertex.sum())
    for f in FTV_FIELDS:
        del aout[f]
    g = torch.Generator(device='cuda').manual_seed(a.seed + 1)
    second = torch.randint(-2000, 2000, (meta.n_obs, P), generator=g, device='cuda',
                           dtype=torch.int16)
    if a.float64:
        second = second.to(torch.float64) * 0.37
    fout = eng.alloc_outputs(meta.n_years, 0, P, FTV_FIELDS + ('status',))
    run_f = lambda: eng.ftv_tile(meta, winner, spike, vertex, second, out=fout)
    for _ in range(3):
        run_f()
    torch.cuda.synchronize()
    ftv_ms = timed(run_f, a.launches, a.reps, torch)
    best = min(ftv_ms)
    written = 48.0 * present
    res = {'tool': 'ftv_rate', 'pixels': P, 'years': meta.n_years,
           'second_index': 'float64' if a.float64 else 'int16',
           'present_pixel_years': present, 'vertices_per_pixel': round(n_vertex / P, 3),
           'launches': a.launches, 'ftv_ms': [round(v, 4) for v in ftv_ms],
           'ftv_ms_best': round(best, 4), 'ftv_mpx_per_s': round(P / best / 1e3, 1),
           'ftv_written_tb_per_s': round(written / (best * 1e-3) / 1e12, 3),
           'analyze_ms': [round(v, 4) for v in an_ms],
           'analyze_mpx_per_s': round(P / min(an_ms) / 1e3, 1),
           'status_nonzero': int((fout['status'] != 0).sum())}
    # the launch at full occupancy, checked: a second launch gives the same bits in every plane, and
    # a seeded sample of pixels equals the kernel's per-pixel code run on the host
    # (tests/native/ftv_host_check.hip, the checker here, never a producer)
    differing = {}
    for f in FTV_FIELDS + ('status',):
        first = fout[f].clone()
        run_f()
        torch.cuda.synchronize()
        a_, b_ = (t.view(torch.int64) if t.dtype == torch.float64 else t for t in (first, fout[f]))
        differing[f] = int((a_ != b_).sum())
        del first
    res['second_launch_differing'] = differing
    if a.check > 0:
        import numpy as np
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import ftvfixture as fx
        gen = torch.Generator().manual_seed(a.seed + 2)
        idx = torch.randperm(P, generator=gen)[:a.check].sort().values.cuda()
        host = fx.run_host(fx.load_host(), meta, winner[:, idx].cpu().numpy(),
                           spike[:, idx].cpu().numpy(), vertex[:, idx].cpu().numpy(),
                           second[:, idx].cpu().numpy())
        res['check'] = {'pixels': int(idx.numel()), 'checker': "the kernel's per-pixel code on the "
                        'host (liblt_ftvcheck.so)',
                        'mismatches': {f: int((~fx.bits_equal(fout[f][..., idx].cpu().numpy(),
                                                              host[f])).sum())
                                       if f != 'status' else
                                       int((fout[f][idx].cpu().numpy() != host[f]).sum())
                                       for f in FTV_FIELDS + ('status',)}}
    if store is not None:
        res['store_pattern'] = store
        ceil = store['patterns'].get('wave64_nt')
        if ceil:
            res['store_ceiling_tb_per_s'] = ceil['TB_s']
            res['ratio_to_store_ceiling'] = round(res['ftv_written_tb_per_s'] / ceil['TB_s'], 3)
    print(json.dumps(res), flush=True)
    if any(differing.values()) or any(res.get('check', {}).get('mismatches', {}).values()):
        sys.exit(3)


if __name__ == '__main__':
    main()
