"""The zonal-table kernels' rate alone (lt_zonal_stats, land_trendr_amd/csrc/lt_zonal.hip), beside
lt_label_counts on the same matched / onset-year planes: the kernel of the library that reads a
subset of the same bytes (5 of the 21 a pixel).

Input: a --rows x --cols field (default 7000 x 7000) made on the device from --seed: onset years
over --years years in 16 x 16-pixel patches, a --matched share of the pixels matched (default 0.5),
durations 1-12 and magnitudes N(400, 250). Zone layouts: 'one' (a single zone), 'blocks' (64 x 64-
pixel block zones) and 'random' (a random zone per pixel out of 65,536: the worst case of the wave
combine); 'one' is timed on both paths (the LDS table it gets by default, and the wave-combined
global adds forced), the others on the path they get. Timed: warmed up, HIP events around
--launches launches, --reps times, alternating with lt_label_counts (all values shown, the best
used). Reported per layout: ms per launch, its ratio to 4.2 times lt_label_counts' time (21 / 5
bytes: the bytes-proportional mark), the algorithmic bytes (21 a pixel) over the time and their
share of 8 TB/s. Every timed table is also checked: a second launch must give the same words, and
all four words of every cell must equal sums made with torch on the device (exit 3 otherwise).
Prints one JSON line.

  python tools/zonal_rate.py [--rows 7000 --cols 7000 --years 30 --launches 20 --reps 3]
                             [--matched 0.5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=7000)
    ap.add_argument('--cols', type=int, default=7000)
    ap.add_argument('--years', type=int, default=30)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--seed', type=int, default=1000)
    ap.add_argument('--matched', type=float, default=0.5)
    a = ap.parse_args()
    H, W, B = a.rows, a.cols, a.years
    P = H * W
    import torch
    from land_trendr_amd.engine import get_engine
    eng = get_engine(0)
    dev = eng.device
    gen = torch.Generator(device=dev).manual_seed(a.seed)
    r = torch.arange(H, device=dev)[:, None].expand(H, W).reshape(-1)
    c = torch.arange(W, device=dev)[None, :].expand(H, W).reshape(-1)
    lo = 1985
    patch = torch.randint(0, B, ((H + 15) // 16, (W + 15) // 16), generator=gen, device=dev)
    key = (lo + patch[r // 16, c // 16]).to(torch.int32)
    matched = (torch.rand(P, generator=gen, device=dev) < a.matched).to(torch.uint8)
    duration = torch.randint(1, 13, (P,), generator=gen, device=dev, dtype=torch.int32)
    value = torch.randn(P, generator=gen, device=dev, dtype=torch.float64) * 250.0 + 400.0
    nbw = (W + 63) // 64
    zones = {'one': (torch.zeros(P, dtype=torch.int32, device=dev), 1),
             'blocks': (((r // 64) * nbw + c // 64).to(torch.int32), ((H + 63) // 64) * nbw),
             'random': (torch.randint(0, 65536, (P,), generator=gen, device=dev,
                                      dtype=torch.int32), 65536)}
    del r, c, patch
    variants = [('one', 0), ('one', 2), ('blocks', 0), ('random', 0)]
    tables = {v: torch.zeros((zones[v[0]][1] + 1, B + 1, 4), dtype=torch.int64, device=dev)
              for v in variants}
    counts = torch.zeros(B + 1, dtype=torch.int64, device=dev)

    def run(v):
        z, nz = zones[v[0]]
        return lambda: eng.zonal_stats(matched, z, key, lo, B, nz, duration, value,
                                       out=tables[v], _path=v[1])
    run_c = lambda: eng.label_counts(matched, key, lo, B, out=counts)  # noqa: E731
    runs = [run(v) for v in variants]
    for _ in range(3):
        run_c()
        for f in runs:
            f()
    torch.cuda.synchronize()
    c_ms, z_ms = [], [[] for _ in variants]
    for _ in range(a.reps):  # alternating, so that all see the same state of the device
        c_ms.append(timed(run_c, a.launches, torch))
        for ms, f in zip(z_ms, runs):
            ms.append(timed(f, a.launches, torch))
    mark = 4.2 * min(c_ms)
    res = {'tool': 'zonal_rate', 'pixels': P, 'years': B, 'launches': a.launches,
           'matched_share': round(float(matched.ne(0).sum()) / P, 4),
           'label_counts': {'ms': [round(v, 4) for v in c_ms], 'ms_best': round(min(c_ms), 4),
                            'bytes': 5 * P,
                            'tb_per_s': round(5 * P / (min(c_ms) * 1e-3) / 1e12, 3)},
           'mark_ms': round(mark, 4), 'runs': []}
    bad = False
    from land_trendr_amd import _abi
    on = matched.ne(0)
    q = torch.round(value.clamp(-2.0 ** 30, 2.0 ** 30) * 16.0)  # (half to even; no NaN here)
    for v, ms, f in zip(variants, z_ms, runs):
        z, nz = zones[v[0]]
        cells = (nz + 1) * (B + 1)
        path = v[1] or (1 if cells <= _abi.LT_ZONAL_LDS_CELLS else 2)
        tb = 21 * P / (min(ms) * 1e-3) / 1e12
        out = {'zones': v[0], 'n_zones': nz, 'path': 'lds' if path == 1 else 'wave',
               'ms': [round(x, 4) for x in ms], 'ms_best': round(min(ms), 4),
               'times_mark': round(min(ms) / mark, 3), 'bytes': 21 * P, 'tb_per_s': round(tb, 3),
               'share_of_8_tb_per_s': round(tb / PEAK_TB_S, 3),
               'mpx_per_s': round(P / min(ms) / 1e3, 1)}
        tables[v].zero_()
        f()
        first = tables[v].clone()
        tables[v].zero_()
        f()
        torch.cuda.synchronize()
        out['second_launch_differing'] = int((first != tables[v]).sum())
        cell = (z.long() * (B + 1) + (key.long() - lo))[on]
        want = torch.stack([
            torch.bincount(cell, minlength=cells),
            torch.bincount(cell, weights=duration[on].double(), minlength=cells).long(),
            torch.bincount(cell, weights=q[on], minlength=cells).long(),
            torch.bincount(cell, minlength=cells)], dim=1)
        out['differing_from_torch_sums'] = int((want != first.view(-1, 4)).sum())
        del first, want, cell
        bad = bad or out['second_launch_differing'] or out['differing_from_torch_sums']
        res['runs'].append(out)
    print(json.dumps(res), flush=True)
    if bad:
        sys.exit(3)


if __name__ == '__main__':
    main()
