"""The MMU sieve's rate alone (lt_sieve_labels, land_trendr_amd/csrc/lt_sieve.hip) on three fields
of a --rows x --cols raster (default 7000 x 7000):

  analysis   the GD rule's matched / onset_year planes of one analyze launch on the seeded
             synthetic scene (--years years, one int16 observation a year): many tiny patches
  random     every pixel matched with probability 0.59, one key: giant tortuous patches
  all        every pixel matched, one key: one patch

Per field, 8-connectivity, min_pixels --mmu (default 11), apply on a fresh copy of matched: ms per
launch of the four launches one by one (HIP events round each; lt_sieve_in.phases) and of the whole
call, best of --reps; Mpx/s; the algorithmic bytes (14 B a pixel: matched and key read, root and
size written, matched written) over the time and their share of 8 TB/s; the patch count, the
largest patch and the pixels cleared; for `analysis` the analyze launch's own time beside it. The
call is also checked: a second call must agree in every element, and (--check) the kernels' host
twin on one thread must give the same root, size and matched (its time is reported, and
scipy.ndimage.label's on the matched mask if scipy imports). Exit 3 on any difference. Prints one
JSON line.

  python tools/sieve_rate.py [--rows 7000 --cols 7000 --years 30 --reps 3 --mmu 11]
                             [--fields analysis,random,all] [--no-check]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TB_S = 8.0  # the MI355X's HBM3E peak
PHASES = ('local', 'merge', 'resolve', 'expand')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=7000)
    ap.add_argument('--cols', type=int, default=7000)
    ap.add_argument('--years', type=int, default=30)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--mmu', type=int, default=11)
    ap.add_argument('--seed', type=int, default=1000)
    ap.add_argument('--fields', default='analysis,random,all')
    ap.add_argument('--no-check', action='store_true')
    a = ap.parse_args()
    H, W = a.rows, a.cols
    P = H * W
    import numpy as np
    import torch
    from land_trendr_amd.engine import get_engine
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import sievefixture as sx
    eng = get_engine(0)
    dev = eng.device
    res = {'tool': 'sieve_rate', 'rows': H, 'cols': W, 'pixels': P, 'min_pixels': a.mmu,
           'connectivity': 8, 'fields': {}}
    bad = False

    def event():
        return torch.cuda.Event(enable_timing=True)

    def field(name):
        extra = {}
        if name == 'analysis':
            from land_trendr_amd.scene import build_scene, parse_date
            from land_trendr_amd.settings import compile_params
            from land_trendr_amd.synth import make_scene
            sc = make_scene(P, n_years=a.years, k_min=1, k_max=1, mask_prob=0.0, seed=a.seed,
                            device='cuda')
            meta = build_scene(sc.dates, parse_date('2014-07-01'))
            index = sc.values.to(torch.int16)
            del sc
            params, _ = compile_params(10.0, [{'name': 'gd', 'val': 1, 'change_type': 'GD'}])
            fields = ('matched', 'onset_year', 'status')
            out = eng.alloc_outputs(meta.n_years, 1, P, fields)
            eng.analyze_tile(meta, params, index, None, fields, out=out)  # warm
            e0, e1 = event(), event()
            e0.record()
            eng.analyze_tile(meta, params, index, None, fields, out=out)
            e1.record()
            e1.synchronize()
            extra['analyze_launch_ms'] = round(e0.elapsed_time(e1), 3)
            m, k = out['matched'][0].clone(), out['onset_year'][0].clone()
            del out, index
            return m, k, extra
        if name == 'random':
            gen = torch.Generator(device=dev).manual_seed(a.seed + 1)
            m = (torch.rand(P, device=dev, generator=gen) < 0.59).to(torch.uint8)
        else:
            m = torch.ones(P, dtype=torch.uint8, device=dev)
        return m, torch.full((P,), 2000, dtype=torch.int32, device=dev), extra

    for name in a.fields.split(','):
        m0, key, run = field(name)
        m = m0.clone()
        out = {f: torch.empty(P, dtype=torch.int32, device=dev) for f in ('root', 'size')}
        work = torch.empty(eng.lib.lt_sieve_workspace_bytes(H, W) // 4, dtype=torch.int32,
                           device=dev)

        def call(phases):
            eng.sieve(m, key, (H, W), a.mmu, 8, True, out=out, _phases=(work, phases))
        m.copy_(m0)
        call(0)  # warm
        per = {p: [] for p in PHASES}
        whole = []
        for _ in range(a.reps):
            m.copy_(m0)
            ev = [event() for _ in range(5)]
            ev[0].record()
            for i in range(4):
                call(1 << i)
                ev[i + 1].record()
            ev[4].synchronize()
            for i, p in enumerate(PHASES):
                per[p].append(ev[i].elapsed_time(ev[i + 1]))
            m.copy_(m0)
            e0, e1 = event(), event()
            e0.record()
            call(0)
            e1.record()
            e1.synchronize()
            whole.append(e0.elapsed_time(e1))
        best = min(whole)
        tb = 14 * P / (best * 1e-3) / 1e12
        size, root = out['size'], out['root']
        run.update({
            'matched': int((m0 != 0).sum()), 'cleared': int((m0 != 0).sum() - (m != 0).sum()),
            'patches': int((root == torch.arange(P, dtype=torch.int32, device=dev)).sum()),
            'largest_patch': int(size.max()),
            'phase_ms': {p: round(min(v), 4) for p, v in per.items()},
            'ms': [round(v, 4) for v in whole], 'ms_best': round(best, 4),
            'mpx_per_s': round(P / best / 1e3, 1), 'bytes': 14 * P, 'tb_per_s': round(tb, 3),
            'share_of_8_tb_per_s': round(tb / PEAK_TB_S, 4)})
        first = {f: t.clone() for f, t in dict(out, matched=m).items()}
        m.copy_(m0)
        call(0)
        torch.cuda.synchronize()
        run['second_launch_differing'] = {f: int((first[f] != t).sum())
                                          for f, t in dict(out, matched=m).items()}
        bad = bad or any(run['second_launch_differing'].values())
        if not a.no_check:
            hm, hk = m0.cpu().numpy(), key.cpu().numpy()
            t0 = time.perf_counter()
            r, s, mm = sx.run_host(sx.load_host(), hm, hk, (H, W), a.mmu, 8)
            run['host_twin_one_thread_s'] = round(time.perf_counter() - t0, 3)
            run['check'] = {'checker': "the kernels' phase steps on the host (liblt_sievecheck.so)",
                            'mismatches': {'root': int((first['root'].cpu().numpy() != r).sum()),
                                           'size': int((first['size'].cpu().numpy() != s).sum()),
                                           'matched': int((first['matched'].cpu().numpy()
                                                           != mm).sum())}}
            bad = bad or any(run['check']['mismatches'].values())
            try:
                from scipy import ndimage
                t0 = time.perf_counter()
                _, n = ndimage.label((hm != 0).reshape(H, W), structure=np.ones((3, 3), int))
                run['scipy_label_s'] = round(time.perf_counter() - t0, 3)
                run['scipy_label_patches_of_the_mask'] = int(n)
            except ImportError:
                pass
        res['fields'][name] = run
        del m0, m, key, out, work, first
    print(json.dumps(res), flush=True)
    if bad:
        sys.exit(3)


if __name__ == '__main__':
    main()
