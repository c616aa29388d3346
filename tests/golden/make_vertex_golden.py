"""Generate tests/golden/vertex_table.npz: every accepted golden pixel's vertices and disturbances,
made by the REFERENCE itself.

Survey container only (loads the reference through ref_shim.py). For every pixel of every golden
scene whose analysis the reference accepts (err '' or 'label:AttributeError') it runs the
reference's own analyze on the pixel's valid observations and stores
  - the vertex points of the Trendline as parse_disturbances walks them (classes.py:156-176: the
    first point, then every later point with .vertex): the year of index_date, val_fit, val_raw;
  - the list Trendline.parse_disturbances() yields: onset_year, duration, initial_val, magnitude.
Data only: plain arrays (np.savez_compressed, no pickles), committed as a fixture; the GPU box only
reads it. The lists are ragged, so they are stored flat with offsets.

Per scene <s> the file holds
  <s>_pix                          [n]     pixel ids in scene_<s>.npz
  <s>_voff                         [n+1]   pixel i's vertices are [voff[i], voff[i+1]) of
  <s>_vyear, <s>_vfit, <s>_vraw    [nv]    int32, float64, float64
  <s>_doff                         [n+1]   pixel i's disturbances are [doff[i], doff[i+1]) of
  <s>_donset, <s>_dduration        [nd]    int32
  <s>_dinitial, <s>_dmagnitude     [nd]    float64

Per scene the script asserts that its segment count equals the count the scene's own winner /
vertex planes give.

Run: python tests/golden/make_vertex_golden.py
"""
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

OK_ERR = ('', 'label:AttributeError')
_REF = None


def _ref():
    global _REF
    if _REF is None:
        import ref_shim
        _REF = ref_shim.load_reference()
    return _REF


def _eval_pixel(args):
    """The reference's analyze on one pixel: (vertex rows, disturbance rows), plain floats / ints."""
    pix_datas, line_cost, target = args
    utils, _ = _ref()
    tl = utils.analyze(pix_datas, line_cost, utils.parse_date(target))
    verts = [(utils.parse_date(p.index_date).year, float(p.val_fit), float(p.val_raw))
             for i, p in enumerate(tl.points) if i == 0 or p.vertex]
    dists = [(int(d.onset_year), int(d.duration), float(d.initial_val), float(d.magnitude))
             for d in tl.parse_disturbances()]
    return verts, dists


def plane_segments(g, pix):
    """Segments per pixel from the scene's own planes: the flagged present slots after the first
    present one."""
    present = g.ref['winner'][:, pix] >= 0
    later = present & (np.cumsum(present, 0) > 1)
    return (later & (g.ref['vertex'][:, pix] != 0)).sum(0)


def main():
    import golden_io
    out = {}
    total_pix = total_seg = 0
    lo, hi = 1 << 30, 0
    with mp.Pool(max(1, min(16, os.cpu_count() or 1))) as pool:
        for name in golden_io.scene_names():
            g = golden_io.GoldenScene(name)
            dates, K = g.meta['dates'], g.values.shape[0]
            pix = [p for p in range(g.n_pix) if g.err[p] in OK_ERR]
            jobs = [([{'date': dates[k], 'val': float(g.values[k, p])} for k in range(K)
                      if g.valid[k, p]], g.meta['line_cost'], g.meta['target']) for p in pix]
            res = pool.map(_eval_pixel, jobs, chunksize=4)
            voff = np.cumsum([0] + [len(v) for v, _ in res]).astype(np.int64)
            doff = np.cumsum([0] + [len(d) for _, d in res]).astype(np.int64)
            verts = [r for v, _ in res for r in v]
            dists = [r for _, d in res for r in d]
            n_seg = np.diff(doff)
            assert (np.diff(voff) == n_seg + 1).all(), name
            assert (n_seg == plane_segments(g, np.asarray(pix, np.int64))).all(), name
            out[name + '_pix'] = np.asarray(pix, np.int32)
            out[name + '_voff'], out[name + '_doff'] = voff, doff
            out[name + '_vyear'] = np.array([r[0] for r in verts], np.int32)
            out[name + '_vfit'] = np.array([r[1] for r in verts], np.float64)
            out[name + '_vraw'] = np.array([r[2] for r in verts], np.float64)
            out[name + '_donset'] = np.array([r[0] for r in dists], np.int32)
            out[name + '_dduration'] = np.array([r[1] for r in dists], np.int32)
            out[name + '_dinitial'] = np.array([r[2] for r in dists], np.float64)
            out[name + '_dmagnitude'] = np.array([r[3] for r in dists], np.float64)
            total_pix += len(pix)
            total_seg += int(n_seg.sum())
            if len(pix):
                lo, hi = min(lo, int(n_seg.min())), max(hi, int(n_seg.max()))
            print('scene %-9s %4d pixels %6d segments (mean %.1f)'
                  % (name, len(pix), int(n_seg.sum()), n_seg.mean() if len(pix) else 0.0),
                  flush=True)
    path = os.path.join(HERE, 'vertex_table.npz')
    np.savez_compressed(path, **out)
    print('%d pixels, %d segments (%d..%d per pixel), %d bytes'
          % (total_pix, total_seg, lo, hi, os.path.getsize(path)))


if __name__ == '__main__':
    main()
