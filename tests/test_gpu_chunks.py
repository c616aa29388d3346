"""The HIP chunk decoder (lt_tiff_decode_chunks_dev, lt_chunks.hip) through
GeoTiff.read_device_chunks, Engine.decode_chunks and LocalJob(device_formats='all'), against the
per-chunk Python path (GeoTiff.read(native=False)), the host build of the same source
(tiffcodec.decode_chunks) and, on LZW strip files, the strip decoder. Only intact files go to the
device, plus the corrupt chunks of inflatefixture, which the host and sanitizer tests of the same
source have already taken (test_inflate_core_host.py, test_inflate_core_sanitized.py,
test_chunks_host.py)."""
import os

import numpy as np
import pytest

import inflatefixture
from chunkfixture import MATRIX, chunk_pixels, chunk_tiff, host_chunks, rand, retile
from land_trendr_amd.geotiff import GeoTiff, TiffError
from land_trendr_amd.raster import write_geotiff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from land_trendr_amd.engine import get_engine
    return get_engine(0)


def _same(eng, path):
    g = GeoTiff(path)
    assert g.device_chunks_eligible()
    want = g.read(native=False)
    got, err = g.read_device_chunks(eng)
    assert tuple(got.shape) == want.shape and int(err.item()) == 0
    assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8))
    return g, got


@pytest.mark.parametrize('dtype,bo,planar,predictor,compression', MATRIX)
def test_layout_matrix(eng, tmp_path, dtype, bo, planar, predictor, compression):
    """(3, 37, 41): 16 x 16 tiles (3 x 3 per band, clipped on both axes) and strips of 4 rows (a
    short last strip)."""
    a = rand(np.random.default_rng(1), dtype, (3, 37, 41))
    p = chunk_tiff(str(tmp_path / 't.tif'), a, bo, planar, predictor, compression, tile=(16, 16))
    g, _ = _same(eng, p)
    assert g.chunk_layout()[5] == (27 if planar == 2 else 9)
    p = chunk_tiff(str(tmp_path / 's.tif'), a, bo, planar, predictor, compression, rps=4)
    g, got = _same(eng, p)
    if compression != 8:  # the strip decoder's file: bit for bit the same planes
        old, err = g.read_device(eng)
        assert int(err.item()) == 0
        assert np.array_equal(old.cpu().numpy().view(np.uint8), got.cpu().numpy().view(np.uint8))


# test_gpu_decode.py's matrix of LZW / uncompressed strip files
STRIP_MATRIX = [('int16', '<', 2, 1, 5), ('int16', '>', 2, 2, 5), ('uint16', '<', 1, 2, 5),
                ('int32', '>', 1, 1, 1), ('uint8', '<', 2, 2, 5), ('int16', '<', 1, 1, 1),
                ('int64', '>', 1, 2, 5), ('int64', '<', 2, 2, 5), ('float64', '>', 2, 1, 5)]


@pytest.mark.parametrize('dtype,bo,planar,predictor,compression', STRIP_MATRIX)
def test_strip_files_equal_the_strip_decoder(eng, tmp_path, dtype, bo, planar, predictor,
                                             compression):
    """The strip decoder's own shapes, (3, 11, 7) with 4 rows per strip and the one-band
    (1, 300, 50) of 7 rows, through both decoders: the same planes bit for bit."""
    rng = np.random.default_rng(7)
    for shape, rps in (((3, 11, 7), 4), ((1, 300, 50), 7)):
        a = rng.standard_normal(shape).astype(dtype) if dtype == 'float64' else rand(rng, dtype,
                                                                                      shape)
        p = chunk_tiff(str(tmp_path / 's.tif'), a, bo, planar, predictor, compression, rps=rps)
        g, got = _same(eng, p)
        assert g.device_eligible()
        old, err = g.read_device(eng)
        assert int(err.item()) == 0
        assert np.array_equal(old.cpu().numpy().view(np.uint8), got.cpu().numpy().view(np.uint8))


def test_more_than_one_wave(eng, tmp_path):
    """(2, 130, 70) int16 in 16 x 16 Deflate tiles: 90 chunks, a partial second wave."""
    a = rand(np.random.default_rng(2), 'int16', (2, 130, 70))
    p = chunk_tiff(str(tmp_path / 'w.tif'), a, '<', 2, 2, 8, tile=(16, 16))
    g, _ = _same(eng, p)
    assert g.chunk_layout()[5] == 90


def test_block_types_side_by_side(eng, tmp_path):
    """One uint8 strip file, one row per strip, whose strips are fixture streams: the lanes of one
    wave take stored, fixed and dynamic blocks, overlapping copies, an empty stored block, the
    farthest distance and 15-bit codes at the same time. Short strips are zero-padded."""
    names = ['low-stored', 'low-fixed', 'low-l6', 'zeros-l6', 'period3-l6', 'low-flush',
             'fib-huffman', 'int16pred-l6', 'rand8400-stored', 'ramp-l9', 'empty-l6']
    rows = [inflatefixture.stream(n) for n in names] + [inflatefixture.far()]
    width = 121392
    assert max(len(raw) for _, raw in rows) == width
    a = np.zeros((1, len(rows), width), np.uint8)
    for k, (_, raw) in enumerate(rows):
        a[0, k, :len(raw)] = np.frombuffer(raw, np.uint8)
    p = chunk_tiff(str(tmp_path / 'b.tif'), a[:, :, :1], compression=8, rps=1, width=width,
                   replace={k: s for k, (s, _) in enumerate(rows)})
    g = GeoTiff(p)
    assert (g.width, g.height, g.chunk_layout()[5]) == (width, len(rows), len(rows))
    want, rc = host_chunks(g)
    assert rc == 0 and np.array_equal(want, a)
    got, err = g.read_device_chunks(eng)
    assert int(err.item()) == 0 and np.array_equal(got.cpu().numpy(), want)


def test_seventeen_images_in_one_call(eng, tmp_path):
    """A batch that crosses the 16-image launch boundary, one preallocated output."""
    import torch
    rng = np.random.default_rng(3)
    dev = eng.device
    jobs, wants, keep = [], [], []
    out = torch.zeros((17, 1, 16, 16), dtype=torch.int16, device=dev)
    for k in range(17):
        a = rand(rng, 'int16', (1, 16, 16))
        g = GeoTiff(chunk_tiff(str(tmp_path / ('i%d.tif' % k)), a, '<', 2, 2, 8, tile=(16, 16)))
        assert g.chunk_layout()[5] == 1
        data = torch.from_numpy(np.frombuffer(g._d, np.uint8).copy()).to(dev)
        offs = torch.tensor(list(g.tags[324]), dtype=torch.int64, device=dev)
        cnts = torch.tensor(list(g.tags[325]), dtype=torch.int64, device=dev)
        keep.append((data, offs, cnts))
        jobs.append(dict(file=data, offsets=offs, counts=cnts, compression=8, predictor=2,
                         dtype=g.dtype, width=16, height=16, bands=1, planar=2, chunk_w=16,
                         chunk_h=16, tiled=True, out=out[k]))
        wants.append(a)
    outs, err = eng.decode_chunks(jobs)
    torch.cuda.synchronize(dev)
    assert err.cpu().tolist() == [0] * 17
    assert np.array_equal(out.cpu().numpy(), np.stack(wants))
    assert all(o.data_ptr() == out[k].data_ptr() for k, o in enumerate(outs))


def test_rejected_before_launch(eng, tmp_path):
    import torch
    from land_trendr_amd.engine import LtError
    dev = eng.device
    z = torch.zeros(64, dtype=torch.uint8, device=dev)
    t = torch.zeros(4, dtype=torch.int64, device=dev)
    base = dict(file=z, offsets=t, counts=t, compression=8, predictor=1, dtype=np.dtype('u1'),
                width=8, height=8, bands=1, planar=2, chunk_w=4, chunk_h=4, tiled=True)
    for kw in (dict(compression=32773), dict(predictor=3), dict(planar=3), dict(chunk_w=0),
               dict(width=40, height=32, chunk_w=16, chunk_h=16),   # 6 tiles needed, 4 given
               dict(tiled=False),                                   # strips narrower than the image
               dict(width=2048, height=512, chunk_w=1024, chunk_h=1024)):  # a chunk of 1 MiB
        with pytest.raises(LtError):
            eng.decode_chunks([dict(base, **kw)])
    torch.cuda.synchronize(dev)


def test_failing_chunks(eng, tmp_path):
    """One tile replaced by too_far_back and one tile whose offset lies past the file: TiffError
    with check=True; with check=False the error word is -2 and every other tile is right."""
    a = rand(np.random.default_rng(4), 'int16', (3, 37, 41))

    def edit(offs, counts, size):
        offs[20] = size + 5
    p = chunk_tiff(str(tmp_path / 'b.tif'), a, '<', 2, 2, 8, tile=(16, 16),
                   replace={5: inflatefixture.too_far_back()}, edit=edit)
    g = GeoTiff(p)
    with pytest.raises(TiffError):
        g.read_device_chunks(eng)
    got, err = GeoTiff(p).read_device_chunks(eng, check=False)
    got = got.cpu().numpy()
    assert int(err.item()) == -2
    ok = np.ones(a.shape, bool)
    for k in (5, 20):
        b, ys, xs = chunk_pixels(g, k)
        ok[b, ys, xs] = False
    assert (~ok).any() and np.array_equal(got[ok], a[ok])
    host, rc = host_chunks(g, check=False)
    assert rc == -2 and np.array_equal(host[ok], a[ok])


def _job_dir(tmp_path, mode):
    from jobfixture import GT, make_job
    root = str(tmp_path / mode)
    make_job(root)
    tiled = retile(root)
    rdir = os.path.join(root, 'synth', 'input', 'rasters')
    masks = sorted(f for f in os.listdir(rdir) if f.endswith('_cloudmask.tif'))
    m = GeoTiff(os.path.join(rdir, masks[0])).read()
    write_geotiff(os.path.join(rdir, masks[0]), m, geotransform=GT, nodata=None,
                  compress='deflate')
    return root, len(tiled)


def test_job_all_formats_equals_host(tmp_path):
    from land_trendr_amd.job import LocalJob
    jobs, files = {}, {}
    modes = {'host': {}, 'all': dict(decode='device', sample='device', device_formats='all'),
             'strips': dict(decode='device', sample='device')}
    for mode, kw in modes.items():
        root, n_tiled = _job_dir(tmp_path, mode)
        j = jobs[mode] = LocalJob(root, 'synth', device=0, tile_pixels=50, on_error='skip', **kw)
        files[mode] = j.run()
    h, d, s = jobs['host'], jobs['all'], jobs['strips']
    K = len(d.rast_fns)
    assert n_tiled >= 3 and h.decode_stats['device'] == 0
    # every raster goes to the device with 'all'; the rewritten ones stay on the host without it,
    # and so does the Deflate mask (the behaviour before device_formats)
    assert d.device_formats == 'all' and s.device_formats == 'strips'
    assert d.decode_stats == {'device': K, 'host': 0}
    on_host = sum(1 for r, m in zip(s.rast_fns, s.mask_fns)
                  if not (GeoTiff(r).device_eligible() and (not m or GeoTiff(m).device_eligible())))
    assert n_tiled <= on_host < K and s.decode_stats == {'device': K - on_host, 'host': on_host}
    n_masks = sum(1 for m in d.mask_fns if m)
    assert d.sample_stats['masks_host'] == 0 and d.sample_stats['masks_device'] == n_masks
    assert s.sample_stats['masks_host'] >= 1
    for other in (d, s):
        assert sorted(h.planes) == sorted(other.planes)
        for k in h.planes:
            assert h.planes[k].dtype == other.planes[k].dtype, k
            assert np.asarray(h.planes[k]).tobytes() == np.asarray(other.planes[k]).tobytes(), k
        hb, ob = h.stack['bands'], other.stack['bands']
        assert hb.dtype == ob.dtype and hb.tobytes() == ob.tobytes()
        hv, ov = h.stack['valid'], other.stack['valid']
        assert hv.dtype == ov.dtype and hv.tobytes() == ov.tobytes()
    for mode in ('all', 'strips'):
        assert sorted(files['host']) == sorted(files[mode])
        for k, paths in files['host'].items():
            for ph, pd in zip(paths, files[mode][k]):
                assert os.path.basename(ph) == os.path.basename(pd)
                assert open(ph, 'rb').read() == open(pd, 'rb').read(), k
