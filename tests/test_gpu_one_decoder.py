"""The one HIP TIFF decoder (lt_chunks.hip) behind its two entries, lt_tiff_decode_strips_dev and
lt_tiff_decode_chunks_dev: the kernel instance with or without Deflate chosen per launch, the
strips entry as a translation into chunk jobs, and one scratch set per stream shared by both.
Beside test_gpu_decode.py and test_gpu_chunks.py, which cover each entry's formats. Every result is
compared bit for bit with the host build of the same decoder (tiffcodec.decode_chunks)."""
import numpy as np
import pytest

from chunkfixture import chunk_tiff, host_chunks, rand
from land_trendr_amd.geotiff import GeoTiff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from land_trendr_amd.engine import get_engine
    return get_engine(0)


def _job(eng, g, keep):
    """An open GeoTiff as an Engine.decode_chunks job, its bytes and tag lists on the device
    (`keep` holds them until the caller has synchronised)."""
    import torch
    otag, ctag, cw, ch, tiled, _ = g.chunk_layout()
    data = torch.from_numpy(np.frombuffer(g._d, np.uint8).copy()).to(eng.device)
    offs = torch.tensor(list(g.tags[otag]), dtype=torch.int64, device=eng.device)
    cnts = torch.tensor(list(g.tags[ctag]), dtype=torch.int64, device=eng.device)
    keep.append((data, offs, cnts))
    return dict(file=data, offsets=offs, counts=cnts, compression=g.compression,
                predictor=g.predictor, dtype=g.dtype, width=g.width, height=g.height,
                bands=g.bands, planar=g.planar, chunk_w=cw, chunk_h=ch, tiled=tiled)


def _decode_all(eng, files):
    """One decode_chunks call over the files: every error word 0, every image the host decoder's
    bit for bit."""
    import torch
    keep = []
    gs = [GeoTiff(p) for p in files]
    outs, err = eng.decode_chunks([_job(eng, g, keep) for g in gs])
    torch.cuda.synchronize(eng.device)
    assert err.cpu().tolist() == [0] * len(gs)
    for g, o in zip(gs, outs):
        want, rc = host_chunks(g)
        assert rc == 0 and np.array_equal(o.cpu().numpy().view(np.uint8), want.view(np.uint8))


def test_mixed_compressions_in_one_launch(eng, tmp_path):
    """A chunky LZW strip image, a Deflate tile image and an uncompressed planar strip image in
    one launch: the Deflate instance with LZW tables and chunk buffers in the same wave."""
    rng = np.random.default_rng(11)
    files = [chunk_tiff(str(tmp_path / 'l.tif'), rand(rng, 'int16', (3, 11, 7)), '<', 1, 2, 5,
                        rps=4),
             chunk_tiff(str(tmp_path / 'd.tif'), rand(rng, 'int16', (2, 40, 24)), '<', 2, 2, 8,
                        tile=(16, 16)),
             chunk_tiff(str(tmp_path / 'u.tif'), rand(rng, 'int16', (1, 9, 5)), '<', 2, 1, 1,
                        rps=4)]
    _decode_all(eng, files)


@pytest.mark.parametrize('deflate_first', [False, True])
def test_each_launch_picks_its_own_instance(eng, tmp_path, deflate_first):
    """17 images, two launches: 16 LZW strip images in one (the Deflate-free instance) and a
    Deflate tile image in the other, in either order."""
    rng = np.random.default_rng(12)
    files = [chunk_tiff(str(tmp_path / ('l%d.tif' % k)), rand(rng, 'int16', (1, 16, 16)), '<', 2,
                        2, 5, rps=4) for k in range(16)]
    d = chunk_tiff(str(tmp_path / 'd.tif'), rand(rng, 'int16', (1, 16, 16)), '<', 2, 2, 8,
                   tile=(16, 16))
    _decode_all(eng, [d] + files if deflate_first else files + [d])


def test_strips_entry_still_refuses(eng, tmp_path):
    """Engine.decode_strips is the strips entry, now a translation into chunk jobs: Deflate, which
    a chunk job may hold, and a strip of no rows are refused before anything launches."""
    import torch
    from land_trendr_amd.engine import LtError
    g = GeoTiff(chunk_tiff(str(tmp_path / 's.tif'), rand(np.random.default_rng(13), 'int16',
                                                         (1, 16, 16)), '<', 2, 1, 8, rps=4))
    keep = []
    base = {k: v for k, v in _job(eng, g, keep).items()
            if k not in ('chunk_w', 'chunk_h', 'tiled')}
    for kw in (dict(compression=8), dict(compression=32946), dict(compression=5, rows_per_strip=0)):
        with pytest.raises(LtError):
            eng.decode_strips([dict(dict(base, rows_per_strip=4), **kw)])
    torch.cuda.synchronize(eng.device)


def test_shared_scratch_across_the_two_entries(eng, tmp_path):
    """read_device (the strips entry) and then read_device_chunks of a larger chunky file on one
    stream: both use the stream's one scratch set, whose chunk buffers grow between the calls
    (176 to 7200 bytes a lane). Then the pair on a second stream, a set of its own."""
    import torch
    rng = np.random.default_rng(14)
    small = chunk_tiff(str(tmp_path / 'a.tif'), rand(rng, 'int16', (3, 11, 7)), '<', 1, 2, 5, rps=4)
    large = chunk_tiff(str(tmp_path / 'b.tif'), rand(rng, 'int16', (3, 40, 300)), '<', 1, 2, 5,
                       rps=4)
    for _ in range(2):
        st = torch.cuda.Stream(device=eng.device)
        for p, read in ((small, GeoTiff.read_device), (large, GeoTiff.read_device_chunks)):
            g = GeoTiff(p)
            want, rc = host_chunks(g)
            got, err = read(g, eng, stream=st)
            assert rc == 0 and int(err.item()) == 0
            assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8))
