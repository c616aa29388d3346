"""The Deflate core the device runs (land_trendr_amd/csrc/lt_inflate_core.h), compiled for the host
(liblt_io.so lt_inflate_core), against Python's zlib: same bytes on intact streams, the same
error-or-success on truncated, corrupt and hand-made streams (inflatefixture.ref), the lazy rule at
short caps, and no write outside the output buffer or past the returned count."""
import numpy as np
import pytest

import inflatefixture as fx
from land_trendr_amd import tiffcodec

ERR_DATA = -2
CANARY = 64


def _run(stream, cap):
    """(return value, the cap output bytes) of lt_inflate_core on a buffer of 0xEE bytes between
    two 64-byte canaries; asserts the canaries and that nothing past the count was written."""
    buf = np.full(cap + 2 * CANARY, 0xA5, np.uint8)
    buf[CANARY:CANARY + cap] = 0xEE
    n = tiffcodec._lib().lt_inflate_core(bytes(stream), len(stream), buf.ctypes.data + CANARY, cap)
    assert (buf[:CANARY] == 0xA5).all() and (buf[CANARY + cap:] == 0xA5).all(), 'canary'
    out = buf[CANARY:CANARY + cap].copy()
    assert n <= cap
    if n >= 0:
        assert (out[n:] == 0xEE).all(), 'a write past the returned count'
    return n, out


def _same_as_ref(stream, cap):
    """lt_inflate_core's outcome equals inflatefixture.ref's; returns whether it was a success."""
    want = fx.ref(stream, cap)
    n, out = _run(stream, cap)
    if want is None:
        assert n == ERR_DATA, (n, 'zlib rejects')
        return False
    assert n == len(want), (n, len(want))
    assert out[:n].tobytes() == want
    return True


INTACT = [(n, s, raw) for n, s, raw in fx.streams()] + [('far',) + fx.far()]


@pytest.mark.parametrize('name,stream,raw', INTACT, ids=[s[0] for s in INTACT])
def test_intact(name, stream, raw):
    n, out = _run(stream, len(raw) + 32)
    assert n == len(raw)
    assert out[:n].tobytes() == raw
    n, out = _run(stream + b'garbage', len(raw) + 32)  # bytes behind the trailer are ignored
    assert n == len(raw) and out[:n].tobytes() == raw


def test_every_prefix():
    rng = np.random.default_rng(3)
    raw = np.concatenate([rng.integers(0, 256, 300, dtype=np.uint8), np.zeros(200, np.uint8),
                          rng.integers(0, 8, 700, dtype=np.uint8)]).tobytes()
    import zlib
    enc = zlib.compress(raw, 6)
    assert 600 <= len(enc) <= 1000
    oks = [_same_as_ref(enc[:m], len(raw)) for m in range(len(enc) + 1)]
    assert oks == [False] * len(enc) + [True]


def test_corrupt_streams():
    corpus = fx.corrupt_streams()
    assert len(corpus) == 2000
    types = set()
    for enc, _ in fx.corrupt_bases():
        types |= {b['type'] for b in fx.blocks(enc)}
    assert types == {0, 1, 2}  # the intact bases cover every block type
    kinds = set()
    for k, (stream, size) in enumerate(corpus):
        try:
            kinds.add(_same_as_ref(stream, max(size, 1)))
        except AssertionError as e:
            raise AssertionError('corrupt stream %d: %s' % (k, e))
    assert kinds == {False, True}  # the corpus reaches both outcomes


@pytest.mark.parametrize('name,stream', fx.bad_streams(), ids=[s[0] for s in fx.bad_streams()])
def test_hand_made_errors(name, stream):
    assert fx.ref(stream, 64) is None
    assert _same_as_ref(stream, 64) is False


def test_short_cap():
    for name, stream, raw in INTACT:
        if len(raw) < 2:
            continue
        for cap in (len(raw) - 1, len(raw) // 2, 1):
            n, out = _run(stream, cap)
            assert n == cap and out.tobytes() == raw[:cap], (name, cap)
            assert fx.ref(stream, cap) == raw[:cap]


def test_wrapper_equals_decode():
    for name, stream, raw in INTACT:
        a = tiffcodec.inflate_core(stream, len(raw))
        assert np.array_equal(a, tiffcodec.decode(8, stream, len(raw))), name
        b = tiffcodec.inflate_core(stream, len(raw) + 100)
        assert np.array_equal(b, tiffcodec.decode(8, stream, len(raw) + 100)), name
        assert not b[len(raw):].any()
    with pytest.raises(ValueError):
        tiffcodec.inflate_core(fx.too_far_back(), 16)
