"""The LZW decoder core the device runs (land_trendr_amd/csrc/lt_lzw_core.h), compiled for the host
(liblt_io.so lt_lzw_decode_core), against the tuned host decoder lt_lzw_decode: same counts, bytes
and errors on intact, truncated and corrupt streams, and no write outside the output buffer."""
import ctypes

import numpy as np
import pytest

import lzwfixture
from land_trendr_amd import tiffcodec

ERR_DATA, ERR_SPACE = -2, -3
CANARY = 64


def _run(fn, stream, cap):
    """(return value, the cap output bytes, canaries intact) of one decoder on a buffer that sits
    between two 64-byte canaries."""
    buf = np.full(cap + 2 * CANARY, 0xA5, np.uint8)
    buf[CANARY:CANARY + cap] = 0
    n = fn(bytes(stream), len(stream), buf.ctypes.data + CANARY, cap)
    ok = bool((buf[:CANARY] == 0xA5).all() and (buf[CANARY + cap:] == 0xA5).all())
    return n, buf[CANARY:CANARY + cap].copy(), ok


def _both(stream, cap):
    L = tiffcodec._lib()
    n0, b0, ok0 = _run(L.lt_lzw_decode, stream, cap)
    n1, b1, ok1 = _run(L.lt_lzw_decode_core, stream, cap)
    assert ok0 and ok1, 'a decoder wrote outside its buffer'
    return n0, b0, n1, b1


@pytest.mark.parametrize('name,raw', lzwfixture.sources(), ids=[s[0] for s in lzwfixture.sources()])
def test_round_trip(name, raw):
    enc = tiffcodec.lzw_encode(raw)
    n0, b0, n1, b1 = _both(enc, len(raw) + 32)
    assert n0 == n1 == len(raw)
    assert b1[:n1].tobytes() == raw and b0[:n0].tobytes() == raw
    assert (b1[n1:] == 0).all()  # the core writes nothing past its count
    assert tiffcodec.lzw_decode_core(enc, len(raw)).tobytes() == raw
    if name == 'rand8400':
        codes = lzwfixture.read_codes(enc)
        assert codes[0][0] == lzwfixture.CLEAR
        assert any(c == lzwfixture.CLEAR for c, _ in codes[1:]), 'no table-full Clear'
        assert max(w for _, w in codes) == 12
        assert codes[-1][0] == lzwfixture.EOI


def test_truncation():
    rng = np.random.default_rng(3)
    raw = np.concatenate([rng.integers(0, 256, 300, dtype=np.uint8), np.zeros(200, np.uint8),
                          rng.integers(0, 8, 400, dtype=np.uint8)]).tobytes()
    enc = tiffcodec.lzw_encode(raw)
    assert 500 <= len(enc) <= 800
    for m in range(len(enc) + 1):
        n0, b0, n1, b1 = _both(enc[:m], len(raw))
        assert n0 == n1, m
        assert n1 >= 0 and np.array_equal(b0[:n0], b1[:n1]), m


def test_corrupt_streams():
    corpus = lzwfixture.corrupt_streams()
    assert len(corpus) == 2000
    corpus.append((lzwfixture.bad_code_strip(), 16))
    kinds = set()
    for k, (stream, size) in enumerate(corpus):
        n0, b0, n1, b1 = _both(stream, size)
        assert n0 == n1, k
        if n1 >= 0:
            assert np.array_equal(b0[:n0], b1[:n1]), k
        kinds.add(min(n1, 0))
    assert kinds == {0, ERR_DATA, ERR_SPACE}  # the corpus reaches every outcome
    n0, _, n1, _ = _both(lzwfixture.bad_code_strip(), 16)
    assert n0 == n1 == ERR_DATA


def test_short_cap():
    for name, raw in lzwfixture.sources():
        if len(raw) < 2:
            continue
        enc = tiffcodec.lzw_encode(raw)
        for cap in (len(raw) - 1, len(raw) // 2, 1, 0):
            n0, _, n1, _ = _both(enc, cap)
            assert n0 == n1 == ERR_SPACE, (name, cap)


def test_core_rejects_a_mebibyte():
    """The packed table holds 20-bit positions: a strip of 1 MiB or more is the host path's."""
    L = tiffcodec._lib()
    enc = tiffcodec.lzw_encode(b'abc')
    out = (ctypes.c_uint8 * 8)()
    assert L.lt_lzw_decode_core(enc, len(enc), ctypes.addressof(out), 1 << 20) == -1
