"""The LZW encoder core the device runs (land_trendr_amd/csrc/lt_lzw_core.h), compiled for the host
(liblt_io.so lt_lzw_encode_core), against the host encoder lt_lzw_encode: the same bytes for every
input (greedy LZW under the TIFF stream rules is deterministic), nothing written outside the
output buffer, LT_IO_ERR_SPACE for every short cap, and the same core stand-alone under
AddressSanitizer / UBSan (tests/native/lzw_encode_core_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import lzwfixture
from land_trendr_amd import tiffcodec

ERR_SPACE = -3
CANARY = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = np.random.default_rng(7).integers(0, 256, 9000, dtype=np.uint8)
FULL_AT_END = 3941            # the table fills on the final code: a Clear before EOI
WIDER_EOI = (255, 771, 1812)  # the final code takes the width step: EOI one bit wider


def _run(fn, raw, cap):
    """(return value, the cap output bytes, canaries intact) of one encoder on a buffer that sits
    between two 64-byte canaries."""
    buf = np.full(cap + 2 * CANARY, 0xA5, np.uint8)
    buf[CANARY:CANARY + cap] = 0
    n = fn(bytes(raw), len(raw), buf.ctypes.data + CANARY, cap)
    ok = bool((buf[:CANARY] == 0xA5).all() and (buf[CANARY + cap:] == 0xA5).all())
    return n, buf[CANARY:CANARY + cap].copy(), ok


@pytest.mark.parametrize('name,raw', lzwfixture.sources(), ids=[s[0] for s in lzwfixture.sources()])
def test_sources(name, raw):
    assert tiffcodec.lzw_encode_core(raw) == tiffcodec.lzw_encode(raw)


def test_rule_boundary_scan():
    for n in range(1, 6001):
        raw = SCAN[:n].tobytes()
        assert tiffcodec.lzw_encode_core(raw) == tiffcodec.lzw_encode(raw), n
    # the scan holds the end-of-input cases of the stream rules (read off the host stream)
    codes = lzwfixture.read_codes(tiffcodec.lzw_encode(SCAN[:FULL_AT_END].tobytes()))
    assert codes[-1][0] == lzwfixture.EOI and codes[-2][0] == lzwfixture.CLEAR
    assert codes[-1][1] == 9 and codes[-2][1] == 12
    for n in WIDER_EOI:
        codes = lzwfixture.read_codes(tiffcodec.lzw_encode(SCAN[:n].tobytes()))
        assert codes[-1][0] == lzwfixture.EOI and codes[-2][0] != lzwfixture.CLEAR, n
        assert codes[-1][1] == codes[-2][1] + 1, n


def test_canaries_and_short_caps():
    L = tiffcodec._lib()
    cases = list(lzwfixture.sources()) + [('scan%d' % n, SCAN[:n].tobytes())
                                          for n in (FULL_AT_END,) + WIDER_EOI]
    for name, raw in cases:
        want = tiffcodec.lzw_encode(raw)
        cap = len(raw) * 3 // 2 + 16
        n, out, ok = _run(L.lt_lzw_encode_core, raw, cap)
        assert ok, name
        assert n == len(want) and out[:n].tobytes() == want, name
        assert not out[n:].any(), name  # nothing past the returned count
        n, out, ok = _run(L.lt_lzw_encode_core, raw, len(want))  # the exact size fits
        assert ok and n == len(want) and out.tobytes() == want, name
        for cap in (len(want) - 1, len(want) // 2, 1, 0):
            n, _, ok = _run(L.lt_lzw_encode_core, raw, cap)
            assert ok, (name, cap)
            assert n == ERR_SPACE, (name, cap)


@pytest.mark.parametrize('name,raw', lzwfixture.sources(), ids=[s[0] for s in lzwfixture.sources()])
def test_round_trip(name, raw):
    enc = tiffcodec.lzw_encode_core(raw)
    assert tiffcodec.lzw_decode_core(enc, len(raw)).tobytes() == raw


def test_core_standalone_under_sanitizers(tmp_path):
    """The core in a program of its own (its own main), compiled with AddressSanitizer and UBSan
    and run as a child process: nothing is preloaded, nothing sanitized is loaded into Python."""
    src = os.path.join(ROOT, 'tests', 'native', 'lzw_encode_core_check.cpp')
    exe = str(tmp_path / 'lzw_encode_core_check')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined',
            '-fno-sanitize-recover=all', '-o', exe, src]
    built = False
    for extra in (['-static-libasan', '-static-libubsan'], ['-static-libasan'], []):
        if subprocess.run(base + extra, capture_output=True).returncode == 0:
            built = True
            break
    if not built:
        pytest.skip('g++ cannot link the sanitizer runtimes here')
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith('ok '), r.stdout
