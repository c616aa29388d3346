"""The Deflate core (lt_inflate_core.h) in a program of its own (tests/native/
inflate_core_check.cpp, its own main), compiled with AddressSanitizer and UBSan and run as a child
process on the intact, prefix, corrupt and hand-made streams of inflatefixture with their caps:
every input in a heap buffer of exactly its size, every output in one of exactly cap bytes.
Nothing is preloaded and nothing sanitized is loaded into Python."""
import os
import struct
import subprocess

import pytest

import inflatefixture as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    out = []
    intact = [(s, raw) for _, s, raw in fx.streams()] + [fx.far()]
    for s, raw in intact:
        caps = {len(raw) + 32, len(raw)}
        if len(raw) >= 2:
            caps |= {len(raw) - 1, len(raw) // 2, 1}
        out += [(s, cap) for cap in sorted(caps) if cap >= 1]
    enc, raw = fx.stream('low-l6')
    out += [(enc[:m], len(raw)) for m in range(len(enc) + 1)]
    enc, raw = fx.stream('low-flush')
    out += [(enc[:m], len(raw)) for m in range(0, len(enc) + 1, 7)]
    out += [(s, max(size, 1)) for s, size in fx.corrupt_streams()]
    out += [(s, 64) for _, s in fx.bad_streams()]
    return out


def test_core_standalone_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'native', 'inflate_core_check.cpp')
    exe = str(tmp_path / 'inflate_core_check')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined',
            '-fno-sanitize-recover=all']
    # which way the sanitizer runtimes link here, found with a trivial program: the real build
    # below must then succeed (a compile error in the core is a failure, not a skip)
    probe = tmp_path / 'probe.cpp'
    probe.write_text('int main() { return 0; }\n')
    link = None
    for extra in (['-static-libasan', '-static-libubsan'], ['-static-libasan'], []):
        if subprocess.run(base + extra + ['-o', str(tmp_path / 'probe'), str(probe)],
                          capture_output=True).returncode == 0:
            link = extra
            break
    if link is None:
        pytest.skip('g++ cannot link the sanitizer runtimes here')
    r = subprocess.run(base + link + ['-o', exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = _cases()
    corpus = str(tmp_path / 'corpus.bin')
    n_err = 0
    with open(corpus, 'wb') as f:
        for s, cap in cases:
            want = fx.ref(s, cap)
            n_err += want is None
            f.write(struct.pack('<qqq', len(s), cap, -2 if want is None else len(want)))
            f.write(s)
            f.write(want or b'')
    assert n_err > 500 and len(cases) - n_err > 200  # both outcomes, many times
    r = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == 'ok %d' % len(cases), r.stdout
