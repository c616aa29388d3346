"""The MMU sieve's phase steps (lt_sieve.h) in a program of its own (tests/native/
sieve_core_check.cpp, its own main), compiled with AddressSanitizer and UBSan and run as a child
process on the hand-made cases of sievefixture with the reference's outputs: every buffer on the
heap with exactly the size the ABI names. Nothing is preloaded and nothing sanitized is loaded into
Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import sievefixture as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_core_standalone_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'native', 'sieve_core_check.cpp')
    exe = str(tmp_path / 'sieve_core_check')
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
    corpus = str(tmp_path / 'corpus.bin')
    n = 0
    with open(corpus, 'wb') as f:
        for tag in sx.case_tags():
            shape, m, k = sx.case(tag)
            for conn in (4, 8):
                for with_key in (True, False):
                    root, size = sx.case_reference(tag, conn, with_key)
                    for i, min_pixels in enumerate(sx.thresholds(size)[1:]):
                        f.write(struct.pack('<6q', shape[0], shape[1], conn, min_pixels,
                                            int(with_key), (n + i) % 2))
                        f.write(m.tobytes())
                        if with_key:
                            f.write(k.tobytes())
                        f.write(root.tobytes())
                        f.write(size.tobytes())
                        f.write(sx.applied(m, size, min_pixels).tobytes())
                        n += 1
        f.write(struct.pack('<6q', 0, 9, 8, 1, 0, 0))  # nothing to do
        n += 1
    assert n > 600
    r = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == 'ok %d' % n, r.stdout
