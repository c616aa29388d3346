"""The zonal table's per-pixel code (lt_zonal.h) in a program of its own (tests/native/
zonal_core_check.cpp, its own main), compiled with AddressSanitizer and UBSan and run as a child
process on the cases of zonalfixture with the reference's tables: every buffer on the heap with
exactly the size the ABI names. Nothing is preloaded and nothing sanitized is loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import zonalfixture as zx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_core_standalone_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'native', 'zonal_core_check.cpp')
    exe = str(tmp_path / 'zonal_core_check')
    base = ['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined',
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
        for pattern in zx.PATTERNS:
            for P, Z, B in zx.shapes(pattern):
                if (Z + 1) * (B + 1) > 1 << 16 or (pattern == 'mixed' and P > 16385):
                    continue   # (the tables travel through a file: the small ones)
                c = zx.case(pattern, P, Z, B)
                if c['times'] != 1:
                    continue
                f.write(struct.pack('<8q', P, c['key_lo'], B, Z, c['duration'] is not None,
                                    c['value'] is not None, 0, 0))
                for a in zx.planes(c).values():
                    if a is not None:
                        f.write(np.ascontiguousarray(a).tobytes())
                start = (np.zeros((Z + 1, B + 1, 4), np.int64) if c['start'] is None
                         else c['start'])
                f.write(start.tobytes())
                f.write(zx.case_dense(pattern, P, Z, B).tobytes())
                n += 1
    assert n > 150
    r = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == 'ok %d' % n, r.stdout
