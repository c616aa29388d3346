"""The change maps' per-pixel code (lt_change.h) in a program of its own (tests/native/
change_core_check.cpp, its own main), compiled with AddressSanitizer and UBSan and run as a child
process on the hand-made cases of changefixture with the reference's outputs: every buffer on the
heap with exactly the size the ABI names. Nothing is preloaded and nothing sanitized is loaded into
Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

import changefixture as cx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_core_standalone_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'native', 'change_core_check.cpp')
    exe = str(tmp_path / 'change_core_check')
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
        for tag in cx.case_tags():
            rules, kw = cx.case(tag)
            want = cx.case_reference(tag)
            Y, P = kw['val_fit'].shape
            fit = 'val_raw' in kw
            kind = 1 if 'present' in kw else 2 if 'winner' in kw else 0
            f.write(struct.pack('<6q', P, Y, len(rules), kind, int(fit), 0))
            f.write(np.ascontiguousarray(kw['years'], np.int32).tobytes())
            f.write(bytes(cx.c_rules(rules)))
            f.write(np.ascontiguousarray(kw['val_fit'], np.float64).tobytes())
            f.write(np.ascontiguousarray(kw['vertex'], np.uint8).tobytes())
            if kind == 1:
                f.write(np.ascontiguousarray(kw['present'], np.uint8).tobytes())
            elif kind == 2:
                f.write(np.ascontiguousarray(kw['winner'], np.int16).tobytes())
            if fit:
                f.write(np.ascontiguousarray(kw['val_raw'], np.float64).tobytes())
                f.write(np.ascontiguousarray(kw['spike'], np.uint8).tobytes())
            for fld in cx.default_fields(fit):
                f.write(np.ascontiguousarray(want[fld], cx.DTYPE[fld]).tobytes())
            n += 1
        f.write(struct.pack('<6q', 0, 5, 1, 0, 0, 0))  # nothing to do
        f.write(np.arange(5, dtype=np.int32).tobytes())
        f.write(bytes(cx.c_rules([{'delta': 'loss'}])))
        n += 1
    assert n > 90
    r = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == 'ok %d' % n, r.stdout
