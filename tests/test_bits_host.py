"""The point-mask helpers of lt_bits.h (the only code of the analyze / resolve kernels that knows
whether a pixel's masks are 32 or 64 bits wide) in a program of its own (tests/native/
bits_check.cpp, its own main), compiled with AddressSanitizer and UBSan and run as a child process:
for both widths and every bit position each helper equals the 64-bit expression the kernels used,
truncated, including bits_above and 2 << k at the last position and drop_lowest on single-bit
masks. Built with the default and with -DLT_MASK32=0 (the type selection). Nothing is preloaded and
nothing sanitized is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('defs', [[], ['-DLT_MASK32=0']], ids=['default', 'mask32_off'])
def test_bits_standalone_under_sanitizers(tmp_path, defs):
    src = os.path.join(ROOT, 'tests', 'native', 'bits_check.cpp')
    exe = str(tmp_path / 'bits_check')
    base = ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined',
            '-fno-sanitize-recover=all']
    # which way the sanitizer runtimes link here, found with a trivial program: the real build
    # below must then succeed (a compile error in the header is a failure, not a skip)
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
    r = subprocess.run(base + link + defs + ['-o', exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == 'ok', r.stdout
