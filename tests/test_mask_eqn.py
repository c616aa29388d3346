"""settings.json mask_eqn on the host: the grammar and typing of index_eqn.MaskProgram, its numpy
evaluation against numpy's own evaluation of the expression text, the generated HIP source
(lt_mask_codegen: compiles for gfx950, rejects malformed programs; the generator stand-alone under
AddressSanitizer / UBSan), and a LocalJob on the CPU engine double against the equivalent
`_cloudmask` job. Every comparison is exact."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import maskfixture as mf
from land_trendr_amd import _abi, index_eqn
from land_trendr_amd.index_eqn import MaskProgram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMBERS = [1, 2, 3, 4]


# ---- parsing and typing ----
def test_accepted_grammar_and_node_types():
    p = MaskProgram('B3 != 0', np.int16, NUMBERS)
    assert p.bands == [3] and p.slots == [2] and p.band_numbers == NUMBERS
    assert [op for op, _, _ in p.ops] == [_abi.LT_OP_BAND, _abi.LT_OP_CONST_I, _abi.LT_OP_NE]
    assert p.ops[-1][1] == np.int16  # compared in the legacy promotion of (int16, 0)
    # a band's slot is its position in band_numbers, not among the expression's own bands
    assert MaskProgram('B6 > B2', np.int16, [2, 4, 6]).slots == [0, 2]
    # Python precedence as ast gives it: B3 & 6 == 0 is (B3 & 6) == 0
    p = MaskProgram('B3 & 6 == 0', np.uint8, NUMBERS)
    assert [op for op, _, _ in p.ops] == [_abi.LT_OP_BAND, _abi.LT_OP_CONST_I, _abi.LT_OP_AND,
                                          _abi.LT_OP_CONST_I, _abi.LT_OP_EQ]
    # comparison operands promote as arithmetic nodes do (index_eqn.result_dtype)
    assert MaskProgram('B1 + 40000 > 40000', np.int16, NUMBERS).ops[-1][1] == np.int32
    assert MaskProgram('B1 > -1', np.uint8, NUMBERS).ops[-1][1] == np.int16
    assert MaskProgram('B1 > 0.5', np.int16, NUMBERS).ops[-1][1] == np.float64
    assert MaskProgram('B1 > 0.5', np.float32, NUMBERS).ops[-1][1] == np.float32
    # booleans combine through & | ^ ~ == != with booleans
    p = MaskProgram('~(B1 > 0) ^ (B2 > 0) | (B3 == 0) == (B4 != 0)', np.int16, NUMBERS)
    assert all(t == np.bool_ for op, t, _ in p.ops
               if op in (_abi.LT_OP_NOT, _abi.LT_OP_XOR, _abi.LT_OP_OR))
    # a shift carries its literal count; its node has the promoted type of (operand, count)
    p = MaskProgram('(B3 >> 15) & 1 == 1', np.int16, NUMBERS)
    assert (_abi.LT_OP_SHR, np.dtype(np.int16), 15) in p.ops
    assert MaskProgram('B3 << 7 != 0', np.uint8, NUMBERS).ops[1] == (_abi.LT_OP_SHL,
                                                                     np.dtype(np.uint8), 7)
    # scalar-only sub-expressions fold on the host (Python 2 rules: 7 / 2 floors)
    p = MaskProgram('B1 > (1 << 4) + 7 / 2', np.int16, NUMBERS)
    assert p.ops[1] == (_abi.LT_OP_CONST_I, np.dtype(np.int64), 19) and len(p.ops) == 3
    p = MaskProgram('(1 < 2) & (B1 > 0)', np.int16, NUMBERS)
    assert p.ops[0] == (_abi.LT_OP_CONST_I, np.dtype(np.bool_), 1)
    # to_c: the existing lt_index_prog, n_bands the planes of the stack
    c = MaskProgram('B3 != 0', np.int16, NUMBERS).to_c()
    assert (c.n_ops, c.n_bands, c.band_type) == (3, 4, _abi.LT_T_I16)
    assert (c.ops[0].ival, c.ops[2].op, c.ops[2].type) == (2, _abi.LT_OP_NE, _abi.LT_T_I16)
    c = MaskProgram('(B1 > 0) & (B2 > 0)', np.int16, NUMBERS).to_c()
    assert c.ops[c.n_ops - 1].type == _abi.LT_T_BOOL == 9


REJECTED = [
    'B1 > 0 and B2 > 0', 'B1 > 0 or B2 > 0', 'not B1 > 0', '0 < B1 < 5',     # numpy raises
    '(B1 > 0) + 1', '(B1 > 0) * (B2 > 0)', '-(B1 > 0)', '(B1 > 0) / 2',       # bool arithmetic
    'B1 - B2', 'B3 & 6', 'B3 >> 2', '~B3',                                    # non-boolean root
    '(B1 > 0) & B3', '(B1 > 0) == 1', '(B1 > 0) < (B2 > 0)',                  # bool with number
    'B3 >> 16 == 0', 'B3 << -1 == 0', 'B3 >> B1 == 0', 'B3 >> 1.0 == 0', '1 >> B3 == 0',
    '3 > 2', '(1 < 2) == (2 < 3)',                                            # no band
    'C1 > 0', 'abs(B1) > 0', 'B1.real > 0', 'np.where(B1 > 0, 1, 0) == 1',    # names, calls
    'B1 ** 2 > 0', 'B1 % 3 == 0', 'B1 >', 'B1 is B2', 'B1 in B2', 'True & (B1 > 0)',
    ' & '.join('(B%d > 0)' % (1 + k % 4) for k in range(17)),                 # 67 operations
]


@pytest.mark.parametrize('eqn', REJECTED)
def test_rejected_expressions(eqn):
    with pytest.raises(ValueError, match='mask_eqn'):
        MaskProgram(eqn, np.int16, NUMBERS)


def test_rejected_by_type():
    for eqn in ('B1 & 1 == 1', 'B1 | B2 != 0', '~B1 == 0', 'B1 ^ 1 == 0', 'B1 >> 1 == 0',
                'B1 * 0.5 & 1 == 0'):
        with pytest.raises(ValueError, match='mask_eqn'):
            MaskProgram(eqn, np.float32, NUMBERS)
    with pytest.raises(ValueError, match='mask_eqn'):
        MaskProgram('B3 & 1.5 == 0', np.int16, NUMBERS)
    with pytest.raises(ValueError, match='mask_eqn'):  # a shift count past the uint8 node
        MaskProgram('B3 >> 8 == 0', np.uint8, NUMBERS)
    with pytest.raises(ValueError, match='more than %d bands' % _abi.LT_MAX_BANDS):
        MaskProgram('B1 > 0', np.int16, list(range(1, 18)))
    with pytest.raises(ValueError, match='more than %d operations' % _abi.LT_MAX_PROG):
        MaskProgram(' | '.join('(B%d != %d)' % (1 + k % 4, k) for k in range(17)), np.int16,
                    NUMBERS)
    # 64 operations and 16 bands are accepted
    p = MaskProgram(_eqn64(), np.int16, list(range(1, 17)))
    assert len(p.ops) == _abi.LT_MAX_PROG and len(p.slots) == _abi.LT_MAX_BANDS


def _eqn64():
    return '~(B1 > 0) & ' + ' & '.join('(B%d > 0)' % b for b in range(2, 17))


def test_band_number_errors_have_the_reference_messages():
    with pytest.raises(Exception, match='Band 7 not present'):
        MaskProgram('B7 != 0', np.int16, [1, 2, 7], raster_count=6)
    with pytest.raises(Exception, match='Band 3 not present'):
        MaskProgram('B3 != 0', np.int16, [1, 2])  # not among the planes
    with pytest.raises(Exception, match='Invalid band'):
        MaskProgram('B0 != 0', np.int16, [1, 2])


def test_index_eqn_still_rejects_the_mask_operators():
    for eqn in ('B1 > 0', 'B1 & 3', 'B1 >> 2', '~B1', 'B1 == B2'):
        with pytest.raises(ValueError, match='index_eqn'):
            index_eqn.IndexProgram(eqn)


# ---- MaskProgram.evaluate against numpy ----
CASES = [(eqn, dt) for eqn, dts in mf.CORPUS for dt in dts]


@pytest.fixture(scope='module')
def bands_by_type():
    return {np.dtype(dt): mf.band_values(dt, (4, 3, 211), seed=3) for dt in mf.DTYPES}


@pytest.mark.parametrize('eqn,dt', CASES)
def test_evaluate_equals_numpy(eqn, dt, bands_by_type):
    b = bands_by_type[np.dtype(dt)]
    got = MaskProgram(eqn, dt, NUMBERS).evaluate(b)
    want = mf.numpy_mask(eqn, b)
    assert got.dtype == np.bool_ and got.shape == want.shape
    assert np.array_equal(got, want)
    if eqn != 'B1 == B1' or np.dtype(dt).kind == 'f':
        assert want.any() and not want.all()  # the inputs reach both outcomes


def test_evaluate_known_answers_where_the_promotions_differ_or_wrap():
    i16 = np.array([[32767, -32768, 0, -1, 5]], np.int16)
    # (B1 + 1) wraps in int16: 32767 + 1 = -32768, which is not above 32767
    assert MaskProgram('(B1 + 1) > B1', np.int16, [1]).evaluate(i16).tolist() == \
        [False, True, True, True, True]
    # int16 + 40000 is an int32 node (legacy value-based promotion): no wrap
    assert MaskProgram('B1 + 40000 > 40000', np.int16, [1]).evaluate(i16).tolist() == \
        [True, False, False, False, True]
    u8 = np.array([[0, 1, 255, 128]], np.uint8)
    # compared in int16: every uint8 is above -1 (numpy 2.x raises on the literal instead)
    assert MaskProgram('B1 > -1', np.uint8, [1]).evaluate(u8).all()
    assert MaskProgram('B1 + 1 > 0', np.uint8, [1]).evaluate(u8).tolist() == \
        [True, True, False, True]  # 255 + 1 wraps to 0 in uint8
    assert MaskProgram('B1 << 1 == 0', np.uint8, [1]).evaluate(u8).tolist() == \
        [True, False, False, True]  # 128 << 1 wraps to 0
    # Python 2 classic division floors on integers; a division by zero gives 0
    d = np.array([[7, -7, 1, 0]], np.int16)
    assert MaskProgram('B1 / 2 == -4', np.int16, [1]).evaluate(d).tolist() == \
        [False, True, False, False]
    assert MaskProgram('5 / B1 == 0', np.int16, [1]).evaluate(d).tolist() == \
        [True, False, False, True]
    # an arithmetic shift keeps the sign
    assert MaskProgram('B1 >> 15 == -1', np.int16, [1]).evaluate(i16).tolist() == \
        [False, True, False, True, False]
    f = np.array([[np.nan, 1.0, -np.inf, 0.0]], np.float32)
    assert MaskProgram('B1 == B1', np.float32, [1]).evaluate(f).tolist() == \
        [False, True, True, True]
    assert MaskProgram('~(B1 > 0)', np.float32, [1]).evaluate(f).tolist() == \
        [True, False, True, True]


# ---- generated source ----
def _codegen(prog_c):
    lib = _abi.load_lib()
    n = lib.lt_mask_codegen(ctypes.byref(prog_c), None, 0)
    if n < 0:
        return n
    buf = ctypes.create_string_buffer(n + 1)
    assert lib.lt_mask_codegen(ctypes.byref(prog_c), buf, n + 1) == n
    return buf.value.decode()


def test_codegen_compiles_for_gfx950(tmp_path):
    picks = [('B3 & 6 == 0', np.uint8), ('~(B3 >> 3) & 1 == 1', np.int16),
             ('(B4 - B3) / (B4 + B3) > 0', np.float32), ('(B1 <= B2) | (B3 >= 100) ^ (B2 < 7)',
                                                         np.int32), ('B1 > 0.5', np.uint16)]
    for k, (eqn, dt) in enumerate(picks):
        src = _codegen(MaskProgram(eqn, dt, NUMBERS).to_c())
        assert 'lt_mask_kernel(' in src and 'lt_mask_kernel_v4(' in src and eqn not in src
        wide = 'lt_mask_kernel_v%d(' % max(4, 16 // np.dtype(dt).itemsize)
        assert wide in src  # 16-byte band loads
        f = tmp_path / ('mask%d.hip' % k)
        f.write_text('#include <hip/hip_runtime.h>\n' + src)  # hiprtc provides it implicitly
        subprocess.check_call(['/opt/rocm/bin/hipcc', '-x', 'hip', '--offload-arch=gfx950',
                               '--cuda-device-only', '-c', '-O3', '-ffp-contract=off', '-o',
                               str(tmp_path / ('mask%d.o' % k)), str(f)])


def _malformed():
    """(what, program) of programs a host could hand over that the generator must refuse."""
    out = []
    p = MaskProgram('B1 > B2', np.int16, NUMBERS).to_c()
    p.n_ops = 2
    out.append(('unbalanced stack', p))
    p = MaskProgram('B1 > B2', np.int16, NUMBERS).to_c()
    p.n_ops = 1
    out.append(('non-boolean root', p))
    p = MaskProgram('B1 > B2', np.int16, NUMBERS).to_c()
    p.ops[0].ival = 4
    out.append(('slot out of range', p))
    p = MaskProgram('B1 > B2', np.int16, NUMBERS).to_c()
    p.ops[1].ival = -1
    out.append(('negative slot', p))
    p = MaskProgram('(B1 > 0) & (B2 > 0)', np.int16, NUMBERS).to_c()
    p.ops[p.n_ops - 1].op = _abi.LT_OP_ADD
    out.append(('boolean into arithmetic', p))
    p = MaskProgram('(B1 > 0) & (B2 > 0)', np.int16, NUMBERS).to_c()
    p.ops[p.n_ops - 1].type = _abi.LT_T_I16
    out.append(('booleans into an integer node', p))
    p = MaskProgram('B3 >> 3 == 0', np.int16, NUMBERS).to_c()
    p.ops[1].ival = 99
    out.append(('shift count 99', p))
    p = MaskProgram('B3 >> 3 == 0', np.int16, NUMBERS).to_c()
    p.ops[1].type = _abi.LT_T_F32
    out.append(('shift in a float node', p))
    p = MaskProgram('B3 != 0', np.int16, NUMBERS).to_c()
    p.ops[2].op = 22
    out.append(('unknown opcode', p))
    p = MaskProgram('B3 != 0', np.int16, NUMBERS).to_c()
    p.ops[2].type = 10
    out.append(('unknown type', p))
    p = MaskProgram('B3 != 0', np.int16, NUMBERS).to_c()
    p.n_bands = 17
    out.append(('too many bands', p))
    p = MaskProgram('B3 != 0', np.int16, NUMBERS).to_c()
    p.n_ops = 65
    out.append(('too many operations', p))
    p = MaskProgram('B3 != 0', np.int16, NUMBERS).to_c()
    p.ops[0].op = _abi.LT_OP_NOT
    out.append(('stack underflow', p))
    return out


def test_codegen_rejects_malformed_programs():
    for what, p in _malformed():
        assert _codegen(p) < 0, what
    lib = _abi.load_lib()
    assert lib.lt_mask_codegen(None, None, 0) < 0
    # the index generator does not take a mask program
    p = MaskProgram('B3 != 0', np.int16, NUMBERS).to_c()
    p.out_type = _abi.LT_T_I16
    assert lib.lt_index_codegen(ctypes.byref(p), None, 0) < 0


def test_codegen_standalone_under_sanitizers(tmp_path):
    """The code generator in a program of its own (its own main), its host code compiled with
    AddressSanitizer and UBSan and run as a child process over the corpus, a 64-operation 16-band
    program and the malformed programs: nothing is preloaded, nothing sanitized is loaded into
    Python."""
    src = os.path.join(ROOT, 'tests', 'native', 'mask_codegen_check.cpp')
    exe = str(tmp_path / 'mask_codegen_check')
    base = ['g++', '-O1', '-g', '-std=c++17', '-D__HIP_PLATFORM_AMD__', '-I/opt/rocm/include',
            '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-o', exe, src]
    errs = []
    for extra in (['-static-libasan', '-static-libubsan'], ['-static-libasan'], []):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        if r.returncode == 0:
            break
        errs.append(r.stderr)
    assert r.returncode == 0, '\n'.join(errs)
    progs = [(1, MaskProgram(eqn, dt, NUMBERS).to_c()) for eqn, dt in CASES]
    progs.append((1, MaskProgram(_eqn64(), np.int16, list(range(1, 17))).to_c()))
    progs.append((1, MaskProgram(_eqn64().replace('> 0', '> -9223372036854775807'), np.float32,
                                 list(range(1, 17))).to_c()))
    progs += [(0, p) for _, p in _malformed()]
    with open(tmp_path / 'progs.bin', 'wb') as fh:
        for ok, p in progs:
            fh.write(struct.pack('i', ok) + bytes(p))
    r = subprocess.run([exe, str(tmp_path / 'progs.bin')], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith('ok %d accepted, %d rejected' % (len(CASES) + 2,
                                                                len(_malformed()))), r.stdout


def test_mask_io_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of lt_mask_io from a C program against the ctypes mirror."""
    header = os.path.join(ROOT, 'include', 'lt_abi.h')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % header,
             'int main(void){', 'printf("size %zu\\n", sizeof(lt_mask_io));']
    for f, _ in _abi.LtMaskIO._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(lt_mask_io, %s));' % (f, f))
    lines.append('return 0;}')
    (tmp_path / 'l.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-o', str(tmp_path / 'l'), str(tmp_path / 'l.c')])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / 'l')],
                                                          text=True).splitlines())
    assert int(got['size']) == ctypes.sizeof(_abi.LtMaskIO)
    for f, _ in _abi.LtMaskIO._fields_:
        assert int(got[f]) == getattr(_abi.LtMaskIO, f).offset, f


# ---- a job on the CPU engine double ----
def test_cpu_job_mask_eqn_equals_the_cloudmask_job(tmp_path):
    from engine_double import OracleEngine
    from land_trendr_amd.job import LocalJob
    jobs = {}
    for mode in ('eqn', 'cloud'):
        root = str(tmp_path / mode)
        mf.make_mask_job(root, mode)
        j = jobs[mode] = LocalJob(root, 'synth', tile_pixels=40, on_error='skip',
                                  engine=OracleEngine())
        j.setup()
        j.parse()
        j.analyze()
    e, c = jobs['eqn'], jobs['cloud']
    assert e.stack['band_numbers'] == [1, 2, 3] and c.stack['band_numbers'] == [1, 2]
    assert len(e.mosaic.mine) >= 3
    assert sorted(e.planes) == sorted(c.planes)
    for k in e.planes:
        assert np.asarray(e.planes[k]).tobytes() == np.asarray(c.planes[k]).tobytes(), k
    # the mask is not written into the stack: its validity stays the ingest's (coverage only)
    b, v = e.stack['bands'], e.stack['valid']
    keep = b[:, 2, :] != 0
    assert np.array_equal(np.where(keep, v, 0), c.stack['valid'])
    assert c.mask_stats is None
    assert e.mask_stats == {'eqn': 'B3 != 0', 'observations': int(np.count_nonzero(v)),
                            'dropped': int(np.count_nonzero((v != 0) & ~keep))}
    assert 0 < e.mask_stats['dropped'] < e.mask_stats['observations']
    # the job did label something with the masked observations gone
    assert e.planes['matched'].any()
