"""settings.json `index_eqn` (README.md:47, :75) compiled for the GPU load stage.

The reference evaluates the equation per raster with Python 2 `eval` on numpy band arrays
(`rast_algebra`, utils.py:447-484; band names from `parse_eqn_bands`, utils.py:219-225) and
writes the result with the input raster's band type (`array2raster`, utils.py:374-412, data_type
taken from the template at :396-397); `apply_grid` then reads it back as `float(val)`
(utils.py:357). Here the equation is parsed into a typed postfix program (no `eval`): the arithmetic
subset — band names B<n>, int and float literals, + - * / // and unary +/- with parentheses —
with numpy 1.x semantics as the reference ran them under Python 2:

  * dtypes follow numpy's legacy value-based promotion: array (+) array -> promote_types; array (+)
    Python scalar -> the scalar's min_scalar_type joins the promotion when its kind is not above
    the array's (int16 - 1 stays int16, int16 + 40000 becomes int32), else the scalar's own type
    (int16 * 0.5 -> float64);
  * integer results wrap (two's complement); `/` on integers is floor division (Python 2
    classic division), division by zero gives 0 (numpy's integer loops);
  * scalar-only subexpressions fold with Python 2 rules (int / int floors).

The store into the template type (GDAL's conversion, not available here) is: identity for the same
type, saturation for a narrower integer type, round-half-up (floor(x + 0.5)) then saturation for
float -> integer, NaN -> 0. Those three rules are parity-unpinned (no GDAL in this image); the
arithmetic is pinned by numpy itself (tests/test_index_eqn.py).

The program is compiled to a device kernel with hiprtc by the C++ side (lt_index_compile); the
kernel source is generated there from the program, never from the equation text.

settings.json `mask_eqn` (rast_algebra's mask_eqn parameter, dead in the reference) goes the same
way: MaskProgram shares the emitter, adds comparisons, bitwise operators and shifts by a literal,
and must end in a boolean; lt_mask_compile / lt_mask_apply clear the validity bytes of the
observations it is false on.
"""
import ast
import re

import numpy as np

from . import _abi

# numpy dtype <-> LT_T_* element type codes (include/lt_abi.h)
DTYPES = {
    np.dtype(np.float64): _abi.LT_T_F64,
    np.dtype(np.int16): _abi.LT_T_I16,
    np.dtype(np.uint16): _abi.LT_T_U16,
    np.dtype(np.int32): _abi.LT_T_I32,
    np.dtype(np.float32): _abi.LT_T_F32,
    np.dtype(np.uint8): _abi.LT_T_U8,
    np.dtype(np.uint32): _abi.LT_T_U32,
    np.dtype(np.int8): _abi.LT_T_I8,
    np.dtype(np.int64): _abi.LT_T_I64,
}
CODES = {v: k for k, v in DTYPES.items()}

_BAND = re.compile(r'B(?P<band_num>\d+)')
_KIND_RANK = {'b': 0, 'u': 1, 'i': 1, 'f': 2}


def parse_eqn_bands(eqn):
    """Band numbers an equation references (utils.py:219-225): '(B2-B2)/(B3+B4)-B6' -> 2, 3, 4, 6.
    The reference returns them in set order; sorted here."""
    return sorted(int(d) for d in set(_BAND.findall(eqn)))


def multiple_replace(string, replacements):
    """utils.py:227-236: every key of `replacements` replaced in one regex pass."""
    pattern = re.compile('|'.join(replacements.keys()))
    return pattern.sub(lambda x: replacements[x.group()], string)


def _min_scalar_type(v, signed_array=False):
    """numpy's legacy min_scalar_type, with its 'small unsigned' rule: a non-negative integer
    that fits the signed type of its width promotes as that signed type next to a signed array
    (int8 array + 1000 -> int16, not int32)."""
    if isinstance(v, float):
        return np.min_scalar_type(v)
    order = ((np.int8, np.int16, np.int32, np.int64) if v < 0 or signed_array else
             (np.uint8, np.uint16, np.uint32, np.uint64))
    for t in order:
        info = np.iinfo(t)
        if info.min <= v <= info.max:
            return np.dtype(t)
    if v >= 0 and signed_array and v <= np.iinfo(np.uint64).max:
        return np.dtype(np.uint64)
    raise ValueError('index_eqn: integer literal %r out of range' % v)


def _scalar_default_type(v):
    return np.dtype(np.float64) if isinstance(v, float) else np.dtype(np.int64)  # Py2 int = C long


def result_dtype(a, b):
    """numpy 1.x (legacy) result type of an operation on a and b, each either a np.dtype (an
    array operand) or a Python int/float (a scalar operand)."""
    arrays = [x for x in (a, b) if isinstance(x, np.dtype)]
    scalars = [x for x in (a, b) if not isinstance(x, np.dtype)]
    if not scalars:
        return np.promote_types(a, b)
    t = arrays[0]
    s = scalars[0]
    s_kind = 'f' if isinstance(s, float) else 'i'
    if _KIND_RANK[s_kind] <= _KIND_RANK[t.kind]:
        return np.promote_types(t, _min_scalar_type(s, t.kind == 'i'))
    return np.promote_types(t, _scalar_default_type(s))


def _py2_binop(op, x, y):
    if isinstance(op, ast.Add):
        return x + y
    if isinstance(op, ast.Sub):
        return x - y
    if isinstance(op, ast.Mult):
        return x * y
    if isinstance(op, (ast.Div, ast.FloorDiv)):
        if isinstance(x, int) and isinstance(y, int):
            return x // y  # Python 2 classic division of ints floors; ZeroDivisionError as in Py2
        return x / y if isinstance(op, ast.Div) else float(np.floor(x / y))
    raise ValueError('index_eqn: unsupported operator %s' % type(op).__name__)


_OPS = {ast.Add: _abi.LT_OP_ADD, ast.Sub: _abi.LT_OP_SUB, ast.Mult: _abi.LT_OP_MUL,
        ast.Div: _abi.LT_OP_DIV, ast.FloorDiv: _abi.LT_OP_FLOORDIV}
# mask_eqn only: comparisons, bitwise operators and shifts by a literal
_CMP = {ast.Eq: _abi.LT_OP_EQ, ast.NotEq: _abi.LT_OP_NE, ast.Lt: _abi.LT_OP_LT,
        ast.LtE: _abi.LT_OP_LE, ast.Gt: _abi.LT_OP_GT, ast.GtE: _abi.LT_OP_GE}
_BIT = {ast.BitAnd: _abi.LT_OP_AND, ast.BitOr: _abi.LT_OP_OR, ast.BitXor: _abi.LT_OP_XOR}
_SHIFT = {ast.LShift: _abi.LT_OP_SHL, ast.RShift: _abi.LT_OP_SHR}
BOOL = np.dtype(bool)
# node type -> LT_T_* (a mask program's comparison and boolean nodes carry LT_T_BOOL)
TYPE_CODES = dict(DTYPES)
TYPE_CODES[BOOL] = _abi.LT_T_BOOL


class _Program:
    """The emitter IndexProgram and MaskProgram share: an `ast` expression over B<n> to typed
    postfix ops (op, dtype, value). `_tag` prefixes the error messages; `_mask` admits the
    comparison / bitwise / shift nodes; `_slot(n)` is the band plane of reference band n."""
    _tag = 'index_eqn'
    _mask = False

    def _slot(self, number):
        return self.bands.index(number)

    def _parse(self, eqn):
        try:
            tree = ast.parse(eqn.strip(), mode='eval')
        except SyntaxError as e:
            raise ValueError('%s: %s' % (self._tag, e))
        self.ops = []
        return self._emit(tree.body)

    def _arith(self, v):
        """v as an arithmetic operand: booleans take no part in arithmetic."""
        if v == BOOL if isinstance(v, np.dtype) else isinstance(v, bool):
            raise ValueError('%s: arithmetic on a boolean' % self._tag)
        return v

    # Returns the operand: a np.dtype for an array value (code emitted) or a Python scalar.
    def _emit(self, node):
        if isinstance(node, ast.Name):
            m = re.fullmatch(r'B(\d+)', node.id)
            if not m:
                raise ValueError('%s: unknown name %r' % (self._tag, node.id))
            self.ops.append((_abi.LT_OP_BAND, self.band_dtype, self._slot(int(m.group(1)))))
            return self.band_dtype
        if isinstance(node, ast.Constant) and type(node.value) in (int, float):
            return node.value
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            v = self._arith(self._emit(node.operand))
            if not isinstance(v, np.dtype):
                return -v if isinstance(node.op, ast.USub) else +v
            if isinstance(node.op, ast.USub):
                self.ops.append((_abi.LT_OP_NEG, v, 0))
            return v
        if isinstance(node, ast.BinOp) and type(node.op) in _OPS:
            # evaluate both sides first (postfix), scalars become typed constants
            n0 = len(self.ops)
            a = self._arith(self._emit(node.left))
            b = self._arith(self._emit(node.right))
            if not isinstance(a, np.dtype) and not isinstance(b, np.dtype):
                return _py2_binop(node.op, a, b)
            return self._binary(_OPS[type(node.op)], n0, a, b, result_dtype(a, b))
        if self._mask:
            r = self._emit_mask(node)
            if r is not None:
                return r
        raise ValueError('%s: unsupported expression %s' % (self._tag, ast.dump(node)))

    def _binary(self, op, n0, a, b, t, result=None):
        """The op node of type t over operands a and b (code from ops[n0:]); a scalar operand
        becomes a typed constant in its place."""
        if not isinstance(a, np.dtype):
            self.ops.insert(n0, self._const(a))  # before the right operand's code
        if not isinstance(b, np.dtype):
            self.ops.append(self._const(b))
        self.ops.append((op, t, 0))
        return t if result is None else result

    def _pair_type(self, a, b, what):
        """Node type of a comparison or bitwise node: booleans only meet booleans, the others
        promote as the arithmetic nodes do."""
        a_bool = a == BOOL if isinstance(a, np.dtype) else isinstance(a, bool)
        b_bool = b == BOOL if isinstance(b, np.dtype) else isinstance(b, bool)
        if a_bool != b_bool:
            raise ValueError('%s: %s of a boolean and a number' % (self._tag, what))
        if not isinstance(a, np.dtype) and not isinstance(b, np.dtype):
            return None  # two scalars: folded on the host
        return BOOL if a_bool else result_dtype(a, b)

    def _emit_mask(self, node):
        tag = self._tag
        if isinstance(node, ast.Compare):
            if len(node.ops) != 1:
                raise ValueError('%s: chained comparison (numpy raises on arrays)' % tag)
            if type(node.ops[0]) not in _CMP:
                raise ValueError('%s: unsupported comparison %s' % (tag, ast.dump(node.ops[0])))
            n0 = len(self.ops)
            a = self._emit(node.left)
            b = self._emit(node.comparators[0])
            op = _CMP[type(node.ops[0])]
            t = self._pair_type(a, b, 'comparison')
            if (isinstance(a, bool) or (isinstance(a, np.dtype) and a == BOOL)) and \
                    op not in (_abi.LT_OP_EQ, _abi.LT_OP_NE):
                raise ValueError('%s: booleans compare with == and != only' % tag)
            if not isinstance(a, np.dtype) and not isinstance(b, np.dtype):
                return _fold(op, a, b)
            return self._binary(op, n0, a, b, t, BOOL)
        if isinstance(node, ast.BinOp) and type(node.op) in _BIT:
            n0 = len(self.ops)
            a = self._emit(node.left)
            b = self._emit(node.right)
            op = _BIT[type(node.op)]
            for v in (a, b):
                if v.kind == 'f' if isinstance(v, np.dtype) else isinstance(v, float):
                    raise ValueError('%s: bitwise operator on a float' % tag)
            t = self._pair_type(a, b, 'bitwise operator')
            if not isinstance(a, np.dtype) and not isinstance(b, np.dtype):
                return _fold(op, a, b)
            return self._binary(op, n0, a, b, t)
        if isinstance(node, ast.BinOp) and type(node.op) in _SHIFT:
            a = self._emit(node.left)
            cnt = node.right
            if not (isinstance(cnt, ast.Constant) and type(cnt.value) is int):
                raise ValueError('%s: a shift count must be an integer literal' % tag)
            n = cnt.value
            op = _SHIFT[type(node.op)]
            if isinstance(a, np.dtype):
                if a.kind not in 'iu':
                    raise ValueError('%s: shift of a %s' % (tag, a))
                t = result_dtype(a, n) if n >= 0 else a
            elif type(a) is int:
                t = np.dtype(np.int64)  # a folded scalar: Python 2 int = C long
            else:
                raise ValueError('%s: shift of a %s' % (tag, type(a).__name__))
            if t.kind not in 'iu' or not 0 <= n < 8 * t.itemsize:
                raise ValueError('%s: shift count %d outside [0, %d] of %s'
                                 % (tag, n, 8 * t.itemsize - 1, t))
            if not isinstance(a, np.dtype):
                return _fold(op, a, n)
            self.ops.append((op, t, n))
            return t
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.Invert):
            v = self._emit(node.operand)
            if isinstance(v, np.dtype):
                if v.kind == 'f':
                    raise ValueError('%s: bitwise operator on a float' % tag)
                self.ops.append((_abi.LT_OP_NOT, v, 0))
                return v
            if isinstance(v, float):
                raise ValueError('%s: bitwise operator on a float' % tag)
            return (not v) if isinstance(v, bool) else ~v
        if isinstance(node, (ast.BoolOp,)) or (isinstance(node, ast.UnaryOp) and
                                                isinstance(node.op, ast.Not)):
            raise ValueError('%s: and / or / not are not defined on arrays (numpy raises); '
                             'use & | ~' % tag)
        return None

    @staticmethod
    def _const(v):
        if isinstance(v, bool):
            return (_abi.LT_OP_CONST_I, BOOL, int(v))
        if isinstance(v, float):
            return (_abi.LT_OP_CONST_F, np.dtype(np.float64), v)
        return (_abi.LT_OP_CONST_I, np.dtype(np.int64), v)

    def _fill(self, p):
        for k, (op, t, v) in enumerate(self.ops):
            p.ops[k].op = op
            p.ops[k].type = TYPE_CODES[np.dtype(t)]
            if op == _abi.LT_OP_CONST_F:
                p.ops[k].fval = float(v)
            else:
                p.ops[k].ival = int(v)
        return p


def _fold(op, x, y):
    """A comparison, bitwise or shift node of two scalars, folded on the host."""
    return {_abi.LT_OP_EQ: lambda: x == y, _abi.LT_OP_NE: lambda: x != y,
            _abi.LT_OP_LT: lambda: x < y, _abi.LT_OP_LE: lambda: x <= y,
            _abi.LT_OP_GT: lambda: x > y, _abi.LT_OP_GE: lambda: x >= y,
            _abi.LT_OP_AND: lambda: x & y, _abi.LT_OP_OR: lambda: x | y,
            _abi.LT_OP_XOR: lambda: x ^ y, _abi.LT_OP_SHL: lambda: x << y,
            _abi.LT_OP_SHR: lambda: x >> y}[op]()


class IndexProgram(_Program):
    """A validated, typed postfix program for one index_eqn.

    bands: the reference band numbers (1-based) the equation uses, in the order of the band planes
    the load kernel receives (plane s holds band bands[s]). ops: (op, dtype, ival, fval) tuples.
    """

    def __init__(self, eqn, band_dtype=np.int16, out_dtype=None, raster_count=None):
        self.eqn = eqn
        self.band_dtype = np.dtype(band_dtype)
        self.out_dtype = np.dtype(out_dtype) if out_dtype is not None else self.band_dtype
        if self.band_dtype not in DTYPES or self.out_dtype not in DTYPES:
            raise ValueError('index_eqn: unsupported raster type %s / %s' %
                             (self.band_dtype, self.out_dtype))
        bands = parse_eqn_bands(eqn)
        if not bands:
            raise ValueError('index_eqn: %r references no band' % eqn)
        # rast_algebra's own checks (utils.py:462-465), same messages
        if raster_count is not None and max(bands) > raster_count:
            raise Exception('Band %s not present in %s' % (max(bands), '<raster>'))
        if min(bands) <= 0:
            raise Exception('Invalid band "%s" - bands must be >= 1')
        self.bands = bands
        root = self._parse(eqn)
        if not isinstance(root, np.dtype):  # a constant equation: numpy broadcasts it
            self.ops.append((_abi.LT_OP_CONST_F if isinstance(root, float) else _abi.LT_OP_CONST_I,
                             _scalar_default_type(root), root))
            root = _scalar_default_type(root)
        self.result_dtype = root
        if len(self.ops) > _abi.LT_MAX_PROG:
            raise ValueError('index_eqn: more than %d operations' % _abi.LT_MAX_PROG)
        if len(self.bands) > _abi.LT_MAX_BANDS:
            raise ValueError('index_eqn: more than %d bands' % _abi.LT_MAX_BANDS)

    def to_c(self):
        p = _abi.LtIndexProg()
        p.n_ops = len(self.ops)
        p.n_bands = len(self.bands)
        p.band_type = DTYPES[self.band_dtype]
        p.out_type = DTYPES[self.out_dtype]
        return self._fill(p)

    def __repr__(self):
        return 'IndexProgram(%r: %s -> %s)' % (self.eqn, self.result_dtype, self.out_dtype)


class MaskProgram(_Program):
    """settings.json `mask_eqn` (the reference's rast_algebra parameter, utils.py:447-484, dead
    there): a boolean expression over the bands of each analysis raster; an observation is kept
    only where it is true. The grammar is IndexProgram's plus comparisons, bitwise & | ^ ~ on
    integer values and booleans, and << >> by an integer literal, typed with the same legacy numpy
    promotion; the root must be boolean.

    band_numbers: the reference band number of each plane the program will run on; a band
    operand's slot is its position there, so the mask runs on the job's whole [K, nb, Q] stack."""
    _tag = 'mask_eqn'
    _mask = True

    def __init__(self, eqn, band_dtype, band_numbers, raster_count=None):
        self.eqn = eqn
        self.band_dtype = np.dtype(band_dtype)
        if self.band_dtype not in DTYPES:
            raise ValueError('mask_eqn: unsupported raster type %s' % self.band_dtype)
        bands = parse_eqn_bands(eqn)
        if not bands:
            raise ValueError('mask_eqn: %r references no band' % eqn)
        self.band_numbers = [int(b) for b in band_numbers]
        # rast_algebra's own checks (utils.py:462-465), same messages
        if raster_count is not None and max(bands) > raster_count:
            raise Exception('Band %s not present in %s' % (max(bands), '<raster>'))
        if min(bands) <= 0:
            raise Exception('Invalid band "%s" - bands must be >= 1')
        for b in bands:
            if b not in self.band_numbers:
                raise Exception('Band %s not present in %s' % (b, '<raster>'))
        self.bands = bands  # the bands the expression reads (ascending)
        if len(self.band_numbers) > _abi.LT_MAX_BANDS:
            raise ValueError('mask_eqn: more than %d bands' % _abi.LT_MAX_BANDS)
        try:
            root = self._parse(eqn)
        except (OverflowError, ZeroDivisionError) as e:
            raise ValueError('mask_eqn: %s' % e)
        if root != BOOL if isinstance(root, np.dtype) else True:
            raise ValueError('mask_eqn: %r is not a boolean expression' % eqn)
        if len(self.ops) > _abi.LT_MAX_PROG:
            raise ValueError('mask_eqn: more than %d operations' % _abi.LT_MAX_PROG)
        for _, t, _ in self.ops:
            if np.dtype(t) not in TYPE_CODES:
                raise ValueError('mask_eqn: unsupported node type %s' % t)
        self.slots = sorted({v for op, _, v in self.ops if op == _abi.LT_OP_BAND})

    def _slot(self, number):
        return self.band_numbers.index(number)

    def to_c(self):
        p = _abi.LtIndexProg()
        p.n_ops = len(self.ops)
        p.n_bands = len(self.band_numbers)
        p.band_type = DTYPES[self.band_dtype]
        p.out_type = _abi.LT_T_BOOL
        return self._fill(p)

    def evaluate(self, bands):
        """The mask in numpy, for hosts without the HIP engine: bands[s] is the plane of slot s
        (band band_numbers[s]) in band_dtype, any shape. Node by node in the node's type, as numpy
        1.x ran the expression: operands cast to the node's type, integer results wrap, `/` on
        integers floors, x // 0 = 0. Returns a boolean array."""
        def cast(x, t):
            return np.asarray(x).astype(t, casting='unsafe', copy=False)
        arith = {_abi.LT_OP_ADD: np.add, _abi.LT_OP_SUB: np.subtract, _abi.LT_OP_MUL: np.multiply,
                 _abi.LT_OP_FLOORDIV: np.floor_divide}
        other = {_abi.LT_OP_EQ: np.equal, _abi.LT_OP_NE: np.not_equal, _abi.LT_OP_LT: np.less,
                 _abi.LT_OP_LE: np.less_equal, _abi.LT_OP_GT: np.greater,
                 _abi.LT_OP_GE: np.greater_equal, _abi.LT_OP_AND: np.bitwise_and,
                 _abi.LT_OP_OR: np.bitwise_or, _abi.LT_OP_XOR: np.bitwise_xor}
        st = []
        with np.errstate(all='ignore'):
            for op, t, v in self.ops:
                t = np.dtype(t)
                if op == _abi.LT_OP_BAND:
                    st.append(np.asarray(bands[v], dtype=self.band_dtype))
                elif op in (_abi.LT_OP_CONST_I, _abi.LT_OP_CONST_F):
                    st.append(bool(v) if t == BOOL else v)
                elif op == _abi.LT_OP_NEG:
                    st.append(np.negative(cast(st.pop(), t)))
                elif op == _abi.LT_OP_NOT:
                    st.append(np.invert(cast(st.pop(), t)))
                elif op in (_abi.LT_OP_SHL, _abi.LT_OP_SHR):
                    f = np.left_shift if op == _abi.LT_OP_SHL else np.right_shift
                    st.append(f(cast(st.pop(), t), t.type(v)))
                else:
                    b = cast(st.pop(), t)
                    a = cast(st.pop(), t)
                    if op in other:
                        st.append(other[op](a, b))
                    elif op == _abi.LT_OP_DIV:
                        st.append((np.true_divide if t.kind == 'f' else np.floor_divide)
                                  (a, b, dtype=t))
                    else:
                        st.append(arith[op](a, b, dtype=t))
        if len(st) != 1 or st[0].dtype != BOOL:
            raise ValueError('mask_eqn: malformed program')
        return st[0]

    def __repr__(self):
        return 'MaskProgram(%r on bands %s)' % (self.eqn, self.band_numbers)
