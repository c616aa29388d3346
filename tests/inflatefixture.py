"""zlib streams shared by the host tests of the Deflate core (test_inflate_core_host.py, the
sanitizer program of test_inflate_core_sanitized.py) and the device chunk tests
(test_gpu_chunks.py): the device only ever sees corrupt streams made here, whose bounds behaviour
the host build of the same source (lt_inflate_core.h) has already shown. The reference is Python's
zlib throughout."""
import functools
import struct
import zlib

import numpy as np

import lzwfixture

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99,
            115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025,
             1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11,
              12, 12, 13, 13)


# ---- a small LSB-first bit reader: the blocks of an intact stream -------------------------------
class _Bits:
    def __init__(self, data):
        self.d = bytes(data) + bytes(4)
        self.pos = 0

    def peek(self, n):  # n <= 24
        k = self.pos >> 3
        return (int.from_bytes(self.d[k:k + 4], 'little') >> (self.pos & 7)) & ((1 << n) - 1)

    def get(self, n):
        x = self.peek(n)
        self.pos += n
        return x


def _code(lens):
    """{(length, code): symbol} of a canonical Huffman code."""
    out, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                out[(n, code)] = s
                code += 1
        code <<= 1
    return out


def _sym(b, table):
    w, code = b.peek(15), 0
    for n in range(1, 16):
        code = (code << 1) | (w & 1)
        w >>= 1
        if (n, code) in table:
            b.pos += n
            return table[(n, code)]
    raise ValueError('bad code')


def blocks(stream):
    """The blocks of an intact zlib stream: dicts with type (0, 1, 2), bytes (decoded), max_bits
    (longest literal/length or distance code), max_len, max_dist, overlap (a match longer than its
    distance)."""
    b = _Bits(stream)
    b.get(16)
    out, total = [], 0
    while True:
        final, typ = b.get(1), b.get(2)
        blk = dict(type=typ, bytes=0, max_bits=0, max_len=0, max_dist=0, overlap=False)
        if typ == 0:
            b.pos += -b.pos % 8
            n = b.get(16)
            assert b.get(16) == n ^ 0xffff
            b.pos += 8 * n
            blk['bytes'] = n
        else:
            if typ == 1:
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                dl = [5] * 30
            else:
                hlit, hdist, hclen = b.get(5) + 257, b.get(5) + 1, b.get(4) + 4
                cl = [0] * 19
                for k in range(hclen):
                    cl[ORDER[k]] = b.get(3)
                ct, lens = _code(cl), []
                while len(lens) < hlit + hdist:
                    s = _sym(b, ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.get(2))
                    elif s == 17:
                        lens += [0] * (3 + b.get(3))
                    else:
                        lens += [0] * (11 + b.get(7))
                ll, dl = lens[:hlit], lens[hlit:]
                blk['max_bits'] = max(ll + dl)
            lt, dt = _code(ll), _code(dl)
            while True:
                s = _sym(b, lt)
                if s < 256:
                    blk['bytes'] += 1
                elif s == 256:
                    break
                else:
                    n = LEN_BASE[s - 257] + b.get(LEN_EXTRA[s - 257])
                    d = _sym(b, dt)
                    dist = DIST_BASE[d] + b.get(DIST_EXTRA[d])
                    blk['bytes'] += n
                    blk['max_len'] = max(blk['max_len'], n)
                    blk['max_dist'] = max(blk['max_dist'], dist)
                    blk['overlap'] |= n > dist
        total += blk['bytes']
        out.append(blk)
        if final:
            return out


# ---- a small LSB-first bit writer: hand-made streams -------------------------------------------
class _Writer:
    def __init__(self):
        self.out, self.v, self.n = bytearray(), 0, 0

    def put(self, x, n):  # n bits of x, least significant first (header fields, extra bits)
        self.v |= x << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.v & 255)
            self.v >>= 8
            self.n -= 8

    def code(self, x, n):  # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            self.put((x >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):  # whole bytes, on a byte boundary
        assert self.n == 0
        self.out += data

    def bytes(self):
        self.align()
        return bytes(self.out)


def _fixed_lit(w, s):
    if s < 144:
        w.code(0x30 + s, 8)
    elif s < 256:
        w.code(0x190 + s - 144, 9)
    elif s < 280:
        w.code(s - 256, 7)
    else:
        w.code(0xc0 + s - 280, 8)


def _fixed_match(w, length, dist):
    ls = max(k for k in range(29) if LEN_BASE[k] <= length)
    if length == 258:
        ls = 28
    _fixed_lit(w, 257 + ls)
    w.put(length - LEN_BASE[ls], LEN_EXTRA[ls])
    ds = max(k for k in range(30) if DIST_BASE[k] <= dist)
    w.code(ds, 5)
    w.put(dist - DIST_BASE[ds], DIST_EXTRA[ds])


HEADER = b'\x78\x9c'


def far():
    """(stream, decoded bytes): a stored block of 32,768 random bytes, then a fixed block with one
    match of length 258 at distance 32,768 (zlib's own encoder never goes past 32,506)."""
    raw = np.random.default_rng(5).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = _Writer()
    w.put(0, 1)
    w.put(0, 2)
    w.align()
    w.put(32768, 16)
    w.put(32768 ^ 0xffff, 16)
    w.raw(raw)
    w.put(1, 1)
    w.put(1, 2)
    _fixed_match(w, 258, 32768)
    _fixed_lit(w, 256)
    full = raw + raw[:258]
    stream = HEADER + w.bytes() + struct.pack('>I', zlib.adler32(full))
    assert zlib.decompress(stream) == full
    return stream, full


def too_far_back():
    """A fixed block whose first symbol is a match: zlib's 'invalid distance too far back'."""
    w = _Writer()
    w.put(1, 1)
    w.put(1, 2)
    _fixed_match(w, 4, 1)
    _fixed_lit(w, 256)
    stream = HEADER + w.bytes() + struct.pack('>I', 1)
    try:
        zlib.decompress(stream)
    except zlib.error as e:
        assert 'too far back' in str(e)
    else:
        raise AssertionError('zlib accepts too_far_back')
    return stream


def bad_streams():
    """[(name, stream)]: hand-made streams zlib rejects."""
    good = zlib.compress(b'hello, hello, hello', 6)
    w3 = _Writer()
    w3.put(1, 1)
    w3.put(3, 2)
    st = _Writer()
    st.put(1, 1)
    st.put(0, 2)
    st.align()
    st.put(5, 16)
    st.put(5 ^ 0xfffe, 16)
    st.raw(b'abcde')
    out = [('too_far_back', too_far_back()),
           ('bad_fcheck', b'\x78\x9d' + good[2:]),
           ('fdict', b'\x78\xbb' + good[2:]),  # 0x78bb % 31 == 0, FDICT set
           ('btype3', HEADER + w3.bytes() + struct.pack('>I', 1)),
           ('len_nlen', HEADER + st.bytes() + struct.pack('>I', zlib.adler32(b'abcde'))),
           ('bad_adler', good[:-1] + bytes([good[-1] ^ 1]))]
    assert 0x78bb % 31 == 0
    for name, s in out:
        try:
            zlib.decompress(s)
        except zlib.error:
            continue
        raise AssertionError('zlib accepts %s' % name)
    return out


# ---- sources and intact streams ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sources():
    fibs = [1, 1]
    while len(fibs) < 24:
        fibs.append(fibs[-1] + fibs[-2])
    fib = np.concatenate([np.full(f, i, np.uint8) for i, f in enumerate(fibs)])
    assert len(fib) == 121392
    rng = np.random.default_rng(17)
    rng.shuffle(fib)
    a = np.random.default_rng(1).integers(0, 4096, 40000).astype(np.int16)
    pred = a.copy()
    pred[1:] = a[1:] - a[:-1]
    return tuple(lzwfixture.sources()) + (('fib', fib.tobytes()), ('int16pred', pred.tobytes()))


def _compress(raw, level, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(raw) + c.flush()


def source(name):
    return dict(sources())[name]


@functools.lru_cache(maxsize=None)
def streams():
    """((name, stream, decoded bytes), ...): every source at level 0 (stored), Z_FIXED, level 6 and
    level 9, and the extra streams. The properties the tests rely on are asserted here."""
    out = []
    for name, raw in sources():
        out.append((name + '-stored', _compress(raw, 0), raw))
        out.append((name + '-fixed', _compress(raw, 6, zlib.Z_FIXED), raw))
        out.append((name + '-l6', _compress(raw, 6), raw))
        out.append((name + '-l9', _compress(raw, 9), raw))
    fib, low = source('fib'), source('low')
    out.append(('fib-huffman', _compress(fib, 9, zlib.Z_HUFFMAN_ONLY), fib))
    c = zlib.compressobj(6)
    out.append(('low-flush', c.compress(low[:1000]) + c.flush(zlib.Z_FULL_FLUSH) +
                c.compress(low[1000:]) + c.flush(), low))
    out.append(('low-wbits9', _compress(low, 6, wbits=9), low))
    by = {n: s for n, s, _ in out}
    for name, s, raw in out:
        assert zlib.decompress(s) == raw, name
        if name.endswith('-stored'):
            assert {b['type'] for b in blocks(s)} == {0}, name
        if name.endswith('-fixed'):
            # (zlib stores what a fixed block would only lengthen: the near-random sources)
            stored = name.split('-')[0] in ('rand8400', 'rand70000')
            assert {b['type'] for b in blocks(s)} == ({0} if stored else {1}), name
    assert len(blocks(by['rand70000-stored'])) == 2
    assert [b['type'] for b in blocks(by['low-l6'])] == [2]
    fl = blocks(by['low-flush'])
    assert [(b['type'], b['bytes'] > 0) for b in fl] == [(2, True), (0, False), (2, True)]
    assert by['low-wbits9'][0] >> 4 < 7
    for name, dist in (('zeros-l6', 1), ('period3-l6', 3)):
        bl = blocks(by[name])
        assert any(b['overlap'] and b['max_len'] == 258 and b['max_dist'] == dist for b in bl), name
    fh = blocks(by['fib-huffman'])
    assert len(fh) == 8 and {b['type'] for b in fh} == {2} and max(b['max_bits'] for b in fh) == 15
    ip = blocks(by['int16pred-l6'])
    assert len(ip) == 5 and {b['type'] for b in ip} == {2}
    assert 30000 < max(b['max_dist'] for b in ip) <= 32768
    assert max(b['max_bits'] for b in ip) == 12
    return tuple(out)


def stream(name):
    return {n: (s, raw) for n, s, raw in streams()}[name]


@functools.lru_cache(maxsize=None)
def corrupt_streams(n=2000, seed=11):
    """n seeded (stream, decoded size of the intact stream) pairs: a level-6, fixed or stored
    encode of a short source with 1 to 3 flipped bits. corrupt_bases() names the intact ones."""
    rng = np.random.default_rng(seed)
    base = corrupt_bases()
    out = []
    for k in range(n):
        enc, size = base[k % len(base)]
        b = bytearray(enc)
        for _ in range(int(rng.integers(1, 4))):
            bit = int(rng.integers(0, len(b) * 8))
            b[bit >> 3] ^= 1 << (bit & 7)
        out.append((bytes(b), size))
    return tuple(out)


def corrupt_bases():
    short = [(n, raw) for n, raw in sources()
             if n not in ('empty', 'rand70000', 'fib', 'int16pred')]
    return [(stream('%s-%s' % (n, kind))[0], len(raw)) for n, raw in short
            for kind in ('l6', 'fixed', 'stored')]


def ref(stream_, cap):
    """The reference outcome of decoding `stream_` into `cap` >= 1 bytes: the bytes, or None for
    an error. zlib.decompress when it succeeds (its first cap bytes); else a decompressobj offered
    room for cap + 1 bytes: cap bytes when it fills them (the stream is over-long and its fault
    lies behind them), an error otherwise."""
    try:
        return zlib.decompress(stream_)[:cap]
    except zlib.error:
        pass
    try:
        got = zlib.decompressobj().decompress(stream_, cap + 1)
    except zlib.error:
        return None
    return got[:cap] if len(got) == cap + 1 else None
