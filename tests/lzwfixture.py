"""LZW strips shared by the host tests of the decoder core (test_lzw_core_host.py) and the device
decode tests (test_gpu_decode.py): the device only ever sees corrupt strips made here, whose bounds
behaviour the host build of the same source (lt_lzw_core.h) has already shown."""
import numpy as np

from land_trendr_amd import tiffcodec

CLEAR, EOI, FIRST = 256, 257, 258


def read_codes(stream):
    """The (code, width) pairs of a TIFF LZW stream: MSB first, 9..12 bits, early change."""
    bits = ''.join('{:08b}'.format(b) for b in bytes(stream))
    out, pos, nbits, free, first = [], 0, 9, FIRST, True
    while pos + nbits <= len(bits):
        code = int(bits[pos:pos + nbits], 2)
        out.append((code, nbits))
        pos += nbits
        if code == EOI:
            break
        if code == CLEAR:
            nbits, free, first = 9, FIRST, True
            continue
        if not first and free < 4096:
            free += 1
        first = False
        if free >= (1 << nbits) - 1 and nbits < 12:
            nbits += 1
    return out


def pack_codes(codes, nbits=9):
    """Codes of one fixed width, MSB first, zero-padded to a byte."""
    bits = ''.join('{:0{w}b}'.format(c, w=nbits) for c in codes)
    bits += '0' * (-len(bits) % 8)
    return bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8))


def bad_code_strip():
    """Clear, two literals, then code 300 while the first free code is 259: LT_IO_ERR_DATA."""
    return pack_codes([CLEAR, 65, 66, 300, 67, EOI])


def sources(seed=7):
    """Raw inputs of a few kinds, (name, bytes): what the round-trip cases and the corrupt corpus
    are made from."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 4, 3000, dtype=np.uint8)
    return [('empty', b''), ('one', b'\x2a'), ('zeros', bytes(5000)), ('const', b'\x07' * 4097),
            ('ramp', bytes(range(256)) * 12), ('period3', b'\x01\x02\x03' * 1500),
            ('low', low.tobytes()),
            ('rand8400', rng.integers(0, 256, 8400, dtype=np.uint8).tobytes()),
            ('rand70000', rng.integers(0, 256, 70000, dtype=np.uint8).tobytes())]


def corrupt_streams(n=2000, seed=11):
    """n seeded (stream, decoded size of the intact stream) pairs: an encoded source with 1 to 3
    flipped bits."""
    rng = np.random.default_rng(seed)
    base = [(tiffcodec.lzw_encode(raw), len(raw)) for name, raw in sources()
            if name not in ('empty', 'rand70000')]
    base.append((tiffcodec.lzw_encode(rng.integers(0, 256, 600, dtype=np.uint8).tobytes()), 600))
    out = []
    for k in range(n):
        enc, size = base[k % len(base)]
        b = bytearray(enc)
        for _ in range(int(rng.integers(1, 4))):
            bit = int(rng.integers(0, len(b) * 8))
            b[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append((bytes(b), size))
    return out
