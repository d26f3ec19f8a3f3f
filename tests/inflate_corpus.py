"""Member corpus for the BGZF inflation tests (helper, no tests).

A member is what ss_inflate_members_* takes: raw DEFLATE data followed by the
8-byte gzip trailer (CRC32, ISIZE).  Valid members come from Python's zlib,
plus hand-written fixed-Huffman streams for what zlib never emits (its longest
distance is 32 506); malformed members are paired with the status they must
get.  The helper asserts the block types it promises by reading the streams'
block headers itself.
"""
import os
import random
import struct
import sys
import zlib
from collections import namedtuple
from functools import lru_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_STREAM, E_SIZE, E_CRC = 0, 1, 2, 3

# comp: DEFLATE data + trailer; olen: the output span; data: the expected bytes (valid members)
Member = namedtuple("Member", "name comp olen status data")


# ---------------------------------------------------------------- bit level
class Bits:
    """LSB-first bit writer; Huffman codes go in most significant bit first."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        for i in range(n - 1, -1, -1):
            self.bits(c >> i & 1, 1)

    def done(self) -> bytes:
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


class Fixed(Bits):
    """One fixed-Huffman block (BTYPE 1), RFC 1951 3.2.6."""

    def __init__(self, final=1):
        super().__init__()
        self.bits(final, 1)
        self.bits(1, 2)

    def sym(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def lits(self, data):
        for b in data:
            self.sym(b)

    def dist_sym(self, s, extra=0):
        self.code(s, 5)
        if s < 30:
            self.bits(extra, DIST_EXTRA[s])

    def match(self, length, dist):
        ls = max(i for i in range(29) if LEN_BASE[i] <= length and (i == 28 or length < 258))
        self.sym(257 + ls)
        self.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.dist_sym(ds, dist - DIST_BASE[ds])

    def end(self) -> bytes:
        self.sym(256)
        return self.done()


def trailer(data: bytes) -> bytes:
    return struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


# ---------------------------------------------------------------- block headers
class _Reader:
    def __init__(self, data):
        self.d, self.p = data, 0

    def bits(self, n):
        v = 0
        for i in range(n):
            v |= (self.d[self.p >> 3] >> (self.p & 7) & 1) << i
            self.p += 1
        return v


ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def first_block(stream: bytes):
    """(BFINAL, BTYPE, longest literal/length code) of the first block (the
    code length only for a dynamic block)."""
    r = _Reader(stream)
    final, btype = r.bits(1), r.bits(2)
    if btype != 2:
        return final, btype, 0
    nlen, ndist, ncode = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
    cl = [0] * 19
    for i in range(ncode):
        cl[ORDER[i]] = r.bits(3)
    # canonical codes of the code-length code, read bit by bit
    codes, code = {}, 0
    for ln in range(1, 8):
        for s in range(19):
            if cl[s] == ln:
                codes[(ln, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < nlen + ndist:
        c, ln = 0, 0
        while (ln, c) not in codes:
            c, ln = c << 1 | r.bits(1), ln + 1
            assert ln <= 7
        s = codes[(ln, c)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + r.bits(2))
        elif s == 17:
            lens += [0] * (3 + r.bits(3))
        else:
            lens += [0] * (11 + r.bits(7))
    return final, btype, max(lens[:nlen])


def bgzf_members(path_or_bytes):
    """(DEFLATE data + trailer) of every member of a BGZF file, cut with Python only."""
    d = path_or_bytes if isinstance(path_or_bytes, bytes) else open(path_or_bytes, "rb").read()
    out, at = [], 0
    while at < len(d):
        assert d[at:at + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", d, at + 10)[0]
        extra, bsize, p = d[at + 12:at + 12 + xlen], None, 0
        while p + 4 <= xlen:
            sl = struct.unpack_from("<H", extra, p + 2)[0]
            if extra[p:p + 2] == b"BC":
                bsize = struct.unpack_from("<H", extra, p + 4)[0]
            p += 4 + sl
        out.append(d[at + 12 + xlen:at + bsize + 1])
        at += bsize + 1
    return out


# ---------------------------------------------------------------- the corpus
def _valid(name, stream, data=None):
    if data is None:
        data = zlib.decompress(stream, -15)
    else:
        assert zlib.decompress(stream, -15) == data, name
    return Member(name, stream + trailer(data), len(data), OK, data)


def _fib_text(rng, n_sym):
    a, b, data = 1, 1, bytearray()
    for s in range(n_sym):
        data += bytes([65 + s]) * a
        a, b = b, a + b
    data = list(data)
    rng.shuffle(data)
    return bytes(data)


def far_match_stream(rng):
    """Length 258 at distance 32 768, length 3 at distance 1, and matches up to
    a last one that ends exactly on byte 65 536."""
    head = bytes(rng.randrange(256) for _ in range(32768))
    f = Fixed()
    f.lits(head)
    data = bytearray(head)

    def m(length, dist):
        f.match(length, dist)
        for _ in range(length):
            data.append(data[-dist])

    m(258, 32768)
    m(3, 1)
    while len(data) + 258 <= 65536 - 257:
        m(258, 32768)
    rest = 65536 - len(data)
    while rest > 258:
        m(3, 32768)
        rest -= 3
    m(rest, 32768)
    assert len(data) == 65536
    return f.end(), bytes(data)


@lru_cache(maxsize=None)
def valid_members():
    rng = random.Random(20240611)
    out = []
    empty = deflate(b"")
    assert empty == b"\x03\x00"                     # the BGZF EOF marker's fixed block
    out.append(_valid("empty", empty, b""))
    s = deflate(b"ACGT" * 50, 6, zlib.Z_FIXED)
    assert first_block(s)[1] == 1
    out.append(_valid("fixed_acgt", s))
    rnd = bytes(rng.randrange(256) for _ in range(65280))
    for lvl in (0, 6):
        s = deflate(rnd, lvl)
        assert first_block(s)[:2] == (0, 0), lvl    # several stored blocks
        out.append(_valid(f"stored_l{lvl}", s, rnd))
    acgtn = bytes(rng.choice(b"ACGTN") for _ in range(65280))
    s = deflate(acgtn)
    assert first_block(s)[1] == 2
    out.append(_valid("dynamic_acgtn", s, acgtn))
    s = deflate(bytes(65536))
    assert first_block(s)[1] == 2
    out.append(_valid("zeros_64k", s))
    n_sym = 22
    while True:
        fib = _fib_text(rng, n_sym)
        s = deflate(fib, 6, zlib.Z_HUFFMAN_ONLY)
        if first_block(s)[1] == 2 and first_block(s)[2] >= 13:
            break
        n_sym += 1
        assert n_sym < 24, "no long code lengths"   # 24 symbols would pass 64 KiB
    out.append(_valid("fib_long_codes", s, fib))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    a, b = acgtn[:20001], acgtn[20001:45000]
    s = c.compress(a) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(b) + c.flush()
    assert b"\x00\x00\xff\xff" in s
    out.append(_valid("full_flush", s, a + b))
    out.append(_valid("all_bytes", deflate(bytes(range(256)))))
    s, data = far_match_stream(rng)
    out.append(_valid("far_matches", s, data))
    for f in ("t-small.bam", "n-small.bam"):
        for i, m in enumerate(bgzf_members(os.path.join(ROOT, "tests", "golden", "integration", f))):
            out.append(_valid(f"{f}:{i}", m[:-8]))
    return tuple(out)


def bam_members(tmpdir):
    """Members of one bamgen.make_pair BAM (needs a scratch directory)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bamgen
    bamgen.make_pair(str(tmpdir), seed=11, lengths=(2500, 1200), depth_t=40, depth_n=10)
    return tuple(_valid(f"bamgen:{i}", m[:-8]) for i, m in enumerate(bgzf_members(os.path.join(str(tmpdir),
                                                                                               "tumor.bam"))))


@lru_cache(maxsize=None)
def malformed_members():
    good = next(m for m in valid_members() if m.name == "dynamic_acgtn")
    stream, data, tr = good.comp[:-8], good.data, good.comp[-8:]
    out = []

    def bad(name, stream, olen, status, tr=None):
        out.append(Member(name, stream + (tr if tr is not None else struct.pack("<II", 0, olen)), olen, status, None))

    bad("cut_1_byte", stream[:1], len(data), E_STREAM, tr)
    bad("cut_mid", stream[:len(stream) // 2], len(data), E_STREAM, tr)
    crc, isize = struct.unpack("<II", tr)
    bad("crc_bit", stream, len(data), E_CRC, struct.pack("<II", crc ^ 0x00010000, isize))
    bad("isize_plus_1", stream, len(data), E_SIZE, struct.pack("<II", crc, isize + 1))
    bad("isize_plus_1_span", stream, len(data) + 1, E_SIZE, struct.pack("<II", crc, isize + 1))
    bad("isize_minus_1", stream, len(data), E_SIZE, struct.pack("<II", crc, isize - 1))
    f = Fixed()
    f.lits(b"abc")
    f.match(3, 5)                                   # distance 5 at output position 3
    bad("dist_before_start", f.end(), 6, E_STREAM)
    f = Fixed()
    f.lits(b"A")
    f.match(258, 1)                                 # runs past a 10-byte span
    bad("match_past_span", f.end(), 10, E_STREAM)
    f = Fixed()
    f.lits(bytes(range(70)))                        # more literals than the span, over two runs of 64
    bad("literals_past_span", f.end(), 66, E_STREAM)
    f = Fixed()
    f.lits(b"ab")
    f.sym(286)
    bad("symbol_286", f.end(), 2, E_STREAM)
    f = Fixed()
    f.lits(b"ab")
    f.sym(257)
    f.dist_sym(30)
    bad("dist_symbol_30", f.end(), 5, E_STREAM)
    b = Bits()                                      # dynamic: four code-length codes of length 1
    b.bits(1, 1), b.bits(2, 2), b.bits(0, 5), b.bits(0, 5), b.bits(0, 4)
    for _ in range(4):
        b.bits(1, 3)
    bad("oversubscribed", b.done() + bytes(8), 4, E_STREAM)
    b = Bits()                                      # dynamic: the code-length code has one code only
    b.bits(1, 1), b.bits(2, 2), b.bits(0, 5), b.bits(0, 5), b.bits(0, 4)
    b.bits(0, 3), b.bits(0, 3), b.bits(0, 3), b.bits(1, 3)
    bad("incomplete_code_lengths", b.done() + bytes(40), 4, E_STREAM)
    bad("stored_nlen", b"\x01\x05\x00\xfa\xfe" + b"hello", 5, E_STREAM)
    bad("stored_cut", b"\x01\x05\x00\xfa\xff" + b"hel", 5, E_STREAM)
    bad("btype_3", b"\x07\x00\x00", 0, E_STREAM)
    bad("no_trailer", b"", 0, E_STREAM, b"\x03\x00")   # shorter than a trailer
    return tuple(out)


ANY = 0xFFFFFFFF


def mutated_members(count=400):
    """Small valid members with a few bytes changed, for the sanitizer driver:
    whatever they decode to, nothing outside their spans may be touched."""
    rng = random.Random(77)
    base = [m for m in valid_members() if len(m.comp) < 600] + \
           [_valid("mut_text", deflate(bytes(rng.choice(b"ACGTN\n") for _ in range(3000)))),
            _valid("mut_runs", deflate(b"".join(bytes([rng.randrange(4)]) * rng.randrange(1, 40) for _ in range(300))))]
    out = []
    for i in range(count):
        m = base[i % len(base)]
        c = bytearray(m.comp)
        for _ in range(rng.randrange(1, 4)):
            c[rng.randrange(len(c) - 8)] = rng.randrange(256) if rng.random() < 0.5 else c[rng.randrange(len(c))]
        out.append(Member(f"mut:{i}", bytes(c), m.olen, ANY, None))
    return out


def pack(members):
    """(comp bytes, comp_off, out_off) as the inflate calls take them."""
    import numpy as np
    coff, ooff = [0], [0]
    for m in members:
        coff.append(coff[-1] + len(m.comp))
        ooff.append(ooff[-1] + m.olen)
    return (np.frombuffer(b"".join(m.comp for m in members), np.uint8), np.asarray(coff, np.uint64),
            np.asarray(ooff, np.uint64))


def write_file(path, members):
    """For tests/native/inflate_driver.c: u32 count, then per member u32 clen,
    u32 olen, u32 status, u32 crc of the expected bytes, and the clen bytes."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(members)))
        for m in members:
            want = zlib.crc32(m.data if m.data is not None else bytes(m.olen)) & 0xFFFFFFFF
            f.write(struct.pack("<IIII", len(m.comp), m.olen, m.status, want))
            f.write(m.comp)
