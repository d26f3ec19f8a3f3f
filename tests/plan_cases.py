"""Byte spans for the device planner's tests (test_plan_split_cpu / _gpu /
_sanitizers): a record generator on top of bamgen.encode_record that makes
records of an exact size (trailing aux bytes, so block_size exceeds the need),
the boundary, break and decoy cases scaled to a chunk size C, byte-mutated
spans, a plain chain walk, and the corpus file tests/native/plan_driver.c reads.

A decoy is built from the guess rule as csrc/ss_plan_core.h has it: a head
written into a record's quality bytes at a chunk start, plausible field by
field, whose block_size lands on a true record start -- so the chunk's guess
is wrong and the stitch has to repair it.
"""
import os
import random
import struct
import sys
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bamgen  # noqa: E402

N_REF = 4
MIN_REC = 44                  # block_size + 32 + "r\0" + one CIGAR word + one base + one quality
A_LSEQ = 200
A_TOTAL = 36 + 2 + 4 + A_LSEQ // 2 + A_LSEQ      # 342: its last 200 bytes are qualities
TAIL = 80                     # bytes of an A record that lie past the chunk boundary it straddles


@dataclass
class Span:
    name: str
    data: bytes
    chunk: int                # the chunk size at which the case bites
    n_ref: int = N_REF
    min_repairs: int = 0      # decoys: the repairs the case forces at `chunk`


def walk(b):
    """The plain chain walk: (offsets, end_at, bad_block)."""
    at, out = 0, []
    while len(b) - at >= 4:
        block, = struct.unpack_from("<i", b, at)
        if block < 32:
            return out, at, True
        if len(b) - at - 4 < block:
            break
        out.append(at)
        at += 4 + block
    return out, at, False


class Gen:
    """Records of one contig in position order."""

    def __init__(self, seed=5):
        self.rng = random.Random(seed)
        self.pos = 10
        self.tid = 0

    def sized(self, total, lseq=None, mapq=60, flag=0):
        """A record of exactly `total` bytes (block_size field included)."""
        assert total >= MIN_REC, total
        fixed = 36 + 2 + 4
        if lseq is None:
            lseq = min(30, ((total - fixed) * 2) // 3)
            while fixed + (lseq + 1) // 2 + lseq > total:
                lseq -= 1
        lseq = max(1, lseq)
        aux = total - (fixed + (lseq + 1) // 2 + lseq)
        assert aux >= 0, (total, lseq)
        seq = "".join(self.rng.choice("ACGT") for _ in range(lseq))
        qual = [self.rng.randrange(2, 60) for _ in range(lseq)]
        raw = bytearray(bamgen.encode_record(self.tid, self.pos, "r", mapq, flag, [("M", lseq)], seq, qual))
        assert len(raw) == total - aux, (len(raw), total, aux)
        raw += bytes(self.rng.randrange(256) for _ in range(aux))        # aux bytes: never parsed
        struct.pack_into("<i", raw, 0, total - 4)
        self.pos += self.rng.randrange(1, 9)
        return bytes(raw)

    def fill(self, n):
        """Records that take exactly n bytes."""
        out = []
        while n > 400:
            out.append(self.sized(200))
            n -= 200
        if n:
            out.append(self.sized(n))
        return b"".join(out)

    def some(self, k):
        return b"".join(self.sized(self.rng.randrange(MIN_REC, 160)) for _ in range(k))


def boundary_cases(C):
    """Record starts around a chunk boundary, long records, short spans, cut and bad records."""
    out = []
    for d in range(-3, 4):
        g = Gen(20 + d)
        out.append(Span(f"start_at_boundary{d:+d}", g.fill(C + d) + g.some(6) + g.fill(C) + g.some(3), C))
    g = Gen(30)
    out.append(Span("ends_at_boundary", g.fill(C) + g.fill(C) + g.some(4), C))
    g = Gen(31)
    out.append(Span("longer_than_one_chunk", g.some(2) + g.sized(C + C // 2 + 7, lseq=30) + g.some(5) + g.fill(C), C))
    g = Gen(32)
    out.append(Span("longer_than_three_chunks", g.some(3) + g.sized(3 * C + C // 2 + 5, lseq=30) + g.some(5), C))
    g = Gen(33)
    one = g.sized(60)
    for n in (0, 3, 35, 36):
        out.append(Span(f"len_{n}", one[:n], C))
    g = Gen(34)
    whole = g.fill(C + 90) + g.some(2)
    last = g.sized(120)
    out.append(Span("cut_in_head", whole + last[:20], C))
    out.append(Span("cut_in_body", whole + last[:-5], C))
    for name, block in (("block_31", 31), ("block_negative", -5)):
        g = Gen(35)
        bad = bytearray(g.sized(100))
        struct.pack_into("<i", bad, 0, block)
        out.append(Span(name, g.fill(C + 50) + g.some(3) + bytes(bad) + g.some(4) + g.fill(C), C))
    return out


def _decoy_head(block):
    """36 + 8 bytes that pass every test of ssp_plausible, with the given block_size."""
    h = struct.pack("<iiiBBHHHiiii", block, 0, 5, 2, 60, 4681, 1, 0, 1, -1, -1, 0) + b"d\0" + struct.pack("<I", 1 << 4)
    return h + b"\x10\x20"    # one base, one quality


def decoy_stream(C, n_chunks, decoys, far=False, seed=40):
    """n_chunks chunks in which a long record (A) straddles every boundary with its
    qualities; in each chunk of `decoys` a head at the chunk start, inside A's
    qualities, points at a true record start: the first one after A, or with
    `far` the first one at least two chunks later."""
    assert C >= 512
    g = Gen(seed)
    out = bytearray()
    for k in range(n_chunks - 1):
        out += g.fill((k + 1) * C + TAIL - A_TOTAL - len(out))
        out += g.sized(A_TOTAL, lseq=A_LSEQ)
    out += g.some(4)
    starts, _, _ = walk(bytes(out))
    for k in decoys:
        at = k * C
        want = at + 2 * C if far else at + TAIL
        target = min(s for s in starts if s >= want)
        head = _decoy_head(target - at - 4)
        assert len(head) <= TAIL and target - at - 4 >= 40
        out[at:at + len(head)] = head
    assert walk(bytes(out))[0] == starts                    # the decoys changed qualities only
    return bytes(out)


def decoy_cases(C):
    return [Span("decoy_one", decoy_stream(C, 5, [2]), C, min_repairs=1),
            Span("decoy_rejoins_two_chunks_later", decoy_stream(C, 8, [2], far=True, seed=41), C, min_repairs=1),
            Span("decoy_every_chunk", decoy_stream(C, 16, range(1, 16), seed=42), C, min_repairs=15)]


def cases(C):
    return boundary_cases(C) + (decoy_cases(C) if C >= 512 else [])


def _raw(tid, pos, cigar, mapq=60, flag=0, n_cigar=None):
    lq = sum(n for op, n in cigar if op in "MIS=X")
    b = bytearray(bamgen.encode_record(tid, max(pos, 0), "q", mapq, flag, cigar, "A" * lq, [30] * lq))
    struct.pack_into("<i", b, 8, pos)
    if n_cigar is not None:
        struct.pack_into("<H", b, 16, n_cigar)                # passes the block: name + CIGAR > block_size
    return bytes(b)


def quirk_cases():
    """Hand-made records for the load rules' quirks (the issue's list)."""
    M = lambda n: [("M", n)]                                  # noqa: E731
    out = []
    # the first record of contig 1 ends at or before contig 0's W: dropped, though its `from` would be its pos
    out.append(Span("contig_change_end_below_old_w",
                    b"".join([_raw(0, 100, M(50)), _raw(0, 500, M(50)), _raw(1, 10, M(20)), _raw(1, 20, M(50)),
                              _raw(1, 5, M(10)), _raw(2, 700, M(30)), _raw(2, 0, M(800))]), 64))
    out.append(Span("pos_minus_one",
                    b"".join([_raw(0, -1, M(30)), _raw(0, -1, M(1)), _raw(0, 3, M(20)), _raw(1, -1, M(5)),
                              _raw(1, 0, M(5))]), 64))
    out.append(Span("lower_contig_after_higher",
                    b"".join([_raw(1, 10, M(30)), _raw(1, 20, M(30)), _raw(0, 30, M(30)), _raw(1, 40, M(30))]), 64))
    out.append(Span("filtered_lower_contig_is_no_error",
                    b"".join([_raw(1, 10, M(30)), _raw(0, 20, M(30), flag=0x400), _raw(0, 25, M(30), flag=0x200),
                              _raw(1, 40, M(30))]), 64))
    out.append(Span("cigar_passes_block_filtered_then_kept",
                    b"".join([_raw(0, 10, M(30)), _raw(0, 12, M(30), flag=0x400, n_cigar=500), _raw(0, 14, M(30)),
                              _raw(0, 16, M(30), n_cigar=500), _raw(0, 18, M(30))]), 64))
    out.append(Span("unsorted_and_contained",
                    b"".join([_raw(0, 300, M(50)), _raw(0, 100, M(300)), _raw(0, 120, M(10)), _raw(0, 90, M(500)),
                              _raw(0, 400, [("M", 10), ("D", 300), ("N", 50), ("I", 4), ("M", 5)])]), 64))
    return out


def mutated_cases(count, seed=13):
    """Small spans with a few bytes changed: any outcome, no invalid access."""
    rng = random.Random(seed)
    base = [s for s in boundary_cases(64) + cases(512) if len(s.data) > 40]
    out = []
    for i in range(count):
        src = base[i % len(base)]
        b = bytearray(src.data)
        starts = walk(src.data)[0] or [0]
        for _ in range(rng.randrange(1, 4)):
            at = starts[rng.randrange(len(starts))] + rng.randrange(0, 44) if rng.random() < 0.7 else rng.randrange(len(b))
            if at < len(b):
                b[at] = rng.choice([0, 1, 0x1F, 0x20, 0x7F, 0x80, 0xFF, rng.randrange(256)])
        out.append(Span(f"mut{i}", bytes(b), src.chunk, rng.choice([0, N_REF])))
    return out


def write_corpus(path, spans, headers):
    """The file tests/native/plan_driver.c reads (little-endian): u32 n_spans, per
    span u32 chunk, i32 n_ref, u64 len + bytes; then u32 n_headers, per header
    (whole uncompressed BAM bytes) u64 len + bytes, i32 n_ref, u64 records_at."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(spans)))
        for s in spans:
            f.write(struct.pack("<IiQ", s.chunk, s.n_ref, len(s.data)))
            f.write(s.data)
        f.write(struct.pack("<I", len(headers)))
        for data, n_ref, at in headers:
            f.write(struct.pack("<Q", len(data)))
            f.write(data)
            f.write(struct.pack("<iQ", n_ref, at))
