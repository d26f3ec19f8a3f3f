"""Helpers of the record-pileup tests (test_pileup_cpu / _gpu / _sanitizers):

- a brute-force model of the pileup rules (cli/column_pileup.h) in plain
  Python: for each position, for each record in load order, walk the CIGAR;
- record builders on top of bamgen.encode_record and the test cases built from
  them: one case per branch of the column builder, and the rejection cases;
- the corpus file tests/native/pileup_driver.c reads;
- a parser for the CLI's SS_DUMP_PILEUP lines and a BAM header skipper.
"""
import os
import random
import struct
import sys
from dataclasses import dataclass, field

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bamgen  # noqa: E402

SS_OK, SS_E_INVAL, SS_E_CAPACITY = 0, -1, -5
ANY = 99                      # corpus: any return code (mutated records)


@dataclass
class Rec:
    pos: int
    cigar: list               # [(op_char, len)]
    mapq: int = 60
    flag: int = 0
    seq: str = ""
    qual: list = field(default_factory=list)
    name: str = "r"
    from_: int = None         # default: pos
    raw: bytes = b""          # the record as it lies in the file
    bad: bool = False         # must be rejected: contributes nothing

    def __post_init__(self):
        if self.from_ is None:
            self.from_ = self.pos


def parse_cigar(s):
    out, n = [], ""
    for ch in s:
        if ch.isdigit():
            n += ch
        else:
            out.append((ch, int(n)))
            n = ""
    return out


_rng = random.Random(7)


def rec(pos, cigar, mapq=60, flag=0, name="r", from_=None, seq=None, qual=None, extra_seq=0, tid=0):
    """A record whose l_seq is the CIGAR's query length (M I S = X) + extra_seq."""
    cg = parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    lq = sum(n for op, n in cg if op in "MIS=X") + extra_seq
    if seq is None:
        seq = "".join(_rng.choice("ACGTN") for _ in range(lq))
    if qual is None:
        qual = [_rng.randrange(0, 94) for _ in range(len(seq))]
    r = Rec(pos, cg, mapq, flag, seq, list(qual), name, from_)
    if pos < 1 << 29:
        r.raw = bamgen.encode_record(tid, pos, name, mapq, flag, cg, seq, qual)
    else:                     # past the BAM bin scheme's reach: the bin is not read here, only pos matters
        b = bytearray(bamgen.encode_record(tid, 0, name, mapq, flag, cg, seq, qual))
        struct.pack_into("<i", b, 8, pos)
        r.raw = bytes(b)
    return r


# ---------------------------------------------------------------- the model
def lookup(r: Rec, p: int):
    """('base', q) | ('del', None) | None for record r at position p."""
    if r.bad or p < r.from_:
        return None
    x, y = r.pos, 0
    for op, n in r.cigar:
        if op == "M":
            if x <= p < x + n:
                return ("base", y + p - x)
            x += n
            y += n
        elif op == "D":
            if x <= p < x + n:
                return ("del", None)
            x += n
        elif op == "N":
            x += n
        elif op in "IS":
            y += n
        # H, P, = and X move neither coordinate
    return None


def pack(r: Rec, q: int) -> int:
    nt16 = bamgen.SEQ_CODES.index(r.seq[q])
    return (r.mapq & 0xFF) | (r.qual[q] & 0xFF) << 8 | nt16 << 16 | (1 << 20 if r.flag & 16 else 0)


def model_region(tumor, normal, ref, lo, hi):
    """(pos, refchar, raw_t, raw_n, off_t, off_n, reads_t, reads_n) as numpy arrays."""
    pos, refc, raw_t, raw_n, off_t, off_n, reads_t, reads_n = [], [], [], [], [0], [0], [], []
    for p in range(lo, hi):
        cols = []
        for recs in (tumor, normal):
            raw, pk = 0, []
            for r in recs:
                e = lookup(r, p)
                if e is None:
                    continue
                raw += 1
                if e[0] == "base":
                    pk.append(pack(r, e[1]))
            cols.append((raw, pk))
        if cols[0][0] > 0 and cols[1][0] > 0:
            pos.append(p)
            refc.append(ref[p] if ref is not None and p < len(ref) else ord("N"))
            raw_t.append(cols[0][0])
            raw_n.append(cols[1][0])
            reads_t += cols[0][1]
            reads_n += cols[1][1]
            off_t.append(len(reads_t))
            off_n.append(len(reads_n))
    a = np.asarray
    return (a(pos, np.int32), a(refc, np.uint8), a(raw_t, np.uint32), a(raw_n, np.uint32), a(off_t, np.uint32),
            a(off_n, np.uint32), a(reads_t, np.uint32), a(reads_n, np.uint32))


def region_arrays(reg):
    """The same tuple from a PileupRegion."""
    b = reg.batch
    return (reg.pos, b.ref, reg.raw_t, reg.raw_n, b.off_tumor, b.off_normal, b.reads_tumor, b.reads_normal)


def same(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and (x == y).all() for x, y in zip(a, b))


# ---------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    tumor: list
    normal: list
    lo: int
    hi: int
    ref: bytes = None
    rc: int = SS_OK            # the return code the region calls must give
    whole_call: bool = False   # rc rejects the call as a whole: no columns
    samples: tuple = None      # ((bytes, rec_off, from), (..)) when not simply the records' bytes

    def sample(self, k):
        if self.samples is not None:
            return self.samples[k]
        return sample_of(self.normal if k else self.tumor)


def sample_of(recs):
    off, at = [], 0
    for r in recs:
        off.append(at)
        at += len(r.raw)
    return (np.frombuffer(b"".join(r.raw for r in recs), np.uint8), np.asarray(off, np.uint64),
            np.asarray([r.from_ for r in recs], np.int32))


def _cover(lo, hi, step=30, length=50, **kw):
    return [rec(p, f"{length}M", name=f"c{p}", **kw) for p in range(lo, hi, step)]


REF = bytes(_rng.choice(b"ACGTacgtNn") for _ in range(1200))


def branch_cases():
    """One case per branch of the column builder (the issue's list, in its order)."""
    c = []
    c.append(Case("single_m", [rec(10, "40M"), rec(15, "30M", flag=16), rec(30, "50M", mapq=0)],
                  [rec(5, "60M"), rec(40, "20M", flag=16, mapq=255)], 0, 120, REF))
    mixed = "3H4S10M2I5M3D4M7N6M2=3X1P5M4S2H"
    c.append(Case("every_op", [rec(20, mixed), rec(22, "6M1D1N2I3M", flag=16), rec(25, "2S3=8M")],
                  [rec(18, "1P12M4N2D9M"), rec(30, mixed, name="abc")], 0, 100, REF))
    c.append(Case("from_gt_beg", [rec(10, "40M", from_=25), rec(12, "5M4D20M", from_=25), rec(26, "10M")],
                  [rec(0, "80M"), rec(8, "10M3N20M", from_=30)], 0, 100, REF))
    c.append(Case("tile_edge", [rec(250, "20M")], [rec(250, "20M", flag=16), rec(255, "1M"), rec(256, "1M")],
                  0, 300, REF))
    c.append(Case("three_tiles_n", [rec(200, "10M600N10M"), rec(500, "12M")], _cover(180, 860), 0, 1000, REF))
    c.append(Case("cut_lo_hi", _cover(0, 400, 17, 45), _cover(3, 400, 23, 61, flag=16), 130, 289, REF))
    c.append(Case("deletion_only", [rec(50, "5M3D5M"), rec(53, "2D1M", name="dd")], [rec(40, "40M")], 0, 100, REF))
    c.append(Case("skip_only", [rec(50, "5M10N5M")], [rec(40, "40M")], 0, 100, REF))
    c.append(Case("one_sample_only", [rec(10, "20M"), rec(60, "20M")], [rec(25, "20M"), rec(70, "30M")], 0, 120, REF))
    c.append(Case("depth_65_300",
                  sorted([rec(100 - i % 9, "12M", name=f"t{i}", flag=16 * (i & 1)) for i in range(65)],
                         key=lambda r: r.pos),
                  sorted([rec(104 - i % 5, "9M2D3M", name=f"n{i}") for i in range(300)], key=lambda r: r.pos),
                  80, 130, REF))
    c.append(Case("empty_sample", [rec(10, "30M"), rec(20, "30M")], [], 0, 80, REF))
    c.append(Case("odd_l_seq", [rec(10, "7M"), rec(11, "3S9M1I4M")], [rec(9, "13M"), rec(12, "1M")], 0, 40, REF))
    c.append(Case("qual_255_base_eq", [rec(10, "6M", seq="=A=CN=", qual=[255, 0, 255, 93, 1, 254])],
                  [rec(10, "6M", seq="======", qual=[255] * 6, flag=16)], 0, 30, REF))
    # names of 1..7 characters and odd sequence lengths: every following CIGAR misaligned
    mis_t = [rec(10 + i, f"{5 + 2 * i}M1D{4 + i}M", name="n" * (1 + i % 7)) for i in range(9)]
    mis_n = [rec(8 + 2 * i, f"1S{6 + i}M2N3M", name="m" * (1 + (i + 2) % 7)) for i in range(9)]
    c.append(Case("misaligned_cigars", mis_t, mis_n, 0, 80, REF))
    reads = ([rec(10, "40M"), rec(30, "30M2D10M")], [rec(5, "70M")])
    c.append(Case("ref_null", *reads, 0, 100, None))
    c.append(Case("ref_len_inside", *reads, 0, 100, REF[:33]))
    c.append(Case("ref_lower", *reads, 0, 100, bytes(REF[:100]).lower()))
    # the last, partial tile ends at INT32_MAX, with a record ending there
    top = (1 << 31) - 1
    c.append(Case("ends_at_int32_max", [rec(top - 290, "40M"), rec(top - 50, "50M", flag=16)],
                  [rec(top - 295, "100M"), rec(top - 60, "20M2D38M")], top - 300, top, REF))
    return c


def _patched(raw, at, fmt, value):
    b = bytearray(raw)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def rejection_cases():
    """A rejected record contributes nothing; the others still give their columns."""
    good_t = [rec(10, "40M"), rec(20, "10M2D20M", flag=16), rec(45, "30M")]
    good_n = [rec(5, "90M")]
    c = []
    # block_size reaches past the sample's bytes
    bad = rec(30, "25M", name="past")
    bad.raw = _patched(bad.raw, 0, "<i", len(bad.raw) - 4 + 100000)
    bad.bad = True
    c.append(Case("block_past_span", good_t[:2] + [bad] + good_t[2:], good_n, 0, 120, REF, SS_E_INVAL))
    # the last record's block is cut short by the end of the bytes
    bad = rec(50, "25M", name="cut")
    bad.bad = True
    b, off, frm = sample_of(good_t + [bad])
    c.append(Case("block_truncated", good_t + [bad], good_n, 0, 120, REF, SS_E_INVAL,
                  samples=((b[:-5].copy(), off, frm), sample_of(good_n))))
    # n_cigar reaches past the block
    bad = rec(21, "25M", name="ncig")
    bad.raw = _patched(bad.raw, 4 + 12, "<H", 500)
    bad.bad = True
    c.append(Case("n_cigar_past_block", good_t[:2] + [bad] + good_t[2:], good_n, 0, 120, REF, SS_E_INVAL))
    # the CIGAR's query length exceeds l_seq
    bad = rec(22, "20M", name="qlen")
    bad.raw = bamgen.encode_record(0, 22, "qlen", 60, 0, [("M", 30)], bad.seq, bad.qual)
    bad.bad = True
    c.append(Case("query_past_l_seq", good_t[:2] + [bad] + good_t[2:], good_n, 0, 120, REF, SS_E_INVAL))
    # from < pos
    bad = rec(40, "20M", name="early", from_=39)
    bad.bad = True
    c.append(Case("from_below_pos", good_t[:2] + [bad] + good_t[2:], good_n, 0, 120, REF, SS_E_INVAL))
    # from decreases: the call is refused
    dec = [rec(10, "40M", from_=30), rec(20, "40M", from_=29)]
    c.append(Case("from_decreasing", dec, good_n, 0, 120, REF, SS_E_INVAL, whole_call=True))
    # a record offset outside the bytes: the call is refused
    b, off, frm = sample_of(good_t)
    off = off.copy()
    off[-1] = b.size
    c.append(Case("offset_outside", good_t, good_n, 0, 120, REF, SS_E_INVAL, whole_call=True,
                  samples=((b, off, frm), sample_of(good_n))))
    return c


def mutated_cases(count, seed=11):
    """Valid samples with a few bytes changed: any code, no invalid access."""
    rng = random.Random(seed)
    base = [x for x in branch_cases() if x.name in ("every_op", "misaligned_cigars", "from_gt_beg")]
    out = []
    for i in range(count):
        src = base[i % len(base)]
        smp = []
        for k in range(2):
            b, off, frm = src.sample(k)
            b = b.copy()
            for _ in range(rng.randrange(1, 4)):
                if rng.random() < 0.7 and len(off):      # a byte of some record's fixed part or CIGAR
                    at = int(off[rng.randrange(len(off))]) + rng.randrange(0, 60)
                else:
                    at = rng.randrange(b.size)
                if at < b.size:
                    b[at] = rng.choice([0, 1, 0x7F, 0x80, 0xFF, rng.randrange(256)])
            smp.append((b, off, frm))
        out.append(Case(f"mut{i}", [], [], src.lo, src.hi, src.ref, ANY, samples=tuple(smp)))
    return out


def write_corpus(path, cases):
    """The file tests/native/pileup_driver.c reads (little-endian):
    u32 n_cases, then per case i32 lo, hi, rc, ref_len (-1: NULL) + ref bytes, and
    per sample u32 n, u64 n_bytes, the bytes, n u64 offsets, n i32 from."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            ref = c.ref
            f.write(struct.pack("<iiii", c.lo, c.hi, c.rc, -1 if ref is None else len(ref)))
            if ref is not None:
                f.write(bytes(ref))
            for k in range(2):
                b, off, frm = c.sample(k)
                f.write(struct.pack("<IQ", len(off), b.size))
                f.write(b.tobytes())
                f.write(np.asarray(off, "<u8").tobytes())
                f.write(np.asarray(frm, "<i4").tobytes())


# ---------------------------------------------------------------- files
def bam_records(data: bytes):
    """Uncompressed BAM bytes -> (record bytes after the header, contig names, lengths)."""
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    names, lens = [], []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, at)
        names.append(data[at + 4:at + 4 + l_name - 1].decode())
        lens.append(struct.unpack_from("<i", data, at + 4 + l_name)[0])
        at += 8 + l_name
    return data[at:], names, lens


def parse_dump(text: bytes):
    """SS_DUMP_PILEUP lines -> [(tid, pos, n1, n2, reads_t tuple, reads_n tuple)]."""
    out = []
    for line in text.decode().splitlines():
        tid, pos, n1, n2, _ref, rt, rn = line.split("\t")
        out.append((int(tid), int(pos), int(n1), int(n2), tuple(int(x, 16) for x in rt.split(",") if x),
                    tuple(int(x, 16) for x in rn.split(",") if x)))
    return out


def region_lines(tid, reg):
    """A PileupRegion as parse_dump tuples."""
    b = reg.batch
    return [(tid, int(reg.pos[i]), int(reg.raw_t[i]), int(reg.raw_n[i]),
             tuple(int(x) for x in b.reads_tumor[b.off_tumor[i]:b.off_tumor[i + 1]]),
             tuple(int(x) for x in b.reads_normal[b.off_normal[i]:b.off_normal[i + 1]])) for i in range(len(reg.pos))]
