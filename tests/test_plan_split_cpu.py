"""The device planner's split on the CPU (ss_pileup_split_cpu: the guess, the
walk, the stitch and the repair of csrc/ss_plan_core.h on the calling thread)
against a plain Python chain walk, at chunk sizes down to 64 bytes; and
ss_bam_header_scan.  Every comparison is exact.  No GPU."""
import gzip
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pileup_model as pm  # noqa: E402
import plan_cases as pc  # noqa: E402

CHUNKS = [64, 512, 4096]


def _check(pkg, span, chunk, n_ref=None):
    """The twin equals the plain walk; returns n_repaired."""
    want, end_at, bad = pc.walk(span.data)
    off, got_end, why, rep = pkg.pileup_split_cpu(span.data, span.n_ref if n_ref is None else n_ref, chunk)
    assert off.dtype == np.uint64 and off.tolist() == want, (span.name, chunk)
    assert got_end == end_at, (span.name, chunk)
    assert why == (pkg.SS_PLAN_END_BLOCK if bad else pkg.SS_PLAN_END_DATA), (span.name, chunk)
    n_chunks = -(-len(span.data) // chunk)
    assert rep <= n_chunks, (span.name, chunk, rep)
    return rep


@pytest.fixture(scope="module")
def dataset_records(datasets):
    """(label, record bytes, n_ref) of both BAMs of every pair."""
    out = []
    for i, (d, fa, t, n) in enumerate(datasets):
        for f in (t, n):
            recs, names, lens = pm.bam_records(gzip.decompress(open(os.path.join(d, f), "rb").read()))
            out.append((f"{i}/{f}", recs, len(names)))
    return out


def test_split_equals_plain_walk_on_datasets(pkg, dataset_records):
    assert pkg.SS_PLAN_CHUNK == 16384
    records = 0
    for label, recs, n_ref in dataset_records:
        for chunk in CHUNKS + [pkg.SS_PLAN_CHUNK]:
            _check(pkg, pc.Span(label, recs, chunk, n_ref), chunk)
        records += len(pc.walk(recs)[0])
    assert records > 10000


def test_no_repairs_on_ordinary_files(pkg, dataset_records):
    """A condition on the guess rule: on ordinary files no chunk guesses wrong."""
    chunks = 0
    for label, recs, n_ref in dataset_records:
        for chunk in (512, 4096):
            assert _check(pkg, pc.Span(label, recs, chunk, n_ref), chunk) == 0, (label, chunk)
            chunks += -(-len(recs) // chunk)
    assert chunks > 1000


@pytest.mark.parametrize("span", pc.boundary_cases(64) + pc.boundary_cases(512), ids=lambda s: f"{s.name}@{s.chunk}")
def test_boundary_cases(pkg, span):
    for chunk in (span.chunk, 64, 100, 4096):
        _check(pkg, span, chunk)
        _check(pkg, span, chunk, n_ref=0)


def test_boundary_cases_put_block_size_across_the_boundary():
    """The generator does what the case names say (at the case's own chunk size)."""
    for C in (64, 512):
        by = {s.name: s for s in pc.boundary_cases(C)}
        for d in range(-3, 4):
            assert C + d in pc.walk(by[f"start_at_boundary{d:+d}"].data)[0]
        assert C in pc.walk(by["ends_at_boundary"].data)[0]
        s = by["longer_than_three_chunks"].data
        starts = pc.walk(s)[0]
        assert max(b - a for a, b in zip(starts, starts[1:])) > 3 * C
        assert pc.walk(by["block_31"].data)[2] and pc.walk(by["block_negative"].data)[2]
        assert [len(by[f"len_{n}"].data) for n in (0, 3, 35, 36)] == [0, 3, 35, 36]
        for name in ("cut_in_head", "cut_in_body"):
            starts, end_at, bad = pc.walk(by[name].data)
            assert not bad and end_at < len(by[name].data) and end_at > C


@pytest.mark.parametrize("span", pc.decoy_cases(512), ids=lambda s: s.name)
def test_decoys_are_repaired(pkg, span):
    n_chunks = -(-len(span.data) // span.chunk)
    rep = _check(pkg, span, span.chunk)
    assert 0 < span.min_repairs <= rep <= n_chunks, (rep, n_chunks)
    if span.name == "decoy_every_chunk":
        assert n_chunks == 16 and rep == 15          # every chunk but the first: the bound
    for chunk in (64, 100, 4096):                    # other cuts: exact all the same
        _check(pkg, span, chunk)
    _check(pkg, span, span.chunk, n_ref=0)


def test_mutated_spans(pkg):
    for span in pc.mutated_cases(400):
        for chunk in (span.chunk, 64):
            _check(pkg, span, chunk)


def test_bam_header_scan(pkg, datasets):
    d, fa, t, n = datasets[0]
    data = gzip.decompress(open(os.path.join(d, t), "rb").read())
    recs, names, lens = pm.bam_records(data)
    at = len(data) - len(recs)
    assert pkg.bam_header_scan(data) == (len(names), at)
    assert pkg.bam_header_scan(data[:at]) == (len(names), at)
    for cut in (0, 1, 3, 4, 7, 8, 11, at // 2, at - 1):
        assert pkg.bam_header_scan(data[:cut]) is None, cut
    assert pkg.bam_header_scan(b"BA") is None
    for bad in (b"BAN\1" + data[4:], b"BX", b"XAM\1",
                data[:4] + struct.pack("<i", -1) + data[8:],
                data[:at - 4 - sum(8 + len(x) + 1 for x in names)] + struct.pack("<i", -2)):
        with pytest.raises(pkg.SniperError) as e:
            pkg.bam_header_scan(bad)
        assert e.value.code == pkg.SS_E_INVAL
    d, fa, t, n = datasets[5]                         # region-like contig names
    data = gzip.decompress(open(os.path.join(d, t), "rb").read())
    recs, names, lens = pm.bam_records(data)
    assert pkg.bam_header_scan(data) == (len(names), len(data) - len(recs))
