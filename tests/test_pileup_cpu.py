"""Pileup columns from BAM records, host side (no GPU): the shared core run by
ss_pileup_region_cpu against a brute-force model of the pileup rules, the
rejection of invalid records, and ss_pileup_plan + region against the native
CLI's own site stream (SS_PILEUP_ONLY / SS_DUMP_PILEUP) for every dataset.
Every comparison is exact."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pileup_model as pm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "somatic-sniper_amd", "bam-somaticsniper")

BRANCH = pm.branch_cases()
REJECT = pm.rejection_cases()


@pytest.mark.parametrize("case", BRANCH, ids=[c.name for c in BRANCH])
def test_region_cpu_equals_model(pkg, case):
    want = pm.model_region(case.tumor, case.normal, case.ref, case.lo, case.hi)
    reg = pkg.pileup_region_cpu(case.sample(0), case.sample(1), case.ref, case.lo, case.hi)
    assert reg.rc == 0 and reg.n_invalid == 0
    got = pm.region_arrays(reg)
    assert pm.same(got, want), case.name
    if case.name == "deletion_only":       # a site with zero packed depth in the tumor
        i = list(reg.pos).index(56)
        assert reg.raw_t[i] == 1 and reg.batch.off_tumor[i] == reg.batch.off_tumor[i + 1]
    if case.name == "skip_only":
        assert 57 not in reg.pos and 52 in reg.pos
    if case.name == "empty_sample":
        assert len(reg.pos) == 0 and list(reg.batch.off_tumor) == [0]
    if case.name == "ends_at_int32_max":
        assert reg.pos[-1] == (1 << 31) - 2 and len(reg.pos) == 90
    if case.name == "depth_65_300":
        i = list(reg.pos).index(100)
        j = list(reg.pos).index(104)
        assert reg.raw_t[i] == 65 and reg.raw_n[j] == 300


@pytest.mark.parametrize("case", REJECT, ids=[c.name for c in REJECT])
def test_rejections(pkg, case):
    if case.whole_call:
        with pytest.raises(pkg.SniperError) as e:
            pkg.pileup_region_cpu(case.sample(0), case.sample(1), case.ref, case.lo, case.hi, invalid_ok=True)
        assert e.value.code == case.rc
        return
    with pytest.raises(pkg.SniperError):
        pkg.pileup_region_cpu(case.sample(0), case.sample(1), case.ref, case.lo, case.hi)
    reg = pkg.pileup_region_cpu(case.sample(0), case.sample(1), case.ref, case.lo, case.hi, invalid_ok=True)
    assert reg.rc == pkg.SS_E_INVAL and reg.n_invalid == 1
    want = pm.model_region(case.tumor, case.normal, case.ref, case.lo, case.hi)
    assert pm.same(pm.region_arrays(reg), want), case.name


def test_bad_regions(pkg):
    c = BRANCH[0]
    for lo, hi in ((10, 10), (20, 10), (0, (1 << 22) + 1), (-1, 10)):
        with pytest.raises(pkg.SniperError) as e:
            pkg.pileup_region_cpu(c.sample(0), c.sample(1), c.ref, lo, hi)
        assert e.value.code == pkg.SS_E_INVAL


GUARD = 0xDEADBEEF


def test_capacity_one_too_small_touches_nothing(pkg):
    """Each capacity in turn one below the need: SS_E_CAPACITY, the needed sizes
    reported, and every array -- the guard words after it included -- untouched."""
    lib = pkg.load_library()
    c = BRANCH[0]
    full = pkg.pileup_region_cpu(c.sample(0), c.sample(1), c.ref, c.lo, c.hi)
    ns, nt, nn = len(full.pos), len(full.batch.reads_tumor), len(full.batch.reads_normal)
    assert ns and nt and nn
    st, _alive_t = pkg._pileup_sample(c.sample(0))     # the arrays the structs point into
    sn, _alive_n = pkg._pileup_sample(c.sample(1))
    ref = np.frombuffer(c.ref, np.uint8)
    dts = [np.int32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32]
    for short in range(3):
        caps = [ns, nt, nn]
        caps[short] -= 1
        sizes = [caps[0]] * 4 + [caps[0] + 1] * 2 + [caps[1], caps[2]]
        arrays = []
        for n, dt in zip(sizes, dts):
            a = np.full(n + 4, GUARD & (0xFF if dt is np.uint8 else 0x7FFFFFFF), dt)
            arrays.append(a)
        before = [a.copy() for a in arrays]
        out = pkg._PileupOut(caps[0], caps[1], caps[2], *(a.ctypes.data for a in arrays))
        rc = lib.ss_pileup_region_cpu(C.byref(st), C.byref(sn), ref.ctypes.data, ref.size, c.lo, c.hi, C.byref(out))
        assert rc == pkg.SS_E_CAPACITY
        assert (out.n_sites, out.n_reads_t, out.n_reads_n) == (ns, nt, nn)
        assert all((a == b).all() for a, b in zip(arrays, before))
    # exact capacities: filled, and the guard words stay
    sizes = [ns] * 4 + [ns + 1] * 2 + [nt, nn]
    arrays = [np.full(n + 4, 0x5A, dt) for n, dt in zip(sizes, dts)]
    out = pkg._PileupOut(ns, nt, nn, *(a.ctypes.data for a in arrays))
    assert lib.ss_pileup_region_cpu(C.byref(st), C.byref(sn), ref.ctypes.data, ref.size, c.lo, c.hi,
                                    C.byref(out)) == 0
    for a, n, w in zip(arrays, sizes, pm.region_arrays(full)):
        assert (a[:n] == w).all() and (a[n:] == 0x5A).all()


# ---------------------------------------------------------------- planner
def _plan_file(pkg, path, thresh):
    recs, names, lens = pm.bam_records(gzip.decompress(open(path, "rb").read()))
    off, frm, tid, used = pkg.pileup_plan(recs, -1, thresh)
    assert used == len(recs)
    return np.frombuffer(recs, np.uint8), off, frm, tid, len(names)


def plan_lines(pkg, region, d, t, n, thresh):
    """Every contig of a BAM pair as one region with ref=NULL -> dump tuples."""
    bt, ot, ft, tt, n_ref = _plan_file(pkg, os.path.join(d, t), thresh)
    bn, on, fn, tn, _ = _plan_file(pkg, os.path.join(d, n), thresh)
    lines = []
    for tid in range(n_ref):
        mt, mn = tt == tid, tn == tid
        if not mt.any() or not mn.any():
            continue
        # past the last position any record reaches: no read spans 4096 positions
        hi = min(int(max(ft[mt].max(), fn[mn].max())) + 4096, 1 << 22)
        reg = region((bt, ot[mt], ft[mt]), (bn, on[mn], fn[mn]), None, 0, hi)
        lines += pm.region_lines(tid, reg)
    return lines


def cli_lines(d, fa, t, n, opts, tmp_path):
    name = str(tmp_path / "cli.dump")
    if os.path.exists(name):
        os.remove(name)
    p = subprocess.run([CLI] + opts + ["-f", os.path.join(d, fa), os.path.join(d, t), os.path.join(d, n),
                                       str(tmp_path / "cli.out")], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, SS_PILEUP_ONLY="1", SS_DUMP_PILEUP=name))
    assert p.returncode == 0, p.stderr[-2000:]
    return pm.parse_dump(open(name, "rb").read() if os.path.exists(name) else b"")


@pytest.mark.parametrize("opts", [[], ["-q", "20"]], ids=["default", "q20"])
def test_plan_and_region_equal_cli_site_stream(pkg, datasets, tmp_path, opts):
    """The first-read-of-a-later-contig drop, unsorted positions, unmapped
    reads and an empty normal BAM are all in the datasets."""
    thresh = int(opts[1]) if opts else 0
    total = 0
    for d, fa, t, n in datasets:
        want = cli_lines(d, fa, t, n, opts, tmp_path)
        got = plan_lines(pkg, pkg.pileup_region_cpu, d, t, n, thresh)
        assert len(got) == len(want), (d, len(got), len(want))
        for g, w in zip(got, want):
            assert g == w, (d, g[:4], w[:4])
        total += len(got)
    assert total > 10000


def test_plan_in_chunks_of_three_records(pkg, datasets):
    for d, fa, t, n in datasets:
        for f in (t, n):
            recs, _, _ = pm.bam_records(gzip.decompress(open(os.path.join(d, f), "rb").read()))
            recs = np.frombuffer(recs, np.uint8)
            one = pkg.pileup_plan(recs, -1, 0)
            state = pkg.PileupState()
            at, parts = 0, []
            while True:
                off, frm, tid, used = pkg.pileup_plan(recs[at:], -1, 0, state=state, cap=3)
                parts.append((off + np.uint64(at), frm, tid))
                at += used
                if len(off) < 3:
                    break
            assert at == len(recs) == one[3]
            for k in range(3):
                assert (np.concatenate([p[k] for p in parts]) == one[k]).all(), (d, f, k)


def test_plan_truncated_tail_and_unsorted_contigs(pkg):
    a = pm.rec(10, "20M", tid=1).raw
    b = pm.rec(5, "20M", tid=0).raw
    off, frm, tid, used = pkg.pileup_plan(a + a[:-3])
    assert list(off) == [0] and used == len(a)              # a truncated tail is not an error
    with pytest.raises(pkg.SniperError) as e:
        pkg.pileup_plan(a + b)
    assert e.value.code == pkg.SS_E_INVAL
    # the filter runs first: a masked record on a lower contig is no sortedness error
    masked = pm.rec(5, "20M", tid=0, flag=0x400).raw
    off, frm, tid, used = pkg.pileup_plan(a + masked + a)
    assert list(tid) == [1, 1] and used == 2 * len(a) + len(masked)
