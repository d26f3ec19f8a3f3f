"""Pileup columns from BAM records on the GPU (ss_pileup.hip): the device path
must give the arrays and return codes of the CPU twin (ss_pileup_region_cpu,
itself checked against a model and the CLI by test_pileup_cpu.py) -- on every
branch and rejection case of tests/pileup_model.py, on every dataset contig,
across region splits, chained into the scorer without a host copy, through
the guard-band build and from two threads.  Every comparison is exact.

The rejection cases ran through the ASan / UBSan driver on the CPU first
(test_pileup_sanitizers.py); here they take the kernels' bounded reject path."""
import dataclasses
import gzip
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pileup_model as pm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

BRANCH = pm.branch_cases()
REJECT = pm.rejection_cases()


@pytest.fixture(scope="module")
def pile(pkg):
    with pkg.Pileup(device=0) as p:
        yield p


def _region(pkg, fn, case):
    """(rc, n_invalid, arrays or None) of one region call."""
    try:
        reg = fn(case.sample(0), case.sample(1), case.ref, case.lo, case.hi, invalid_ok=True)
    except pkg.SniperError as e:
        return e.code, None, None
    return reg.rc, reg.n_invalid, pm.region_arrays(reg)


@pytest.mark.parametrize("case", BRANCH + REJECT, ids=[c.name for c in BRANCH + REJECT])
def test_region_device_equals_cpu(pkg, pile, case):
    rc_c, bad_c, cpu = _region(pkg, pkg.pileup_region_cpu, case)
    rc_d, bad_d, dev = _region(pkg, pile.region, case)
    assert (rc_d, bad_d) == (rc_c, bad_c) and rc_c == case.rc
    assert (dev is None) == (cpu is None) == case.whole_call
    if cpu is not None:
        assert pm.same(dev, cpu), case.name
    pile.check()


@pytest.mark.parametrize("case", [c for c in REJECT if c.samples is None], ids=lambda c: c.name)
def test_device_calls_report_invalid_records_at_check(pkg, pile, case):
    """count / fill over device inputs: a rejected record (for the device calls
    also one whose `from` decreases, which only the device can see there)
    contributes nothing, the other columns are written, and ss_pileup_check
    reports SS_E_INVAL once."""
    pile.check()
    tumor = list(case.tumor)
    if case.name == "from_decreasing":
        tumor[1] = dataclasses.replace(tumor[1], bad=True)     # its `from` is below its predecessor's
    want = pm.model_region(tumor, case.normal, case.ref, case.lo, case.hi)
    r = pile.region_device(case.sample(0), case.sample(1), case.ref, case.lo, case.hi)
    ns, (nt, nn) = r["n_sites"], r["n_reads"]
    with pytest.raises(pkg.SniperError) as e:
        pile.check()
    assert e.value.code == pkg.SS_E_INVAL
    pile.check()                                  # cleared
    if case.name == "from_decreasing":            # reported and bounded; the columns are unspecified then
        return
    got = (r["pos"][:ns], r["ref"][:ns], r["raw_t"][:ns], r["raw_n"][:ns], r["off_tumor"], r["off_normal"],
           r["reads_tumor"][:nt], r["reads_normal"][:nn])
    got = tuple(g.cpu().numpy().view(w.dtype) for g, w in zip(got, want))
    assert pm.same(got, want), case.name


DTS = [np.int32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32]
TAIL = 4                                          # guard words after each array


def _sizes(ns, nt, nn):
    return [ns] * 4 + [ns + 1] * 2 + [nt, nn]


def test_region_capacity_one_too_small_touches_nothing(pkg, pile):
    """ss_pileup_region_host with each capacity in turn one below the need:
    SS_E_CAPACITY, the needed sizes reported, every array and the guard words
    after it untouched; with exact capacities the arrays are filled and the
    guard words stay."""
    import ctypes as C
    lib = pkg.load_library()
    c = BRANCH[0]
    full = pkg.pileup_region_cpu(c.sample(0), c.sample(1), c.ref, c.lo, c.hi)
    ns, nt, nn = len(full.pos), len(full.batch.reads_tumor), len(full.batch.reads_normal)
    assert ns and nt and nn
    st, _alive_t = pkg._pileup_sample(c.sample(0))
    sn, _alive_n = pkg._pileup_sample(c.sample(1))
    ref = np.frombuffer(c.ref, np.uint8)
    for short in range(3):
        caps = [ns, nt, nn]
        caps[short] -= 1
        arrays = [np.full(n + TAIL, 0x5A, dt) for n, dt in zip(_sizes(*caps), DTS)]
        out = pkg._PileupOut(*caps, *(a.ctypes.data for a in arrays))
        rc = lib.ss_pileup_region_host(pile.h, C.byref(st), C.byref(sn), ref.ctypes.data, ref.size, c.lo, c.hi,
                                       C.byref(out))
        assert rc == pkg.SS_E_CAPACITY
        assert (out.n_sites, out.n_reads_t, out.n_reads_n) == (ns, nt, nn)
        assert all((a == 0x5A).all() for a in arrays)
    arrays = [np.full(n + TAIL, 0x5A, dt) for n, dt in zip(_sizes(ns, nt, nn), DTS)]
    out = pkg._PileupOut(ns, nt, nn, *(a.ctypes.data for a in arrays))
    assert lib.ss_pileup_region_host(pile.h, C.byref(st), C.byref(sn), ref.ctypes.data, ref.size, c.lo, c.hi,
                                     C.byref(out)) == 0
    for a, n, w in zip(arrays, _sizes(ns, nt, nn), pm.region_arrays(full)):
        assert (a[:n] == w).all() and (a[n:] == 0x5A).all()
    pile.check()


def test_fill_capacity_one_too_small_stores_nothing(pkg, pile):
    """ss_pileup_fill_device with each capacity one short: SS_E_CAPACITY and the
    output tensors untouched; with exact capacities they are filled and the
    words after each array stay."""
    import torch
    dev = torch.device("cuda", 0)
    c = BRANCH[0]
    full = pkg.pileup_region_cpu(c.sample(0), c.sample(1), c.ref, c.lo, c.hi)
    ns, nt, nn = len(full.pos), len(full.batch.reads_tumor), len(full.batch.reads_normal)
    smp = []
    for data, off, frm in (c.sample(0), c.sample(1)):
        smp.append((torch.from_numpy(data.copy()).to(dev), data.size, torch.from_numpy(off.astype(np.int64)).to(dev),
                    torch.from_numpy(frm.copy()).to(dev), len(off)))
    d_ref = torch.from_numpy(np.frombuffer(c.ref, np.uint8).copy()).to(dev)
    torch.cuda.synchronize(dev)
    assert pile.count(smp[0], smp[1], d_ref, len(c.ref), c.lo, c.hi) == (ns, nt, nn)
    tds = [torch.int32, torch.uint8] + [torch.int32] * 6

    def fresh():
        return [torch.full((n + TAIL,), 0x5A, dtype=td, device=dev) for n, td in zip(_sizes(ns, nt, nn), tds)]

    for short in range(3):
        caps = [ns, nt, nn]
        caps[short] -= 1
        out = fresh()
        with pytest.raises(pkg.SniperError) as e:
            pile.fill(*out, *caps)
        assert e.value.code == pkg.SS_E_CAPACITY
        torch.cuda.synchronize(dev)
        assert all(bool((t == 0x5A).all()) for t in out)
    out = fresh()
    pile.fill(*out, ns, nt, nn)
    pile.check()
    for t, n, w in zip(out, _sizes(ns, nt, nn), pm.region_arrays(full)):
        a = t.cpu().numpy().view(w.dtype)
        assert (a[:n] == w).all() and (t[n:] == 0x5A).all()


def _planned(pkg, path):
    recs, names, lens = pm.bam_records(gzip.decompress(open(path, "rb").read()))
    off, frm, tid, used = pkg.pileup_plan(recs)
    assert used == len(recs)
    return np.frombuffer(recs, np.uint8), off, frm, tid, names


def _contigs(pkg, d, t, n):
    """(tid, name, tumor sample, normal sample, hi) of every contig both BAMs cover."""
    bt, ot, ft, tt, names = _planned(pkg, os.path.join(d, t))
    bn, on, fn, tn, _ = _planned(pkg, os.path.join(d, n))
    for tid in range(len(names)):
        mt, mn = tt == tid, tn == tid
        if mt.any() and mn.any():
            hi = int(max(ft[mt].max(), fn[mn].max())) + 4096      # no read spans 4096 positions
            yield tid, names[tid], (bt, ot[mt], ft[mt]), (bn, on[mn], fn[mn]), hi


@pytest.fixture(scope="module")
def contig_results(pkg, datasets):
    """The CPU twin's region of every dataset contig (computed once, read-only)."""
    out = []
    for i, (d, fa, t, n) in enumerate(datasets):
        for tid, name, st, sn, hi in _contigs(pkg, d, t, n):
            reg = pkg.pileup_region_cpu(st, sn, None, 0, hi)
            for a in pm.region_arrays(reg):
                a.setflags(write=False)
            out.append((i, tid, name, st, sn, hi, reg))
    return out


def test_datasets_device_equals_cpu(pkg, pile, contig_results):
    sites = 0
    for i, tid, name, st, sn, hi, cpu in contig_results:
        dev = pile.region(st, sn, None, 0, hi)
        assert pm.same(pm.region_arrays(dev), pm.region_arrays(cpu)), (i, tid)
        sites += len(cpu.pos)
    pile.check()
    assert sites > 10000


def test_three_regions_equal_one(pkg, pile, contig_results):
    """Split points inside reads: the pieces, concatenated, are the whole."""
    i, tid, name, st, sn, hi, whole = max(contig_results, key=lambda r: len(r[6].pos))
    last = int(whole.pos[-1]) + 1
    cuts = [0, last // 3 + 1, 2 * last // 3 - 5, hi]
    parts = [pile.region(st, sn, None, a, b) for a, b in zip(cuts, cuts[1:])]
    assert all(len(p.pos) for p in parts)
    b = [p.batch for p in parts]

    def joined(offs, reads):
        out, base = [np.zeros(1, np.uint32)], 0
        for o, r in zip(offs, reads):
            out.append(o[1:] + np.uint32(base))
            base += len(r)
        return np.concatenate(out)

    got = (np.concatenate([p.pos for p in parts]), np.concatenate([x.ref for x in b]),
           np.concatenate([p.raw_t for p in parts]), np.concatenate([p.raw_n for p in parts]),
           joined([x.off_tumor for x in b], [x.reads_tumor for x in b]),
           joined([x.off_normal for x in b], [x.reads_normal for x in b]),
           np.concatenate([x.reads_tumor for x in b]), np.concatenate([x.reads_normal for x in b]))
    assert pm.same(got, pm.region_arrays(whole))


def _fasta(path):
    seqs, name = {}, None
    for line in open(path):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.strip())
    return {k: "".join(v).encode() for k, v in seqs.items()}


@pytest.mark.parametrize("which", [0, 2], ids=["integration", "pair2_60x30"])
def test_chained_into_scorer(pkg, pile, ctx, datasets, which):
    """count -> fill -> score_device with the batch never leaving the device;
    scores and calls equal score_batch over the CPU twin's batch."""
    import torch
    dev = torch.device("cuda", 0)
    d, fa, t, n = datasets[which]
    fasta = _fasta(os.path.join(d, fa))
    sites = 0
    for tid, name, st, sn, hi in _contigs(pkg, d, t, n):
        ref = fasta[name]
        cpu = pkg.pileup_region_cpu(st, sn, ref, 0, hi)
        want_score, want_calls, _ = ctx.score_batch(cpu.batch, calls_cap=max(16, len(cpu.pos)))
        r = pile.region_device(st, sn, ref, 0, hi)
        ns = r["n_sites"]
        assert ns == len(cpu.pos)
        score = torch.full((ns,), 12345, dtype=torch.int32, device=dev)
        calls = torch.zeros(max(16, ns) * pkg.SS_CALL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        n_calls = torch.zeros(1, dtype=torch.int32, device=dev)
        ctx.score_device(r["ref"], r["off_tumor"], r["off_normal"], r["reads_tumor"], r["reads_normal"], score,
                         calls=calls, calls_cap=max(16, ns), n_calls=n_calls, n_sites=ns)
        ctx.check()
        pile.check()
        assert (score.cpu().numpy() == want_score).all(), (name,)
        k = int(n_calls.cpu()[0])
        got_calls = np.sort(calls.cpu().numpy().view(pkg.SS_CALL_DTYPE)[:k], order="site")
        assert k == len(want_calls) and (got_calls.view("u1") == want_calls.view("u1")).all(), (name,)
        assert (r["pos"][:ns].cpu().numpy() == cpu.pos).all()
        sites += ns
    assert sites > 0


_DEBUG_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import pileup_model as pm
from __graft_entry__ import load_package
pkg = load_package()
same = 1
with pkg.Pileup() as p:                             # one handle: its buffers grow from case to case
    for c in pm.branch_cases():
        cpu = pkg.pileup_region_cpu(c.sample(0), c.sample(1), c.ref, c.lo, c.hi)
        dev = p.region(c.sample(0), c.sample(1), c.ref, c.lo, c.hi)
        same &= int(pm.same(pm.region_arrays(dev), pm.region_arrays(cpu)))
    rc = p.lib.ss_pileup_check(p.h)
print("CHECK", rc, "SAME", same)
"""


def test_debug_build_guard_bands():
    """The branch cases through the guard-band build: no byte around the
    handle's device buffers changes (ss_pileup_check)."""
    lib = os.path.join(ROOT, "somatic-sniper_amd", "build", "debug", "libsniper_amd.so")
    assert os.path.exists(lib), "make -C somatic-sniper_amd debug (built by __graft_entry__.build)"
    p = subprocess.run([sys.executable, "-c", _DEBUG_CHILD, ROOT], env=dict(os.environ, SNIPER_AMD_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "CHECK 0 SAME 1" in p.stdout, (p.stdout, p.stderr[-2000:])
    assert "guard band" not in p.stderr, p.stderr[-2000:]


def test_two_handles_two_threads(pkg, pile, contig_results):
    work = sorted(contig_results, key=lambda r: -len(r[6].pos))[:6]
    got = [None] * len(work)
    errors = []

    def run(k0):
        try:
            with pkg.Pileup(device=0) as p:
                for k in range(k0, len(work), 2):
                    i, tid, name, st, sn, hi, cpu = work[k]
                    got[k] = pm.region_arrays(p.region(st, sn, None, 0, hi))
                p.check()
        except Exception as e:          # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for k, w in enumerate(work):
        assert pm.same(got[k], pm.region_arrays(w[6])), k
        assert pm.same(pm.region_arrays(pile.region(w[3], w[4], None, 0, w[5])), got[k])
