"""The planner on the GPU (ss_pileup_plan_device, csrc/ss_pileup.hip) must give
what ss_pileup_plan gives on the host for the same bytes, mask, threshold,
in-state and capacity: the three arrays, n, consumed, the out-state and the
code -- on the dataset BAMs, on the boundary / break / decoy spans of
tests/plan_cases.py scaled to SS_PLAN_CHUNK, on the load rules' quirks, under
a capacity, across calls that carry the state, and chained from inflated
device bytes into the scorer.  Every comparison is exact.

The spans ran through the ASan / UBSan driver on the CPU first
(test_plan_sanitizers.py)."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pileup_model as pm  # noqa: E402
import plan_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CHUNK = 16384
SPANS = pc.cases(CHUNK)
QUIRKS = pc.quirk_cases()


@pytest.fixture(scope="module")
def pile(pkg):
    assert pkg.SS_PLAN_CHUNK == CHUNK
    with pkg.Pileup(device=0) as p:
        yield p


def host_plan(pkg, data, mask=-1, thresh=0, state=None, cap=None):
    """ss_pileup_plan with its code returned, not raised: (rc, off, from, tid, consumed, out-state)."""
    lib = pkg.load_library()
    a = np.frombuffer(bytes(data), np.uint8)
    st = pkg.PileupState() if state is None else pkg.PileupState.from_buffer_copy(state)
    if cap is None:
        cap = a.size // 36 + 1
    off, frm, tid = np.zeros(cap, np.uint64), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    n, used = C.c_uint32(), C.c_size_t()
    rc = lib.ss_pileup_plan(a.ctypes.data if a.size else None, a.size, mask, thresh, C.byref(st), off.ctypes.data,
                            frm.ctypes.data, tid.ctypes.data, cap, C.byref(n), C.byref(used))
    k = n.value
    return rc, off[:k], frm[:k], tid[:k], int(used.value), st


def to_device(data, shift=3):
    """The bytes at an address `shift` past an allocation's start (record bytes have no
    alignment: they follow a header): (tensor kept alive, address)."""
    import torch
    a = np.zeros(shift + len(data) + 1, np.uint8)
    a[shift:shift + len(data)] = np.frombuffer(bytes(data), np.uint8)
    t = torch.from_numpy(a).to(torch.device("cuda", 0))
    return t, t.data_ptr() + shift


def _state(st):
    return (st.has_prev, st.tid, st.w, st.max_tid)


def ref_end(data, off):
    pos, = struct.unpack_from("<i", data, off + 8)
    l_name = data[off + 12]
    n_cigar, = struct.unpack_from("<H", data, off + 16)
    end = pos
    for k in range(n_cigar):
        c, = struct.unpack_from("<I", data, off + 36 + l_name + 4 * k)
        if c & 0xF in (0, 2, 3):
            end += c >> 4
    return (end + (1 << 31)) % (1 << 32) - (1 << 31)


def grouped(data, off, frm, tid):
    """The runs, from a numpy grouping of the host arrays."""
    out = []
    cuts = [0] + [i for i in range(1, len(tid)) if tid[i] != tid[i - 1]] + [len(tid)]
    for a, b in zip(cuts, cuts[1:]):
        if b > a:
            out.append((int(tid[a]), a, b - a, int(frm[a:b].min()), max(ref_end(data, int(o)) for o in off[a:b])))
    return out


def compare(pkg, pile, data, n_ref, mask=-1, thresh=0, state=None, cap=None, shift=3, runs=True):
    """One device call against one host call; returns the device result and both states."""
    rc, off, frm, tid, used, st_h = host_plan(pkg, data, mask, thresh, state, cap)
    keep, addr = to_device(data, shift)
    st_d = pkg.PileupState() if state is None else pkg.PileupState.from_buffer_copy(state)
    d_off, d_frm, d_tid, d_used, d_runs, rep = pile.plan_device(addr, len(data), n_ref, mask, thresh, st_d, cap,
                                                                invalid_ok=True)
    assert pile.last_plan_rc == rc
    assert d_used == used
    assert _state(st_d) == _state(st_h)
    assert len(d_off) == len(off)
    assert (d_off.cpu().numpy().view(np.uint64) == off).all()
    assert (d_frm.cpu().numpy() == frm).all()
    assert (d_tid.cpu().numpy() == tid).all()
    if runs:
        assert [tuple(int(x) for x in r) for r in d_runs] == grouped(bytes(data), off, frm, tid)
    return (rc, off, frm, tid, used), rep, st_d


@pytest.fixture(scope="module")
def dataset_records(datasets):
    out = []
    for i, (d, fa, t, n) in enumerate(datasets):
        for f in (t, n):
            recs, names, lens = pm.bam_records(gzip.decompress(open(os.path.join(d, f), "rb").read()))
            out.append((f"{i}/{f}", recs, len(names)))
    return out


@pytest.mark.parametrize("mask,thresh", [(-1, 0), (0x400, 20)], ids=["default", "mask400_q20"])
def test_datasets_device_equals_host(pkg, pile, dataset_records, mask, thresh):
    kept = 0
    for label, recs, n_ref in dataset_records:
        (rc, off, *_), rep, _ = compare(pkg, pile, recs, n_ref, mask, thresh, shift=0 if len(recs) % 2 else 3)
        assert rc == 0, label
        assert rep == pkg.pileup_split_cpu(recs, n_ref, CHUNK)[3], label
        kept += len(off)
    pile.check()
    assert kept > 10000


@pytest.mark.parametrize("span", SPANS, ids=lambda s: s.name)
def test_span_corpus_device_equals_host(pkg, pile, span):
    """Boundaries at multiples of SS_PLAN_CHUNK (one LDS window is one chunk), long
    records, short spans, cut and bad records, decoys."""
    n_chunks = -(-len(span.data) // CHUNK)
    assert n_chunks <= 20
    (rc, off, *_), rep, _ = compare(pkg, pile, span.data, span.n_ref)
    want, end_at, bad = pc.walk(span.data)
    assert rc == (pkg.SS_E_INVAL if bad else 0)
    assert len(off) == len(want)                   # ascending positions on one contig: every record is kept
    assert rep == pkg.pileup_split_cpu(span.data, span.n_ref, CHUNK)[3]
    assert span.min_repairs <= rep <= n_chunks
    compare(pkg, pile, span.data, 0, shift=16)     # contig count unknown; an aligned address
    pile.check()


@pytest.mark.parametrize("span", QUIRKS, ids=lambda s: s.name)
def test_load_rule_quirks(pkg, pile, span):
    (rc, off, frm, tid, used), _, _ = compare(pkg, pile, span.data, pc.N_REF)
    starts = pc.walk(span.data)[0]
    if span.name == "contig_change_end_below_old_w":
        assert rc == 0 and starts[2] not in off.tolist() and starts[3] in off.tolist()
        assert frm[off.tolist().index(starts[3])] == 20
    if span.name == "pos_minus_one":
        assert rc == 0 and off.tolist() == [starts[0], starts[2], starts[3], starts[4]]
        assert frm.tolist() == [0, 3, -1, 0]       # -1 only where the contig changes: from = beg there
    if span.name == "lower_contig_after_higher":
        assert rc == pkg.SS_E_INVAL and off.tolist() == starts[:2] and used == starts[2]
    if span.name == "filtered_lower_contig_is_no_error":
        assert rc == 0 and off.tolist() == [starts[0], starts[3]]
    if span.name == "cigar_passes_block_filtered_then_kept":
        assert rc == pkg.SS_E_INVAL and off.tolist() == [starts[0], starts[2]] and used == starts[3]
    compare(pkg, pile, span.data, pc.N_REF, mask=0, thresh=0)
    st = pkg.PileupState(1, 1, 15, 1, 0)
    compare(pkg, pile, span.data, pc.N_REF, state=st)
    st = pkg.PileupState(1, 2, -7, -1, 0)          # an in-state no walk leaves: carried as the host carries it
    compare(pkg, pile, span.data, pc.N_REF, state=st)
    pile.check()


def test_cap_ends_the_walk_after_the_last_kept_record(pkg, pile, dataset_records):
    """cap one below the kept count, with filtered records after the last kept one:
    consumed is the offset after that record, as on the host."""
    label, recs, n_ref = dataset_records[2 * 5]                 # pair 5 tumor: unmapped reads
    rc, off, frm, tid, used, _ = host_plan(pkg, recs, 0x400, 20)
    assert rc == 0 and len(off) > 10
    (rc, off1, _, _, used1), _, _ = compare(pkg, pile, recs, n_ref, 0x400, 20, cap=len(off) - 1)
    assert len(off1) == len(off) - 1 and used1 <= int(off[-1]) < used
    g = pc.Gen(50)
    data = g.some(5) + g.sized(80, flag=0x400) + g.sized(90, flag=0x100) + g.some(1) + g.sized(70, flag=0x200)
    starts = pc.walk(data)[0]
    (rc, off2, _, _, used2), _, _ = compare(pkg, pile, data, pc.N_REF, cap=5)
    assert rc == 0 and len(off2) == 5 and used2 == starts[5]    # not after the filtered records that follow
    (rc, off3, _, _, used3), _, _ = compare(pkg, pile, data, pc.N_REF, cap=6)
    assert len(off3) == 6 and used3 == starts[8]
    compare(pkg, pile, data, pc.N_REF, cap=0)
    pile.check()


def test_three_calls_carrying_the_state_equal_one(pkg, pile, dataset_records):
    label, recs, n_ref = max(dataset_records, key=lambda r: len(r[1]))
    (rc, off, frm, tid, used), _, st_whole = compare(pkg, pile, recs, n_ref)
    assert rc == 0 and used == len(recs)
    cuts = [len(recs) // 3 + 5, 2 * len(recs) // 3 + 11, len(recs)]
    starts = set(pc.walk(recs)[0])
    assert cuts[0] not in starts and cuts[1] not in starts      # cut inside records
    st = pkg.PileupState()
    at, parts = 0, []
    for cut in cuts:
        (rc, o, f, t, u), _, st = compare(pkg, pile, recs[at:cut], n_ref, state=st, runs=False)
        assert rc == 0
        parts.append((o + np.uint64(at), f, t))
        at += u
    assert at == len(recs)
    assert (np.concatenate([p[0] for p in parts]) == off).all()
    assert (np.concatenate([p[1] for p in parts]) == frm).all()
    assert (np.concatenate([p[2] for p in parts]) == tid).all()
    assert _state(st) == _state(st_whole)


def test_capacities_untouched_memory_and_determinism(pkg, pile, dataset_records):
    import torch
    dev = torch.device("cuda", 0)
    lib = pkg.load_library()
    label, recs, n_ref = dataset_records[2 * 4]                 # pair 4: five contigs
    rc, off, frm, tid, used, _ = host_plan(pkg, recs)
    n, n_runs = len(off), len(grouped(recs, off, frm, tid))
    assert n_runs >= 3
    keep, addr = to_device(recs)

    def run(cap_runs, pad=7):
        arrays = [torch.full((n + pad,), 0x5A, dtype=torch.uint8, device=dev).repeat_interleave(w).contiguous()
                  for w in (8, 4, 4)]
        runs = np.full(max(1, cap_runs), 0x5A5A5A5A, np.uint32).repeat(5)
        st = pkg.PileupState()
        k, u, nr, rep = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        torch.cuda.synchronize(dev)
        rc = lib.ss_pileup_plan_device(pile.h, addr, len(recs), n_ref, -1, 0, C.byref(st), arrays[0].data_ptr(),
                                       arrays[1].data_ptr(), arrays[2].data_ptr(), n + pad, C.byref(k), C.byref(u),
                                       runs.ctypes.data, cap_runs, C.byref(nr), C.byref(rep), None)
        torch.cuda.synchronize(dev)
        return rc, [a.cpu().numpy() for a in arrays], runs, k.value, u.value, nr.value

    rc, arrays, runs, k, u, nr = run(n_runs - 1)
    assert rc == pkg.SS_E_CAPACITY and nr == n_runs and (runs == 0x5A5A5A5A).all()
    rc, arrays, runs, k, u, nr = run(n_runs)
    assert rc == 0 and (k, u, nr) == (n, used, n_runs)
    for a, w, want in zip(arrays, (8, 4, 4), (off, frm, tid)):
        assert a[:n * w].tobytes() == want.tobytes()
        assert (a[n * w:] == 0x5A).all()                         # nothing at or past rec_off[n]
    rc2, arrays2, runs2, *_ = run(n_runs)
    assert rc2 == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(arrays, arrays2))
    assert runs.tobytes() == runs2.tobytes()
    pile.check()


_DEBUG_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np, torch
import plan_cases as pc
from __graft_entry__ import load_package
pkg = load_package()
same = 1
with pkg.Pileup() as p:                             # one handle: its buffers grow from case to case
    for s in pc.quirk_cases() + pc.cases(pkg.SS_PLAN_CHUNK):
        a = np.frombuffer(s.data + b"\0", np.uint8).copy()
        t = torch.from_numpy(a).to("cuda:0")
        off, frm, tid, used, runs, rep = p.plan_device(t, len(s.data), s.n_ref, invalid_ok=True)
        try:
            want = pkg.pileup_plan(s.data)
            same &= int((off.cpu().numpy().view(np.uint64) == want[0]).all() and used == want[3])
        except pkg.SniperError:
            same &= int(p.last_plan_rc == pkg.SS_E_INVAL)
    rc = p.lib.ss_pileup_check(p.h)
print("CHECK", rc, "SAME", same)
"""


def test_debug_build_guard_bands():
    """The spans through the guard-band build: no byte around the handle's device
    buffers, the planner's included, changes (ss_pileup_check)."""
    lib = os.path.join(ROOT, "somatic-sniper_amd", "build", "debug", "libsniper_amd.so")
    assert os.path.exists(lib), "make -C somatic-sniper_amd debug (built by __graft_entry__.build)"
    p = subprocess.run([sys.executable, "-c", _DEBUG_CHILD, ROOT], env=dict(os.environ, SNIPER_AMD_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "CHECK 0 SAME 1" in p.stdout, (p.stdout, p.stderr[-2000:])
    assert "guard band" not in p.stderr, p.stderr[-2000:]


def _fasta(path):
    seqs, name = {}, None
    for line in open(path):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.strip())
    return {k: "".join(v).encode() for k, v in seqs.items()}


def _inflate_on_device(pkg, inf, path):
    """File bytes -> (inflated device tensor, n_ref, records_at, inflated length).  The
    header is scanned on a host inflate of the first members only."""
    import torch
    dev = torch.device("cuda", 0)
    comp, coff, ooff = pkg._pack_members(open(path, "rb").read())
    n = len(coff) - 1
    hdr = None
    for k in range(1, n + 1):
        head, status = pkg.inflate_members_cpu(comp[:int(coff[k])], coff[:k + 1], ooff[:k + 1])
        assert not status.any()
        hdr = pkg.bam_header_scan(head)
        if hdr is not None:
            break
    assert hdr is not None
    d_comp = torch.from_numpy(comp).to(dev)
    d_coff = torch.from_numpy(coff.astype(np.int64)).to(dev)
    d_ooff = torch.from_numpy(ooff.astype(np.int64)).to(dev)
    out = torch.zeros(int(ooff[-1]) + 1, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    for a in range(0, n, inf.max_members):
        k = min(inf.max_members, n - a)
        inf.inflate_device(d_comp, d_coff.data_ptr() + 8 * a, k, out, d_ooff.data_ptr() + 8 * a,
                           status.data_ptr() + 4 * a)
    inf.check()
    assert int(status.abs().sum().cpu()) == 0                   # a status word per member is all that comes back
    return out, hdr[0], hdr[1], int(ooff[-1])


@pytest.mark.parametrize("which", [0, 2], ids=["integration", "pair2_60x30"])
def test_chained_inflate_plan_pileup_score(pkg, pile, ctx, datasets, which):
    """bgzf_scan -> inflate_device -> plan_device -> count / fill -> score_device: the
    inflated bytes and the plan arrays stay on the device; scores, calls and
    positions equal score_batch over pileup_region_cpu of the host plan."""
    import torch
    dev = torch.device("cuda", 0)
    d, fa, t, n = datasets[which]
    fasta = _fasta(os.path.join(d, fa))
    host, plans = [], []
    with pkg.Inflater(device=0) as inf:
        for f in (t, n):
            path = os.path.join(d, f)
            recs, names, lens = pm.bam_records(gzip.decompress(open(path, "rb").read()))
            off, frm, tid, used = pkg.pileup_plan(recs)
            host.append((np.frombuffer(recs, np.uint8), off, frm, tid, names))
            out, n_ref, at, total = _inflate_on_device(pkg, inf, path)
            assert n_ref == len(names) and total - at == len(recs)
            d_off, d_frm, d_tid, d_used, runs, rep = pile.plan_device(out.data_ptr() + at, total - at, n_ref)
            assert d_used == used and rep == 0
            plans.append((out, out.data_ptr() + at, total - at, d_off, d_frm, runs))
    names = host[0][4]
    sites = 0
    for rt in plans[0][5]:
        for rn in plans[1][5]:
            if rt["tid"] != rn["tid"]:
                continue
            tid = int(rt["tid"])
            ref = fasta[names[tid]]
            lo, hi = max(0, int(min(rt["lo"], rn["lo"]))), int(max(rt["hi"], rn["hi"]))
            d_ref = torch.from_numpy(np.frombuffer(ref, np.uint8).copy()).to(dev)
            smp_h = [(h[0], h[1][h[3] == tid], h[2][h[3] == tid]) for h in host]
            for a in range(lo, hi, pkg.SS_PILEUP_MAX_SPAN):
                b = min(hi, a + pkg.SS_PILEUP_MAX_SPAN)
                cpu = pkg.pileup_region_cpu(smp_h[0], smp_h[1], ref, a, b)
                want_score, want_calls, _ = ctx.score_batch(cpu.batch, calls_cap=max(16, len(cpu.pos)))
                smp = [(p[1], p[2], p[3][int(r["first"]):], p[4][int(r["first"]):], int(r["n"]))
                       for p, r in zip(plans, (rt, rn))]
                ns, nt, nn = pile.count(smp[0], smp[1], d_ref, len(ref), a, b)
                assert ns == len(cpu.pos)
                i32 = dict(dtype=torch.int32, device=dev)
                pos, raw_t, raw_n = (torch.empty(max(1, ns), **i32) for _ in range(3))
                refc = torch.empty(max(1, ns), dtype=torch.uint8, device=dev)
                off_t, off_n = torch.empty(ns + 1, **i32), torch.empty(ns + 1, **i32)
                reads_t, reads_n = torch.empty(max(1, nt), **i32), torch.empty(max(1, nn), **i32)
                torch.cuda.synchronize(dev)
                pile.fill(pos, refc, raw_t, raw_n, off_t, off_n, reads_t, reads_n, ns, nt, nn)
                score = torch.full((max(1, ns),), 12345, **i32)
                calls = torch.zeros(max(16, ns) * pkg.SS_CALL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                n_calls = torch.zeros(1, **i32)
                if ns:
                    ctx.score_device(refc, off_t, off_n, reads_t, reads_n, score, calls=calls, calls_cap=max(16, ns),
                                     n_calls=n_calls, n_sites=ns)
                ctx.check()
                pile.check()
                assert (score[:ns].cpu().numpy() == want_score).all(), (tid, a)
                k = int(n_calls.cpu()[0])
                got = np.sort(calls.cpu().numpy().view(pkg.SS_CALL_DTYPE)[:k], order="site")
                assert k == len(want_calls) and (got.view("u1") == want_calls.view("u1")).all(), (tid, a)
                assert (pos[:ns].cpu().numpy() == cpu.pos).all()
                sites += ns
    assert sites > 0
