#!/usr/bin/env python3
"""Rates of the record pileup on the GPU and of the chained records -> score path.

    python tools/pileup_bench.py WORKDIR [--length 2500000] [--out JSON]

WORKDIR gets a tools/bamsim.py pair (60x / 30x, --length bases in 4 contigs;
reused when it is already there).  Both BAMs are inflated on the host (gzip)
and planned (ss_pileup_plan); every contig is then built in regions of 2^20
positions.  Reported:

  kernels   ss_pileup_count_device (index + scan + count + tile scan) and
            ss_pileup_fill_device, HIP events on one stream, 3 warm-up and
            --calls timed calls per region, medians summed over the regions;
            entries/s, and the algorithmic bytes (the record bytes once, 4 B
            per packed entry, 21 B per site) over the time against the HBM peak
  chained   records H2D -> pileup -> ss_score_batch_device with the batch
            never leaving the device, scores and emitted calls fetched, wall
            clock, in sites/s; next to
            ss_score_batch_host over the same sites (the CPU twin's batch),
            alternating rounds in one process
  cpu       ss_pileup_region_cpu on one thread over the same regions
"""
import argparse
import gzip
import json
import os
import statistics
import struct
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0         # MI355X: HBM3E 8.0 TB/s spec
REGION = 1 << 20


def make_pair(work, length):
    if not os.path.exists(os.path.join(work, "normal.bam")):
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bamsim.py"), work, "--length", str(length),
                        "--contigs", "4"], check=True)


def records(path):
    """(record bytes after the header as u8, contig names, lengths)."""
    data = gzip.decompress(open(path, "rb").read())
    assert data[:4] == b"BAM\1"
    at = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    names, lens = [], []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, at)
        names.append(data[at + 4:at + 4 + l_name - 1].decode())
        lens.append(struct.unpack_from("<i", data, at + 4 + l_name)[0])
        at += 8 + l_name
    return np.frombuffer(bytearray(data), np.uint8)[at:], names, lens       # writable: uploads take it as it is


def fasta(path):
    seqs, name = {}, None
    for line in open(path):
        if line.startswith(">"):
            name = line[1:].split()[0]
            seqs[name] = []
        else:
            seqs[name].append(line.strip())
    return {k: np.frombuffer("".join(v).encode(), np.uint8) for k, v in seqs.items()}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("work")
    ap.add_argument("--length", type=int, default=2_500_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    os.makedirs(a.work, exist_ok=True)
    make_pair(a.work, a.length)
    dev = torch.device("cuda", 0)

    bt, names, lens = records(os.path.join(a.work, "tumor.bam"))
    bn, _, _ = records(os.path.join(a.work, "normal.bam"))
    t0 = time.perf_counter()
    ot, ft, tt, used_t = pkg.pileup_plan(bt)
    on, fn, tn, used_n = pkg.pileup_plan(bn)
    plan_s = time.perf_counter() - t0
    assert used_t == bt.size and used_n == bn.size
    refs = fasta(os.path.join(a.work, "ref.fa"))

    # the regions: every contig in pieces of 2^20 positions; a region takes the
    # contig's records whose `from` lies before its end (earlier ones are cut by
    # the running-maximum search on the device)
    regions = []
    for tid, name in enumerate(names):
        mt, mn = tt == tid, tn == tid
        if not mt.any() or not mn.any():
            continue
        top = int(max(ft[mt].max(), fn[mn].max())) + 4096
        for lo in range(0, top, REGION):
            regions.append((name, (bt, ot[mt], ft[mt]), (bn, on[mn], fn[mn]), refs[name], lo, min(top, lo + REGION)))

    res = {"length": a.length, "depth": [60, 30], "contigs": len(names), "regions": len(regions),
           "record_bytes": [int(bt.size), int(bn.size)], "records_kept": [int(len(ot)), int(len(on))],
           "plan_seconds": plan_s}

    # ---- the CPU twin (one thread), and its batches for the comparisons below
    t0 = time.perf_counter()
    twins = [pkg.pileup_region_cpu(st, sn, ref, lo, hi) for _, st, sn, ref, lo, hi in regions]
    cpu_s = time.perf_counter() - t0
    n_sites = sum(len(r.pos) for r in twins)
    n_entries = sum(len(r.batch.reads_tumor) + len(r.batch.reads_normal) for r in twins)
    res.update(sites=n_sites, entries=n_entries)
    res["cpu_1_thread"] = {"seconds": cpu_s, "entries_per_s": n_entries / cpu_s, "sites_per_s": n_sites / cpu_s}

    # ---- the kernels, HIP events
    stream = torch.cuda.Stream(dev)
    count_ms = fill_ms = both_ms = 0.0
    alg_bytes = 0
    with pkg.Pileup(device=0) as pile:
        for (name, st, sn, ref, lo, hi), twin in zip(regions, twins):
            smp = []
            for data, off, frm in (st, sn):
                b0, b1 = int(off.min()), int(off.max())
                b1 = b1 + 4 + int.from_bytes(data[b1:b1 + 4].tobytes(), "little")
                smp.append((torch.from_numpy(data[b0:b1].copy()).to(dev), b1 - b0,
                            torch.from_numpy((off - np.uint64(b0)).astype(np.int64)).to(dev),
                            torch.from_numpy(frm.copy()).to(dev), len(off)))
                alg_bytes += b1 - b0
            d_ref = torch.from_numpy(ref.copy()).to(dev)
            ns, nt, nn = len(twin.pos), len(twin.batch.reads_tumor), len(twin.batch.reads_normal)
            alg_bytes += 4 * (nt + nn) + 21 * ns
            i32 = dict(dtype=torch.int32, device=dev)
            out = [torch.empty(max(1, ns), **i32), torch.empty(max(1, ns), dtype=torch.uint8, device=dev),
                   torch.empty(max(1, ns), **i32), torch.empty(max(1, ns), **i32), torch.empty(ns + 1, **i32),
                   torch.empty(ns + 1, **i32), torch.empty(max(1, nt), **i32), torch.empty(max(1, nn), **i32)]
            torch.cuda.synchronize(dev)
            c_ms, f_ms, b_ms = [], [], []
            for it in range(3 + a.calls):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record(stream)
                got = pile.count(smp[0], smp[1], d_ref, ref.size, lo, hi, stream=stream)
                e[1].record(stream)
                pile.fill(*out, ns, nt, nn, stream=stream)
                e[2].record(stream)
                stream.synchronize()
                assert got == (ns, nt, nn), (name, got, (ns, nt, nn))
                if it >= 3:
                    c_ms.append(e[0].elapsed_time(e[1]))
                    f_ms.append(e[1].elapsed_time(e[2]))
                    b_ms.append(e[0].elapsed_time(e[2]))
            pile.check()
            assert (out[6][:nt].cpu().numpy().view(np.uint32) == twin.batch.reads_tumor).all()
            assert (out[4].cpu().numpy().view(np.uint32) == twin.batch.off_tumor).all()
            count_ms += statistics.median(c_ms)
            fill_ms += statistics.median(f_ms)
            both_ms += statistics.median(b_ms)
        res["kernels"] = {
            "count_ms": count_ms, "fill_ms": fill_ms, "count_and_fill_ms": both_ms,
            "entries_per_s": n_entries / (both_ms * 1e-3), "sites_per_s": n_sites / (both_ms * 1e-3),
            "algorithmic_bytes": alg_bytes, "algorithmic_GBps": alg_bytes / (both_ms * 1e-3) / 1e9,
            "share_of_hbm_peak": alg_bytes / (both_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            "count_entries_per_s": n_entries / (count_ms * 1e-3), "fill_entries_per_s": n_entries / (fill_ms * 1e-3)}
        print(json.dumps(res["kernels"]), file=sys.stderr, flush=True)

        # ---- chained (records H2D -> pileup -> score on the device) against
        # ss_score_batch_host over the CPU twin's batches, alternating rounds
        with pkg.Context(pkg.Params.default(), device=0) as ctx:
            chained, hosted = [], []
            want = None
            for r in range(a.rounds + 1):            # round 0 warms both paths
                t0 = time.perf_counter()
                scores, n_emitted = [], 0
                for name, st, sn, ref, lo, hi in regions:
                    d = pile.region_device(st, sn, ref, lo, hi)
                    ns = d["n_sites"]
                    cap = max(16, ns // 64)              # the emitted calls too, sized as score_batch sizes them
                    score = torch.empty(max(1, ns), dtype=torch.int32, device=dev)
                    calls = torch.zeros(cap * pkg.SS_CALL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                    n_calls = torch.zeros(1, dtype=torch.int32, device=dev)
                    ctx.score_device(d["ref"], d["off_tumor"], d["off_normal"], d["reads_tumor"], d["reads_normal"],
                                     score, calls=calls, calls_cap=cap, n_calls=n_calls, n_sites=ns)
                    scores.append(score[:ns].cpu().numpy())
                    k = int(n_calls.cpu()[0])
                    assert k <= cap, (name, k, cap)
                    n_emitted += len(calls[:k * pkg.SS_CALL_DTYPE.itemsize].cpu().numpy())
                ctx.check()
                t1 = time.perf_counter()
                host = [ctx.score_batch(tw.batch) for tw in twins]
                t2 = time.perf_counter()
                host_scores = [h[0] for h in host]
                if want is None:
                    want = np.concatenate(host_scores)
                assert (np.concatenate(scores) == want).all() and (np.concatenate(host_scores) == want).all()
                assert n_emitted == sum(len(h[1]) for h in host) * pkg.SS_CALL_DTYPE.itemsize
                if r:
                    chained.append(n_sites / (t1 - t0))
                    hosted.append(n_sites / (t2 - t1))
            res["chained_sites_per_s"] = spread(chained)
            res["score_batch_host_sites_per_s"] = spread(hosted)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
