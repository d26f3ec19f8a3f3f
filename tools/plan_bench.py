#!/usr/bin/env python3
"""The planner on the GPU against what a caller does without it.

    python tools/plan_bench.py WORKDIR [--length 2500000] [--out JSON]

WORKDIR gets a tools/bamsim.py pair (60x / 30x, --length bases in 4 contigs;
reused when it is already there).  Method of tools/pileup_bench.py: 3 warm-up
and --calls timed calls, medians, the two sides in alternating rounds of one
process.  Reported per sample:

  plan_device   ss_pileup_plan_device over the inflated records in device
                memory: HIP events around the call, the wall clock, and the
                call's own phases (guess + walk, stitch, emit + plan: each ends
                where the call waits for the stream anyway); bytes/s, records/s,
                n_repaired
  today         the same result without it: D2H of the same inflated bytes into
                pinned memory, ss_pileup_plan on one host core, H2D of the three
                arrays; wall clock, each part and the sum
  ratio         today / plan_device (wall clock), per round

and for the pair, in sites/s, wall clock:

  chain_device  packed BGZF members H2D -> inflate_device -> plan_device ->
                count / fill per run and region -> score_device; scores and
                emitted calls fetched
  chain_records section 13's chain: the host-planned records H2D -> pileup ->
                score_device (the host inflate and plan are not in its time)
"""
import argparse
import ctypes as C
import gzip
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
REGION = 1 << 20


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("work")
    ap.add_argument("--length", type=int, default=2_500_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    import pileup_bench as pb
    pkg = load_package()
    lib = pkg.load_library()
    os.makedirs(a.work, exist_ok=True)
    pb.make_pair(a.work, a.length)
    dev = torch.device("cuda", 0)
    refs = pb.fasta(os.path.join(a.work, "ref.fa"))
    res = {"length": a.length, "depth": [60, 30], "chunk": pkg.SS_PLAN_CHUNK, "samples": {}}

    samples = []
    stream = torch.cuda.Stream(dev)
    with pkg.Pileup(device=0) as pile:
        for label in ("tumor", "normal"):
            path = os.path.join(a.work, label + ".bam")
            data = np.frombuffer(bytearray(gzip.decompress(open(path, "rb").read())), np.uint8)
            n_ref, at = pkg.bam_header_scan(data[:1 << 20])
            recs = data[at:]
            d_all = torch.from_numpy(data).to(dev)
            addr, nb = d_all.data_ptr() + at, recs.size
            off, frm, tid, used = pkg.pileup_plan(recs)
            n_records = len(pkg.pileup_split_cpu(recs, n_ref)[0])
            pinned = torch.empty(nb, dtype=torch.uint8).pin_memory()
            ev_ms, wall_ms, phases, today, ratio = [], [], [], [], []
            rep = None
            for it in range(3 + a.calls):
                # the device planner
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                e0.record(stream)
                d_off, d_frm, d_tid, d_used, runs, rep = pile.plan_device(addr, nb, n_ref, stream=stream)
                e1.record(stream)
                stream.synchronize()
                t1 = time.perf_counter()
                ph = (C.c_double * 3)()
                lib.ss__plan_phase_ms(pile.h, ph)
                assert d_used == used and len(d_off) == len(off)
                # without it: bytes out, host plan, arrays in
                torch.cuda.synchronize(dev)
                t2 = time.perf_counter()
                pinned.copy_(d_all[at:])
                torch.cuda.synchronize(dev)
                t3 = time.perf_counter()
                h_off, h_frm, h_tid, h_used = pkg.pileup_plan(pinned.numpy())
                t4 = time.perf_counter()
                up = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
                      for x in (h_off, h_frm, h_tid)]
                torch.cuda.synchronize(dev)
                t5 = time.perf_counter()
                if it == 0:
                    assert (d_off.cpu().numpy().view(np.uint64) == h_off).all()
                    assert (d_frm.cpu().numpy() == h_frm).all() and (d_tid.cpu().numpy() == h_tid).all()
                if it >= 3:
                    ev_ms.append(e0.elapsed_time(e1))
                    wall_ms.append((t1 - t0) * 1e3)
                    phases.append(list(ph))
                    today.append([(t3 - t2) * 1e3, (t4 - t3) * 1e3, (t5 - t4) * 1e3, (t5 - t2) * 1e3])
                    ratio.append((t5 - t2) / (t1 - t0))
                del up
            pile.check()
            med = statistics.median(wall_ms) * 1e-3
            res["samples"][label] = {
                "record_bytes": int(nb), "records": n_records, "records_kept": int(len(off)), "runs": int(len(runs)),
                "n_repaired": rep,
                "plan_device_event_ms": spread(ev_ms), "plan_device_wall_ms": spread(wall_ms),
                "phase_ms": {k: spread([p[i] for p in phases])
                             for i, k in enumerate(("guess_walk", "stitch", "emit_plan"))},
                "bytes_per_s": nb / med, "records_per_s": n_records / med,
                "today_ms": {k: spread([t[i] for t in today])
                             for i, k in enumerate(("d2h_bytes", "host_plan", "h2d_arrays", "sum"))},
                "today_over_plan_device": spread(ratio)}
            print(label, json.dumps(res["samples"][label]), file=sys.stderr, flush=True)
            comp, coff, ooff = pkg._pack_members(open(path, "rb").read())
            samples.append(dict(recs=recs, off=off, frm=frm, tid=tid, n_ref=n_ref, at=at, comp=comp, coff=coff,
                                ooff=ooff, total=data.size))
            del d_all, pinned

        import struct
        hdr = gzip.decompress(open(os.path.join(a.work, "tumor.bam"), "rb").read())[: samples[0]["at"]]
        names, p = [], 12 + struct.unpack_from("<i", hdr, 4)[0]
        for _ in range(samples[0]["n_ref"]):
            l_name, = struct.unpack_from("<i", hdr, p)
            names.append(hdr[p + 4:p + 4 + l_name - 1].decode())
            p += 8 + l_name
        d_refs = {n: torch.from_numpy(refs[n].copy()).to(dev) for n in names}

        def score(ctx, d_ref, off_t, off_n, reads_t, reads_n, ns):
            cap = max(16, ns // 64)
            sc = torch.empty(max(1, ns), dtype=torch.int32, device=dev)
            calls = torch.zeros(cap * pkg.SS_CALL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            n_calls = torch.zeros(1, dtype=torch.int32, device=dev)
            ctx.score_device(d_ref, off_t, off_n, reads_t, reads_n, sc, calls=calls, calls_cap=cap, n_calls=n_calls,
                             n_sites=ns)
            k = int(n_calls.cpu()[0])
            assert k <= cap
            return sc[:ns].cpu().numpy(), len(calls[:k * pkg.SS_CALL_DTYPE.itemsize].cpu().numpy())

        def chain_device(ctx, inf):
            plans = []
            for s in samples:
                n = len(s["coff"]) - 1
                d_comp = torch.from_numpy(s["comp"]).to(dev)
                d_coff = torch.from_numpy(s["coff"].view(np.int64)).to(dev)
                d_ooff = torch.from_numpy(s["ooff"].view(np.int64)).to(dev)
                out = torch.empty(s["total"] + 1, dtype=torch.uint8, device=dev)
                status = torch.zeros(n, dtype=torch.int32, device=dev)
                torch.cuda.synchronize(dev)
                for b in range(0, n, inf.max_members):
                    inf.inflate_device(d_comp, d_coff.data_ptr() + 8 * b, min(inf.max_members, n - b), out,
                                       d_ooff.data_ptr() + 8 * b, status.data_ptr() + 4 * b)
                inf.check()
                nb = s["total"] - s["at"]
                d_off, d_frm, d_tid, used, runs, rep = pile.plan_device(out.data_ptr() + s["at"], nb, s["n_ref"])
                plans.append((out, out.data_ptr() + s["at"], nb, d_off, d_frm, runs))
            scores, emitted, sites = [], 0, 0
            for rt in plans[0][5]:
                for rn in plans[1][5]:
                    if rt["tid"] != rn["tid"]:
                        continue
                    name = names[int(rt["tid"])]
                    lo, hi = max(0, int(min(rt["lo"], rn["lo"]))), int(max(rt["hi"], rn["hi"]))
                    smp = [(p[1], p[2], p[3][int(r["first"]):], p[4][int(r["first"]):], int(r["n"]))
                           for p, r in zip(plans, (rt, rn))]
                    for x in range(lo, hi, REGION):
                        y = min(hi, x + REGION)
                        ns, nt, nn = pile.count(smp[0], smp[1], d_refs[name], refs[name].size, x, y)
                        i32 = dict(dtype=torch.int32, device=dev)
                        o = [torch.empty(max(1, ns), **i32), torch.empty(max(1, ns), dtype=torch.uint8, device=dev),
                             torch.empty(max(1, ns), **i32), torch.empty(max(1, ns), **i32),
                             torch.empty(ns + 1, **i32), torch.empty(ns + 1, **i32), torch.empty(max(1, nt), **i32),
                             torch.empty(max(1, nn), **i32)]
                        torch.cuda.synchronize(dev)
                        pile.fill(*o, ns, nt, nn)
                        sc, k = score(ctx, o[1], o[4], o[5], o[6], o[7], ns)
                        scores.append(sc)
                        emitted += k
                        sites += ns
            return np.concatenate(scores), emitted, sites

        regions = []
        for tid, name in enumerate(names):
            m = [s["tid"] == tid for s in samples]
            if not m[0].any() or not m[1].any():
                continue
            top = int(max(samples[0]["frm"][m[0]].max(), samples[1]["frm"][m[1]].max())) + 4096
            for lo in range(0, top, REGION):
                regions.append((name, tuple((s["recs"], s["off"][k], s["frm"][k]) for s, k in zip(samples, m)),
                                lo, min(top, lo + REGION)))

        def chain_records(ctx):
            scores, emitted, sites = [], 0, 0
            for name, (st, sn), lo, hi in regions:
                d = pile.region_device(st, sn, refs[name], lo, hi)
                sc, k = score(ctx, d["ref"], d["off_tumor"], d["off_normal"], d["reads_tumor"], d["reads_normal"],
                              d["n_sites"])
                scores.append(sc)
                emitted += k
                sites += d["n_sites"]
            return np.concatenate(scores), emitted, sites

        with pkg.Context(pkg.Params.default(), device=0) as ctx, pkg.Inflater(device=0) as inf:
            dev_rate, rec_rate = [], []
            for r in range(a.rounds + 1):                # round 0 warms both chains
                t0 = time.perf_counter()
                s_dev, k_dev, n_dev = chain_device(ctx, inf)
                t1 = time.perf_counter()
                s_rec, k_rec, n_rec = chain_records(ctx)
                t2 = time.perf_counter()
                ctx.check()
                pile.check()
                assert n_dev == n_rec and k_dev == k_rec and (s_dev == s_rec).all()
                if r:
                    dev_rate.append(n_dev / (t1 - t0))
                    rec_rate.append(n_rec / (t2 - t1))
            res["sites"] = int(n_dev)
            res["chain_device_sites_per_s"] = spread(dev_rate)
            res["chain_records_sites_per_s"] = spread(rec_rate)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
