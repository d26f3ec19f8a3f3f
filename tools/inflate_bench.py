#!/usr/bin/env python3
"""Rates of the BGZF inflation paths and their end-to-end effect on the CLI.

    python tools/inflate_bench.py WORKDIR [--length 10000000] [--parent-cli PATH] [--out JSON]

WORKDIR gets a tools/bamsim.py pair (60x / 30x, --length bases; reused when it
is already there) and its indexes.  Reported:

  kernel    one ss_inflate_members_device launch of up to 4096 members of the
            tumor BAM, HIP events around the launch, warm-up first, median of
            --launches launches; GB/s of uncompressed output
  host      the same members through libdeflate (zlib when it is missing) on
            16 threads, through the shared decoder on one thread
            (ss_inflate_members_cpu), and through ss_inflate_members_host
            (copies included)
  cli       wall and user+sys seconds of bam-somaticsniper with and without
            SS_BGZF_DEVICE=1, streaming and with 4 contig groups, and of
            --parent-cli (the previous commit's build) on the same files; the
            variants take turns within every round, --runs rounds, median and
            range
"""
import argparse
import ctypes
import json
import os
import resource
import statistics
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "somatic-sniper_amd", "bam-somaticsniper")
INDEX = os.path.join(ROOT, "somatic-sniper_amd", "ss-index")


def make_pair(work, length):
    if not os.path.exists(os.path.join(work, "normal.bam")):
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bamsim.py"), work, "--length", str(length),
                        "--contigs", "4"], check=True)
    for b in ("tumor.bam", "normal.bam"):
        if not os.path.exists(os.path.join(work, b + ".bai")):
            subprocess.run([INDEX, b], cwd=work, check=True)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def kernel_and_host(pkg, work, launches, n_members):
    import torch
    data = np.fromfile(os.path.join(work, "tumor.bam"), np.uint8)
    span, ooff, _ = pkg.bgzf_scan(data)
    n = min(n_members, len(span))
    span, ooff = span[:n], ooff[:n + 1]
    lens = span[:, 1] - span[:, 0]
    coff = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=coff[1:])
    comp = np.empty(int(coff[-1]), np.uint8)
    for i, (b, e) in enumerate(span):
        comp[int(coff[i]):int(coff[i + 1])] = data[int(b):int(e)]
    out_bytes = int(ooff[-1])
    res = {"members": n, "compressed_bytes": int(coff[-1]), "output_bytes": out_bytes}

    dev = torch.device("cuda", 0)
    d_comp = torch.from_numpy(comp).to(dev)
    d_coff = torch.from_numpy(coff.astype(np.int64)).to(dev)
    d_ooff = torch.from_numpy(ooff.astype(np.int64)).to(dev)
    d_out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
    d_status = torch.empty(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    with pkg.Inflater(max_members=n) as inf:
        ms = []
        for it in range(3 + launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            inf.inflate_device(d_comp, d_coff, n, d_out, d_ooff, d_status, stream=stream)
            e1.record(stream)
            stream.synchronize()
            if it >= 3:
                ms.append(e0.elapsed_time(e1))
        assert not d_status.cpu().numpy().any(), "a member failed on the device"
        want = zlib.crc32(d_out.cpu().numpy().tobytes())
        res["kernel_ms"] = spread(ms)
        res["kernel_GBps"] = out_bytes / (statistics.median(ms) * 1e-3) / 1e9
        # the host call: pageable numpy arrays in, copies both ways included
        ts = []
        for it in range(1 + 5):
            t0 = time.perf_counter()
            out, status = inf.inflate_members(comp, coff, ooff)
            if it:
                ts.append(time.perf_counter() - t0)
        assert not status.any() and zlib.crc32(out.tobytes()) == want
        res["host_call_GBps"] = out_bytes / statistics.median(ts) / 1e9

    # host inflaters, 16 threads
    members = [comp[int(coff[i]):int(coff[i + 1]) - 8].tobytes() for i in range(n)]
    sizes = np.diff(ooff).astype(np.int64)
    try:
        ld = ctypes.CDLL("libdeflate.so.0")
        ld.libdeflate_alloc_decompressor.restype = ctypes.c_void_p
        ld.libdeflate_deflate_decompress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                                     ctypes.c_size_t, ctypes.c_void_p]
        ld.libdeflate_free_decompressor.argtypes = [ctypes.c_void_p]
        name = "libdeflate"

        def work_fn(rng):
            d = ld.libdeflate_alloc_decompressor()
            buf = ctypes.create_string_buffer(65536)
            got = ctypes.c_size_t()
            for i in rng:
                rc = ld.libdeflate_deflate_decompress(d, members[i], len(members[i]), buf, 65536, ctypes.byref(got))
                assert rc == 0 and got.value == sizes[i]
            ld.libdeflate_free_decompressor(d)
    except OSError:
        name = "zlib"

        def work_fn(rng):
            for i in rng:
                assert len(zlib.decompress(members[i], -15)) == sizes[i]
    ts = []
    with ThreadPoolExecutor(16) as ex:
        for it in range(1 + 5):
            t0 = time.perf_counter()
            list(ex.map(work_fn, [range(k, n, 16) for k in range(16)]))
            if it:
                ts.append(time.perf_counter() - t0)
    res["host_16_threads"] = {"library": name, "GBps": out_bytes / statistics.median(ts) / 1e9}
    t0 = time.perf_counter()
    out, status = pkg.inflate_members_cpu(comp, coff, ooff)
    res["shared_decoder_1_thread_GBps"] = out_bytes / (time.perf_counter() - t0) / 1e9
    assert not status.any() and zlib.crc32(out.tobytes()) == want
    return res


def cli_runs(work, parent_cli, runs):
    variants = [("this", CLI, "1", {}), ("this+device", CLI, "1", {"SS_BGZF_DEVICE": "1"}),
                ("this, 4 groups", CLI, "4", {}), ("this+device, 4 groups", CLI, "4", {"SS_BGZF_DEVICE": "1"})]
    if parent_cli:
        variants += [("parent", parent_cli, "1", {}), ("parent, 4 groups", parent_cli, "4", {})]
    wall = {v[0]: [] for v in variants}
    cpu = {v[0]: [] for v in variants}
    outs = {}
    for r in range(runs + 1):                      # round 0 warms the page cache and the table cache
        for name, cli, groups, extra in variants:
            out = f"bench_{abs(hash(name)) % 10000}.out"
            env = dict(os.environ, SS_CONTIG_GROUPS=groups, **extra)
            r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
            t0 = time.perf_counter()
            p = subprocess.run([cli, "-f", "ref.fa", "tumor.bam", "normal.bam", out], cwd=work, env=env,
                               capture_output=True, text=True)
            dt = time.perf_counter() - t0
            r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
            assert p.returncode == 0, (name, p.stderr[-2000:])
            outs[name] = zlib.crc32(open(os.path.join(work, out), "rb").read())
            if r:
                wall[name].append(dt)
                cpu[name].append(r1.ru_utime + r1.ru_stime - r0.ru_utime - r0.ru_stime)
    assert len(set(outs.values())) == 1, ("outputs differ", outs)
    return {name: {"wall_s": spread(wall[name]), "cpu_s": spread(cpu[name])} for name in wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("work")
    ap.add_argument("--length", type=int, default=10_000_000)
    ap.add_argument("--parent-cli")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--members", type=int, default=4096)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from __graft_entry__ import load_package
    pkg = load_package()
    os.makedirs(a.work, exist_ok=True)
    make_pair(a.work, a.length)
    res = {"length": a.length, "depth": [60, 30],
           "bam_bytes": [os.path.getsize(os.path.join(a.work, b)) for b in ("tumor.bam", "normal.bam")]}
    res["rates"] = kernel_and_host(pkg, a.work, a.launches, a.members)
    print(json.dumps(res["rates"]), file=sys.stderr, flush=True)
    if not a.skip_cli:
        res["cli"] = cli_runs(a.work, a.parent_cli, a.runs)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
