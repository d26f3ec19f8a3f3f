"""BGZF inflation on the GPU (ss_inflate_members, one wave per member): the
member corpus of tests/inflate_corpus.py -- every DEFLATE block type, long
codes, far and overlapping matches, malformed and mutated members -- must give
the bytes and statuses of the host decoder and of zlib, touch nothing outside
the members' spans, and the CLI must write the same files with
SS_BGZF_DEVICE=1 as without."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_corpus as ic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "somatic-sniper_amd", "bam-somaticsniper")
INDEX = os.path.join(ROOT, "somatic-sniper_amd", "ss-index")
PAD = 192

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def members(tmp_path_factory):
    return (list(ic.valid_members()) + list(ic.bam_members(tmp_path_factory.mktemp("inflate_bam"))) +
            list(ic.malformed_members()) + ic.mutated_members(200))


@pytest.fixture(scope="module")
def cpu_result(pkg, members):
    """The host decoder's bytes and statuses for the corpus (computed once)."""
    comp, coff, ooff = ic.pack(members)
    out, status = pkg.inflate_members_cpu(comp, coff, ooff)
    out.setflags(write=False)
    status.setflags(write=False)
    return out, status


def _padded(pkg, call, members):
    """Run `call` with the members' output in the middle of a 0xA5-filled buffer."""
    comp, coff, ooff = ic.pack(members)
    buf = np.full(int(ooff[-1]) + 2 * PAD, 0xA5, np.uint8)
    out, status = call(comp, coff, ooff + np.uint64(PAD), buf)
    assert out is buf
    assert (buf[:PAD] == 0xA5).all() and (buf[len(buf) - PAD:] == 0xA5).all(), "bytes outside the spans changed"
    return buf[PAD:len(buf) - PAD], status


def _check_against(members, out, status, cpu_out, cpu_status):
    assert (status == cpu_status).all(), [(m.name, int(s), int(c)) for m, s, c in zip(members, status, cpu_status)
                                          if s != c][:10]
    assert (out == cpu_out).all()
    at = 0
    for m, s in zip(members, status):
        if m.status != ic.ANY:
            assert s == m.status, m.name
        if m.data is not None:
            assert out[at:at + m.olen].tobytes() == m.data, m.name     # zlib's bytes
        at += m.olen


def test_corpus_one_batch(pkg, members, cpu_result):
    with pkg.Inflater(max_members=len(members)) as inf:
        out, status = _padded(pkg, inf.inflate_members, members)
        inf.check()
    _check_against(members, out, status, *cpu_result)


def test_corpus_one_member_per_call(pkg, members, cpu_result):
    cpu_out, cpu_status = cpu_result
    at = 0
    with pkg.Inflater(max_members=1) as inf:
        for i, m in enumerate(members):
            out, status = _padded(pkg, inf.inflate_members, [m])
            assert status[0] == cpu_status[i], m.name
            assert (out == cpu_out[at:at + m.olen]).all(), m.name
            at += m.olen
        inf.check()


def test_inflate_file_bytes(pkg, tmp_path):
    import gzip
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bamgen
    bamgen.make_pair(str(tmp_path), seed=12, lengths=(3000,), depth_t=50, depth_n=8)
    with pkg.Inflater() as inf:
        for path in (os.path.join(ROOT, "tests", "golden", "integration", "t-small.bam"),
                     os.path.join(ROOT, "tests", "golden", "integration", "n-small.bam"),
                     str(tmp_path / "tumor.bam")):
            data = open(path, "rb").read()
            got, status = inf.inflate(data)
            assert not status.any() and got == gzip.decompress(data)
            assert (got, status.tolist()) == (lambda r: (r[0], r[1].tolist()))(pkg.inflate_cpu(data))


_DEBUG_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import inflate_corpus as ic
from __graft_entry__ import load_package
pkg = load_package()
members = list(ic.valid_members()) + list(ic.malformed_members()) + ic.mutated_members(200)
comp, coff, ooff = ic.pack(members)
cpu_out, cpu_status = pkg.inflate_members_cpu(comp, coff, ooff)
with pkg.Inflater(max_members=64) as inf:          # several calls, buffers grow in between
    out, status = inf.inflate_members(comp, coff, ooff)
    rc = inf.lib.ss_inflate_check(inf.h)
print("CHECK", rc, "SAME", int((out == cpu_out).all() and (status == cpu_status).all()))
"""


def test_debug_build_guard_bands():
    """The corpus, malformed members included, through the guard-band build:
    every member yields a status, and no byte around the handle's device
    buffers changes (ss_inflate_check)."""
    lib = os.path.join(ROOT, "somatic-sniper_amd", "build", "debug", "libsniper_amd.so")
    assert os.path.exists(lib), "make -C somatic-sniper_amd debug (built by __graft_entry__.build)"
    p = subprocess.run([sys.executable, "-c", _DEBUG_CHILD, ROOT], env=dict(os.environ, SNIPER_AMD_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    assert "CHECK 0 SAME 1" in p.stdout, (p.stdout, p.stderr[-2000:])
    assert "guard band" not in p.stderr, p.stderr[-2000:]


def test_shuffled_batch_and_handle_reuse(pkg, members, cpu_result):
    """300 members of varied sizes in shuffled order; one handle, three calls,
    the last with a single member."""
    import random
    rng = random.Random(5)
    valid = [m for m in members if m.status == ic.OK]
    small = [m for m in valid if m.olen < 8000]
    batch = [rng.choice(valid) for _ in range(12)] + [rng.choice(small) for _ in range(288)]
    rng.shuffle(batch)
    comp, coff, ooff = ic.pack(batch)
    want = b"".join(m.data for m in batch)
    with pkg.Inflater(max_members=300) as inf:
        for sub in (batch, batch[100:163], batch[7:8]):
            c, co, oo = ic.pack(sub)
            out, status = inf.inflate_members(c, co, oo)
            assert not status.any()
            assert out.tobytes() == b"".join(m.data for m in sub)
        # more members than the handle was made for: the call fails, nothing is touched
        assert inf.lib.ss_inflate_members_host(inf.h, comp.ctypes.data, coff.ctypes.data, 301, None,
                                               ooff.ctypes.data, None) == pkg.SS_E_INVAL
    assert len(want) == int(ooff[-1])


def test_device_call_on_user_stream(pkg, members, cpu_result):
    import torch
    cpu_out, cpu_status = cpu_result
    comp, coff, ooff = ic.pack(members)
    dev = torch.device("cuda", 0)
    d_comp = torch.from_numpy(comp.copy()).to(dev)
    d_coff = torch.from_numpy(coff.astype(np.int64)).to(dev)
    d_ooff = torch.from_numpy((ooff + np.uint64(PAD)).astype(np.int64)).to(dev)
    d_out = torch.full((int(ooff[-1]) + 2 * PAD,), 0xA5, dtype=torch.uint8, device=dev)
    d_status = torch.full((len(members),), 99, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    with pkg.Inflater(max_members=len(members)) as inf:
        inf.inflate_device(d_comp, d_coff, len(members), d_out, d_ooff, d_status, stream=stream)
        stream.synchronize()
        host_out, host_status = inf.inflate_members(comp, coff, ooff)
    out = d_out.cpu().numpy()
    assert (out[:PAD] == 0xA5).all() and (out[len(out) - PAD:] == 0xA5).all()
    assert (out[PAD:len(out) - PAD] == host_out).all() and (host_out == cpu_out).all()
    status = d_status.cpu().numpy().astype(np.uint32)
    assert (status == host_status).all() and (status == cpu_status).all()


# ---------------------------------------------------------------- CLI
def _cli(d, args, env):
    return subprocess.run([CLI] + args, cwd=d, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, **env))


TIMING_LINE = re.compile(r"bgzf device: (\d+) members in (\d+) batches, (\d+) re-inflated on the host")


def _device_lines(stderr):
    got = [tuple(int(x) for x in m.groups()) for m in TIMING_LINE.finditer(stderr)]
    assert got, stderr[-2000:]
    return got


@pytest.mark.parametrize("groups", ["1", "2"])
@pytest.mark.parametrize("fmt", ["classic", "vcf"])
def test_cli_device_inflation_same_files(datasets, tmp_path, fmt, groups):
    """SS_BGZF_DEVICE=1 (8 members per batch): byte-identical output files,
    streaming ("1") and with two contig groups; every member inflated on the GPU."""
    import shutil
    grouped = 0
    for i, (d, fa, t, n) in enumerate(datasets):
        dst = tmp_path / f"{fmt}{i}"
        dst.mkdir()
        for f in os.listdir(d):
            if f.endswith((".bam", ".fa", ".fai")):
                shutil.copy(os.path.join(d, f), dst / f)
        if groups != "1" and any(subprocess.run([INDEX, b], cwd=str(dst), capture_output=True).returncode
                                 for b in (t, n)):
            continue                                   # the unsorted pair has no index
        base = {"SS_CONTIG_GROUPS": groups, "SS_TIMING": "1"}
        p0 = _cli(str(dst), ["-F", fmt, "-f", fa, t, n, "plain.out"], base)
        p1 = _cli(str(dst), ["-F", fmt, "-f", fa, t, n, "dev.out"],
                  dict(base, SS_BGZF_DEVICE="1", SS_BGZF_DEVICE_BATCH="8"))
        assert p0.returncode == 0 and p1.returncode == 0, (d, p0.stderr[-1500:], p1.stderr[-1500:])
        assert (dst / "plain.out").read_bytes() == (dst / "dev.out").read_bytes(), (d, groups)
        assert not TIMING_LINE.search(p0.stderr)
        lines = _device_lines(p1.stderr)
        assert all(m > 0 and b > 0 and f == 0 for m, b, f in lines), lines
        grouped += "contig groups done" in p1.stderr
    assert groups == "1" or grouped >= 3
