"""BGZF inflation without a GPU: the shared DEFLATE decoder on the host
(ss_inflate_members_cpu) over the member corpus, the BGZF scanner, and the
CLI's batched reader (ring + batch thread) over that decoder
(SS_BGZF_DEVICE=cpu), which must read exactly what the default reader reads."""
import gzip
import os
import re
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_corpus as ic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "somatic-sniper_amd", "bam-somaticsniper")
INDEX = os.path.join(ROOT, "somatic-sniper_amd", "ss-index")
ITEST = os.path.join(ROOT, "tests", "golden", "integration")
PAD = 192
TIMING_LINE = re.compile(r"bgzf device: (\d+) members in (\d+) batches, (\d+) re-inflated on the host")


@pytest.fixture(scope="module")
def members(tmp_path_factory):
    return (list(ic.valid_members()) + list(ic.bam_members(tmp_path_factory.mktemp("inflate_bam"))) +
            list(ic.malformed_members()))


def test_corpus_has_what_it_promises(members):
    names = [m.name for m in members]
    assert len([n for n in names if n.startswith("t-small.bam")]) == 2
    assert len([n for n in names if n.startswith("n-small.bam")]) == 3
    assert any(n.startswith("bamgen:") for n in names)
    assert {m.status for m in members} == {ic.OK, ic.E_STREAM, ic.E_SIZE, ic.E_CRC}


def test_inflate_cpu_corpus(pkg, members):
    comp, coff, ooff = ic.pack(members)
    buf = np.full(int(ooff[-1]) + 2 * PAD, 0xA5, np.uint8)
    out, status = pkg.inflate_members_cpu(comp, coff, ooff + np.uint64(PAD), buf)
    assert (buf[:PAD] == 0xA5).all() and (buf[len(buf) - PAD:] == 0xA5).all()
    for i, m in enumerate(members):
        assert status[i] == m.status, (m.name, int(status[i]))
        got = buf[PAD + int(ooff[i]):PAD + int(ooff[i + 1])].tobytes()
        if m.data is not None:
            assert got == m.data == zlib.decompress(m.comp[:-8], -15), m.name
        else:
            assert got == bytes(m.olen), m.name              # a failed member's span is zeroed
    # one member per call, each in its own padded buffer: neighbours cannot hide an overrun
    for m in members:
        c, co, oo = ic.pack([m])
        one = np.full(m.olen + 2 * PAD, 0xA5, np.uint8)
        _, st = pkg.inflate_members_cpu(c, co, oo + np.uint64(PAD), one)
        assert st[0] == m.status, m.name
        assert (one[:PAD] == 0xA5).all() and (one[PAD + m.olen:] == 0xA5).all(), m.name


def test_inflate_cpu_rejects_bad_offsets(pkg):
    m = ic.valid_members()[1]
    comp, coff, ooff = ic.pack([m, m])
    lib = pkg.load_library()
    out = np.zeros(int(ooff[-1]), np.uint8)
    st = np.zeros(2, np.uint32)

    def call(co, oo):
        return lib.ss_inflate_members_cpu(comp.ctypes.data, co.ctypes.data, 2, out.ctypes.data, oo.ctypes.data,
                                          st.ctypes.data)
    assert call(coff, ooff) == 0 and not st.any()
    assert call(coff[::-1].copy(), ooff) == pkg.SS_E_INVAL              # decreasing
    assert call(coff, ooff[::-1].copy()) == pkg.SS_E_INVAL
    assert call(np.array([0, 65536 + 9, 65536 + 9], np.uint64), ooff) == pkg.SS_E_INVAL   # longer than a member
    assert call(coff, np.array([0, 65537, 65537], np.uint64)) == pkg.SS_E_INVAL


def test_bgzf_scan(pkg):
    for name, n in (("t-small.bam", 2), ("n-small.bam", 3)):
        data = open(os.path.join(ITEST, name), "rb").read()
        span, ooff, used = pkg.bgzf_scan(data)
        assert len(span) == n and used == len(data)
        want = ic.bgzf_members(data)
        assert [data[int(a):int(b)] for a, b in span] == want
        isizes = [struct.unpack("<I", w[-4:])[0] for w in want]
        assert ooff.tolist() == np.concatenate([[0], np.cumsum(isizes)]).tolist()
        out, status = pkg.inflate_cpu(data)
        assert not status.any() and out == gzip.decompress(data)
        # cut in the middle of the second member: the scan stops at its header
        cut = int(span[1, 0]) + 3
        span2, ooff2, used2 = pkg.bgzf_scan(data[:cut])
        assert len(span2) == 1 and used2 == int(span[0, 1]) and ooff2.tolist() == ooff[:2].tolist()
        with pytest.raises(ValueError):
            pkg.inflate_cpu(data[:cut])
        # cap: stops after `cap` members
        assert len(pkg.bgzf_scan(data, cap=1)[0]) == 1
    with pytest.raises(pkg.SniperError) as e:
        pkg.bgzf_scan(b"this is not a BGZF file, not even gzip" * 4)
    assert e.value.code == pkg.SS_E_INVAL
    plain = gzip.compress(b"gzip without the BC subfield")
    with pytest.raises(pkg.SniperError):
        pkg.bgzf_scan(plain)
    assert pkg.bgzf_scan(b"")[2] == 0


# ---------------------------------------------------------------- CLI, SS_BGZF_DEVICE=cpu
def _run(args, cwd, env):
    return subprocess.run([CLI] + args, cwd=cwd, capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, **env))


def rechunk(src, dst, size):
    """The BAM at src rewritten with `size` bytes of data per BGZF member."""
    data = gzip.decompress(open(src, "rb").read())
    out = bytearray()
    for i in range(0, len(data), size):
        chunk = data[i:i + size]
        comp = ic.deflate(chunk)
        out += struct.pack("<4BI2BH2BHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, ord("B"), ord("C"), 2, 18 + len(comp) + 7)
        out += comp + ic.trailer(chunk)
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    open(dst, "wb").write(bytes(out))
    return len(range(0, len(data), size)) + 1


@pytest.fixture(scope="module")
def many_member_pair(datasets, tmp_path_factory):
    """Dataset 2 (60x / 30x) with small members: more than 40 per BAM."""
    d, fa, t, n = datasets[2]
    dst = tmp_path_factory.mktemp("many_members")
    for f in (fa, fa + ".fai"):
        if os.path.exists(os.path.join(d, f)):
            shutil.copy(os.path.join(d, f), dst / f)
    assert rechunk(os.path.join(d, t), dst / t, 9001) > 40
    assert rechunk(os.path.join(d, n), dst / n, 4999) > 40
    p = _run(["-f", fa, t, n, "warm.out"], str(dst), {"SS_PILEUP_ONLY": "1"})     # also writes the FASTA index
    assert p.returncode == 0, p.stderr[-2000:]
    return str(dst), fa, t, n


def _pileup(d, fa, t, n, name, env):
    p = _run(["-f", fa, t, n, name + ".out"], d, dict({"SS_PILEUP_ONLY": "1", "SS_DUMP_PILEUP": name, "SS_TIMING": "1"},
                                                      **env))
    assert p.returncode == 0, p.stderr[-2000:]
    path = os.path.join(d, name)
    return (open(path, "rb").read() if os.path.exists(path) else b""), p.stderr


@pytest.mark.parametrize("groups", ["1", "3"])
def test_cli_cpu_batched_reader_same_site_stream(datasets, many_member_pair, tmp_path, groups):
    """The batched reader (4 members per batch, so many batches and ring laps)
    over the host decoder: the site stream equals the default reader's, and
    every member was inflated by the new decoder (no host re-inflation)."""
    grouped = 0
    for i, (d, fa, t, n) in enumerate(list(datasets) + [many_member_pair]):
        dst = tmp_path / f"d{i}"
        dst.mkdir()
        for f in os.listdir(d):
            if f.endswith((".bam", ".fa", ".fai")):
                shutil.copy(os.path.join(d, f), dst / f)
        if groups != "1" and any(subprocess.run([INDEX, b], cwd=str(dst), capture_output=True).returncode
                                 for b in (t, n)):
            continue                                   # the unsorted pair has no index
        env = {"SS_CONTIG_GROUPS": groups}
        ref, err0 = _pileup(str(dst), fa, t, n, "plain.dump", env)
        got, err1 = _pileup(str(dst), fa, t, n, "batched.dump",
                            dict(env, SS_BGZF_DEVICE="cpu", SS_BGZF_DEVICE_BATCH="4"))
        assert got == ref, (d, groups)
        assert not TIMING_LINE.search(err0)
        lines = [tuple(int(x) for x in m.groups()) for m in TIMING_LINE.finditer(err1)]
        assert len(lines) >= 2 and all(m > 0 and b > 0 and f == 0 for m, b, f in lines), (d, lines)
        grouped += "contig groups done" in err1
        if i == len(datasets):
            assert ref and max(m for m, _, _ in lines) > 40
    assert groups == "1" or grouped >= 3


def test_cli_rejects_unknown_mode(datasets):
    d, fa, t, n = datasets[0]
    p = _run(["-f", fa, t, n, "x.out"], d, {"SS_PILEUP_ONLY": "1", "SS_BGZF_DEVICE": "gpu"})
    assert p.returncode != 0 and "SS_BGZF_DEVICE='gpu'" in p.stderr


@pytest.mark.parametrize("where", ["data", "crc", "cut"])
def test_cli_corrupt_member_same_failure(many_member_pair, tmp_path, where):
    """One corrupted member: the batched reader hands it back to the host
    inflater, so the exit code and the messages are the default reader's."""
    d, fa, t, n = many_member_pair
    for f in os.listdir(d):
        shutil.copy(os.path.join(d, f), tmp_path / f)
    data = bytearray(open(os.path.join(d, t), "rb").read())
    span = _scan(bytes(data))
    a, b = span[7]
    if where == "data":
        data[a + (b - a) // 2] ^= 0x5A
    elif where == "crc":
        data[b - 7] ^= 0x01
    else:
        del data[a + 100:]
    open(tmp_path / t, "wb").write(bytes(data))
    env = {"SS_PILEUP_ONLY": "1", "SS_CONTIG_GROUPS": "1"}
    p0 = _run(["-f", fa, t, n, "plain.out"], str(tmp_path), env)
    p1 = _run(["-f", fa, t, n, "batched.out"], str(tmp_path), dict(env, SS_BGZF_DEVICE="cpu", SS_BGZF_DEVICE_BATCH="4"))
    assert (p1.returncode, p1.stderr) == (p0.returncode, p0.stderr)
    p2 = _run(["-f", fa, t, n, "batched.out"], str(tmp_path),
              dict(env, SS_BGZF_DEVICE="cpu", SS_BGZF_DEVICE_BATCH="4", SS_TIMING="1"))
    m = TIMING_LINE.search(p2.stderr)
    if where != "cut":
        assert m and int(m.group(3)) >= 1, p2.stderr[-1500:]      # re-inflated on the host, which then failed


def _scan(data):
    """(start, end) of every member's DEFLATE data + trailer, with Python only."""
    spans, at = [], 0
    while at < len(data):
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        bsize = struct.unpack_from("<H", data, at + 16)[0]
        spans.append((at + 12 + xlen, at + bsize + 1))
        at += bsize + 1
    return spans
