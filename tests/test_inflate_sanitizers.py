"""Sanitizer runs of the BGZF inflation host code (CPU only, nothing here
touches a GPU or loads a sanitizer runtime into Python).

`make -C somatic-sniper_amd sanitize` builds tests/native/inflate_driver.c -- a
stand-alone program over the shared DEFLATE decoder (csrc/ss_inflate_core.h,
the code the GPU kernel runs) -- with ASan+UBSan; it decodes the whole member
corpus, malformed and mutated members included, each member in heap blocks of
exactly its spans.  The ASan and TSan builds of the CLI run the batched reader
(ring, I/O thread, batch thread) with SS_BGZF_DEVICE=cpu."""
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inflate_corpus as ic  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "somatic-sniper_amd", "build", "san")
INDEX = os.path.join(ROOT, "somatic-sniper_amd", "ss-index")
ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1:abort_on_error=0",
       "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
       "TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1"}
TIMING_LINE = re.compile(r"bgzf device: (\d+) members in (\d+) batches, (\d+) re-inflated on the host")


@pytest.fixture(scope="module")
def san_build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "somatic-sniper_amd"), "sanitize"], check=True,
                   capture_output=True, timeout=600)
    return SAN


def _run(cmd, cwd, env):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900,
                          env=dict(os.environ, **ENV, **env))


def _clean(p):
    return p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr


def test_decoder_corpus_under_asan_ubsan(san_build, tmp_path):
    members = (list(ic.valid_members()) + list(ic.bam_members(tmp_path)) + list(ic.malformed_members()) +
               ic.mutated_members(400))
    corpus = tmp_path / "corpus.bin"
    ic.write_file(str(corpus), members)
    p = _run([os.path.join(san_build, "inflate-asan"), str(corpus)], str(tmp_path), {})
    assert _clean(p), p.stderr[-3000:]
    assert f"ok=1 members={len(members)}" in p.stdout, (p.stdout, p.stderr[-2000:])


@pytest.mark.parametrize("kind", ["asan", "tsan"])
def test_cli_batched_reader_under_sanitizers(san_build, datasets, tmp_path, kind):
    """SS_BGZF_DEVICE=cpu, 4 members per batch, pileup-only: no report, and the
    site stream of the default reader, streaming and with three contig groups."""
    cli = os.path.join(san_build, f"bam-somaticsniper-{kind}")
    for i, (d, fa, t, n) in enumerate(datasets):
        dst = tmp_path / f"s{i}"
        dst.mkdir()
        for f in os.listdir(d):
            if f.endswith((".bam", ".fa", ".fai")):
                shutil.copy(os.path.join(d, f), dst / f)
        indexed = not any(subprocess.run([INDEX, b], cwd=str(dst), capture_output=True).returncode for b in (t, n))
        for groups in ("1", "3") if indexed else ("1",):
            dumps = []
            for name, extra in (("plain", {}), ("batched", {"SS_BGZF_DEVICE": "cpu", "SS_BGZF_DEVICE_BATCH": "4"})):
                dump = f"{name}{groups}.dump"
                p = _run([cli, "-f", fa, t, n, f"{name}.out"], str(dst),
                         dict({"SS_PILEUP_ONLY": "1", "SS_CONTIG_GROUPS": groups, "SS_DUMP_PILEUP": dump,
                               "SS_TIMING": "1"}, **extra))
                assert _clean(p), (d, kind, groups, name, p.stderr[-3000:])
                dumps.append((dst / dump).read_bytes() if (dst / dump).exists() else b"")
                lines = [tuple(int(x) for x in m.groups()) for m in TIMING_LINE.finditer(p.stderr)]
                assert bool(lines) == bool(extra) and all(m > 0 and f == 0 for m, _, f in lines), (d, lines)
            assert dumps[0] == dumps[1], (d, kind, groups)
