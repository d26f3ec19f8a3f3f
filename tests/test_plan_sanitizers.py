"""Sanitizer run of the device planner's host-visible code (CPU only; nothing
here touches a GPU or loads a sanitizer runtime into Python).

`make -C somatic-sniper_amd sanitize` builds tests/native/plan_driver.c -- a
stand-alone program over the planner's shared core (csrc/ss_plan_core.h, the
code the GPU kernels run), its CPU twin ss_pileup_split_cpu and
ss_bam_header_scan -- with ASan+UBSan.  It runs every case of
tests/plan_cases.py, the quirk records, the dataset BAMs' records and 400
byte-mutated spans, each in a heap block of exactly its size, and compares the
twin with its own plain walk and the device's plan steps with ss_pileup_plan."""
import gzip
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pileup_model as pm  # noqa: E402
import plan_cases as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "somatic-sniper_amd", "build", "san")
ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1:abort_on_error=0",
       "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


@pytest.fixture(scope="module")
def san_build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "somatic-sniper_amd"), "sanitize"], check=True,
                   capture_output=True, timeout=600)
    return SAN


def test_plan_corpus_under_asan_ubsan(san_build, tmp_path, datasets):
    spans = pc.cases(64) + pc.cases(512) + pc.quirk_cases() + pc.mutated_cases(400)
    headers = []
    for i, (d, fa, t, n) in enumerate(datasets):
        for f in (t, n):
            data = gzip.decompress(open(os.path.join(d, f), "rb").read())
            recs, names, lens = pm.bam_records(data)
            spans.append(pc.Span(f"{i}/{f}", recs, 512, len(names)))
            if i in (0, 5):
                headers.append((data, len(names), len(data) - len(recs)))
    corpus = tmp_path / "corpus.bin"
    pc.write_corpus(str(corpus), spans, headers)
    p = subprocess.run([os.path.join(san_build, "plan-asan"), str(corpus)], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=900, env=dict(os.environ, **ENV))
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert f"ok=1 spans={len(spans)} headers={len(headers)}" in p.stdout, (p.stdout, p.stderr[-2000:])
