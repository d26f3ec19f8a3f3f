"""Sanitizer run of the record pileup's host code (CPU only; nothing here
touches a GPU or loads a sanitizer runtime into Python).

`make -C somatic-sniper_amd sanitize` builds tests/native/pileup_driver.c -- a
stand-alone program over the shared pileup core (csrc/ss_pileup_core.h, the
code the GPU kernels run), the CPU twin and the planner -- with ASan+UBSan.  It
builds every case of tests/pileup_model.py, the rejection cases and 400
byte-mutated samples included, with every input and output in a heap block of
exactly its size."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pileup_model as pm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "somatic-sniper_amd", "build", "san")
ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1:abort_on_error=0",
       "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


@pytest.fixture(scope="module")
def san_build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "somatic-sniper_amd"), "sanitize"], check=True,
                   capture_output=True, timeout=600)
    return SAN


def test_pileup_corpus_under_asan_ubsan(san_build, tmp_path):
    cases = pm.branch_cases() + pm.rejection_cases() + pm.mutated_cases(400)
    corpus = tmp_path / "corpus.bin"
    pm.write_corpus(str(corpus), cases)
    p = subprocess.run([os.path.join(san_build, "pileup-asan"), str(corpus)], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=900, env=dict(os.environ, **ENV))
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert f"ok=1 cases={len(cases)}" in p.stdout, (p.stdout, p.stderr[-2000:])
