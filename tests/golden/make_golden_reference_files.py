#!/usr/bin/env python3
"""Stores what the COMPILED REFERENCE writes for two host-side tests, so that they run where the reference binary is not built:
  tests/golden/<case>/ref_sdbg/k<k>_t<threads>/g.sdbg_info.gz, g.sdbg.<n>.gz   `megagta buildgraph` of <case>/reads.lib
      (test_oracle_golden.py::test_oracle_sdbg_reader_pinned_by_fresh_reference_files)
  tests/golden/filters/filterbylen_450.fa.gz, translate.faa.gz                   `megagta filterbylen 450` / `translate` of
      tests.helpers.write_filter_input (test_buildlib.py::test_filterbylen_and_translate_match_reference)
(build container only: needs oracle/_ref).   python tests/golden/make_golden_reference_files.py"""
import glob
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import helpers as H  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "megagta")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = (("toy", 44, 4), ("toy", 29, 2), ("ragged", 47, 3), ("ragged", 21, 8))     # the test's parameters


def gz(src: str, dst: str) -> None:
    with open(src, "rb") as fi, gzip.GzipFile(dst, "wb", compresslevel=9, mtime=0) as fo:
        shutil.copyfileobj(fi, fo)


d = tempfile.mkdtemp(prefix="mgta_gref_")
try:
    for case, k, threads in CASES:
        out = os.path.join(GOLDEN, case, "ref_sdbg", f"k{k}_t{threads}")
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(out)
        prefix = os.path.join(d, f"{case}_{k}")
        subprocess.run([REF, "buildgraph", "-k", str(k), "-m", "1", "--host_mem", "2000000000", "--mem_flag", "1", "--gpu_mem", "0", "--output_prefix",
                        prefix, "--num_cpu_threads", str(threads), "--num_output_threads", "1", "--read_lib_file", os.path.join(GOLDEN, case, "reads.lib")],
                       check=True, capture_output=True)
        for p in glob.glob(prefix + ".sdbg*"):
            gz(p, os.path.join(out, "g" + os.path.basename(p)[len(os.path.basename(prefix)):] + ".gz"))
        print(out, sorted(os.listdir(out)))
    os.makedirs(os.path.join(GOLDEN, "filters"), exist_ok=True)
    H.write_filter_input(os.path.join(d, "c.fa"))
    with open(os.path.join(d, "c.fa"), "rb") as fin, open(os.path.join(d, "f.fa"), "wb") as fout:
        subprocess.run([REF, "filterbylen", "450"], stdin=fin, stdout=fout, check=True)
    with open(os.path.join(d, "t.faa"), "wb") as fout:
        subprocess.run([REF, "translate", os.path.join(d, "f.fa")], stdout=fout, check=True)
    gz(os.path.join(d, "f.fa"), os.path.join(GOLDEN, "filters", "filterbylen_450.fa.gz"))
    gz(os.path.join(d, "t.faa"), os.path.join(GOLDEN, "filters", "translate.faa.gz"))
finally:
    shutil.rmtree(d, ignore_errors=True)
