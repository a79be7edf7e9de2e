"""The host side of every call that takes a set of contigs (megagta_amd/csrc/contig_jobs.hpp: the check of the offsets, the cut into
batches of at most `cap` windows, the job list of a batch on one strand or both, the window offsets), checked by a stand-alone program
built with the address and undefined-behaviour sanitizers.  No device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "megagta_amd", "csrc")


def test_batches_jobs_and_offset_checks_under_sanitizers(tmp_path):
    exe = str(tmp_path / "contig_jobs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(CSRC, "host", "contig_jobs_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
