"""The host side of every call that takes a set of protein sequences (megagta_amd/csrc/seq_jobs.hpp: the checks of the count, the
offsets and the letters with their error texts, the order longest first, the cut into batches of at most `cap` cells, the reference
columns, the waves that fit the LDS budget), checked by a stand-alone program built with the address and undefined-behaviour
sanitizers.  No device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "megagta_amd", "csrc")


def test_checks_order_batches_columns_and_waves_under_sanitizers(tmp_path):
    exe = str(tmp_path / "seq_jobs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(CSRC, "host", "seq_jobs_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
