"""The host-side arithmetic of the oversized-segment route (megagta_amd/csrc/segment_split.hpp: the packing of the pieces of a split
segment into finish ranges, and the list capacities derived from its bound), checked by a stand-alone program built with the address
and undefined-behaviour sanitizers.  No device."""
import os
import subprocess

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "megagta_amd", "csrc")


def test_packer_and_list_capacities_under_sanitizers(tmp_path):
    exe = str(tmp_path / "segment_split_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(CSRC, "host", "segment_split_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_stats_struct_mirrors_the_header():
    """n_split_levels is the last field of mgta_build_stats, in the header and in the ctypes mirror"""
    from megagta_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    names = H.header_fields("mgta_build_stats", hdr)
    assert names == [n for n, _ in _lib.BuildStats._fields_]
    assert names[-1] == "n_split_levels"
