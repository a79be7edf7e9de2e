"""The error paths of the `megagta` binary, without a device: every invocation of tests/golden/cli_errors/make_cli_errors.py gives the exit
code, the stdout and the stderr lines (those without a time in them) that were recorded from the binary before the host CLI was split
into units, and leaves no file behind.  Only the sentence about an unknown sub-command may list its names in another order."""
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tests", "golden", "cli_errors", "make_cli_errors.py")
spec = importlib.util.spec_from_file_location("make_cli_errors", GEN)
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

WANT = json.load(open(gen.GOLDEN))
PIPELINE = ["buildgraph", "denovo", "search", "findstart", "coverage", "sharecov", "matchreads", "samplecov", "pileup", "derep", "align", "posterior", "cluster", "clustertree",
            "nearest", "chimera"]


@pytest.fixture(scope="module")
def got():
    assert os.path.exists(gen.BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    return gen.run_table(gen.BIN)


def test_the_table_is_the_recorded_table():
    assert list(WANT) == sorted(name for name, _ in gen.CASES) and len(WANT) == len(gen.CASES)
    assert all(WANT[name]["argv"] == argv for name, argv in gen.CASES)
    assert all(f"count {c}" in WANT for c in PIPELINE)
    # every record is an error that wrote nothing; nothing in it names a place
    for name, w in WANT.items():
        assert w["rc"] == 1 and w["new_files"] == [] and w["stderr"], name
        assert "/" not in "".join(w["stderr"]).replace("{BIN}", "").replace("cat contigs.fa | ", "").replace(".words / .start", ""), name


@pytest.mark.parametrize("name", [name for name, _ in gen.CASES if name != "unknown sub-command"])
def test_error_path_is_what_it_was(got, name):
    g, w = got[name], WANT[name]
    assert g["stderr"] == w["stderr"]
    assert (g["rc"], g["stdout"], g["new_files"], g["argv"]) == (w["rc"], w["stdout"], w["new_files"], w["argv"])


def test_usage_lists_the_commands_of_a_run_in_order(got):
    lines = got["no arguments"]["stderr"]
    assert lines[0] == "Usage: {BIN} <sub_program> [sub options]" and lines[1] == "    sub-programs on the MI355X hot path:"
    assert [line.split()[0] for line in lines[2:]] == PIPELINE + ["dumpversion"]


def test_unknown_sub_command_names_the_same_commands(got):
    g, w = got["unknown sub-command"], WANT["unknown sub-command"]
    assert (g["rc"], g["stdout"], g["new_files"]) == (w["rc"], w["stdout"], w["new_files"]) and len(g["stderr"]) == len(w["stderr"]) == 1
    pat = re.compile(r"^(.*\()([^()]*)( are\).*)$")
    mg, mw = pat.match(g["stderr"][0]), pat.match(w["stderr"][0])
    assert mg and mw and (mg.group(1), mg.group(3)) == (mw.group(1), mw.group(3))
    names_g, names_w = mg.group(2).split(", "), mw.group(2).split(", ")
    assert sorted(names_g) == sorted(names_w) and len(set(names_g)) == len(names_g) == 19 and set(PIPELINE) < set(names_g)


@pytest.mark.parametrize("what", ["count", "name"])
def test_the_pairing_check_differs_by_the_command_name_only(got, what):
    lines = {cmd: got[f"{cmd} {what}"]["stderr"] for cmd in gen.PAIRED}
    assert all(len(v) == 1 and f"[ERROR] {cmd}: " in v[0] and v[0].endswith(": nothing written") for cmd, v in lines.items())
    assert len({v[0].replace(f"[ERROR] {cmd}: ", "[ERROR] X: ") for cmd, v in lines.items()}) == 1
    assert ("holds 2 records, n_count.fa holds 1" if what == "count" else "record 1 is b in al.fa and c in n_name.fa") in lines["derep"][0]
