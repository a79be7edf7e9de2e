"""The error paths of the `megagta` binary that end before a device is opened: a table of invocations, and for each the exit code, stdout
and the stderr lines that carry no timing.  `python make_cli_errors.py [BIN]` records them into cli_errors.json beside this file;
tests/test_cli_errors_host.py runs the same table on the built binary and compares.  The records were taken from the binary of the
commit before the host CLI was split into units (megagta_main.cpp), so they pin that split and whatever follows it.

Every invocation runs in a directory of its own that holds INPUTS, with relative paths, so the messages name no place."""
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
GOLDEN = os.path.join(HERE, "cli_errors.json")

INPUTS = {
    "al.fa": ">a\nMK-V\n>b\nMKLV\n",                                       # two aligned protein records of four columns
    "al_uneven.fa": ">a\nMK-V\n>b\nMKL\n",                                 # the second row is narrower
    "al_zero.fa": ">a\nmk\n>b\nMK\n",                                      # the first row has no column at all
    "n_count.fa": ">a\nATGAAAGTT\n",                                       # one nucleotide record for two protein records
    "n_name.fa": ">a\nATGAAAGTT\n>c\nATGAAACTTGTT\n",                      # the second name differs
    "ref.faa": ">r1\nMKLV\n>r2\nMKIV\n",
    "c.fa": ">c\nACGT\n",
    "m_header.txt": "# two columns of one letter\nA A\nA 1 1\n",
    "m_row.txt": "A C\nA 1 x\nC 1 1\n",
    "m_missing.txt": "A C\nA 1 -1\n",
    "x.lib.lib_info": "1234 10\na\n0 3 100 se\nb\n5 9 100 se\n",           # the libraries do not tile: 4 is in neither
    "none.lib.lib_info": "0 0\n",                                         # no library at all
    "many.lib.lib_info": "25700 257\n" + "".join(f"lib {i}\n{i} {i} 100 se\n" for i in range(257)),   # one more than a call takes
    "two.lib.lib_info": "16 4\na\n0 3 4 se\n",                            # names four reads ...
    "two.lib.bin": struct.pack("<IIII", 4, 0x1B000000, 4, 0xE4000000),    # ... the file holds two (uint32 length + packed words each)
}
NEAREST = ["nearest", "ref.faa", "al.fa", "o"]
CHIMERA = ["chimera", "ref.faa", "al.fa", "o"]
PILEUP = ["pileup", "g", "x.lib", "c.fa", "o"]

CASES = [("no arguments", []), ("unknown sub-command", ["nosuchcommand", "x"])]
# wrong argument counts: the sixteen commands of a run, the three host filters, the commands of the tests
CASES += [("count " + a[0], a) for a in (
    ["buildgraph"], ["denovo"], ["search", "g"], ["findstart"], ["coverage", "g", "c.fa"], ["sharecov", "g", "c.fa"], ["matchreads", "g", "x.lib", "c.fa"],
    ["samplecov", "g", "x.lib", "c.fa"], ["pileup", "g", "x.lib", "c.fa"], ["derep", "al.fa"], ["align", "m.hmm", "al.fa"], ["posterior", "m.hmm", "al.fa"],
    ["cluster", "al.fa", "o", "0.01"], ["clustertree", "al.fa", "o", "0.01"], NEAREST + ["10", "1"], CHIMERA + ["10", "1", "1,-1", "5"],
    ["filterbylen"], ["translate"], ["buildlib", "x"], ["libdump", "x", "lib"], ["sdbgcopy", "x"], ["sdbgmerge", "x", "0"], ["hmmdump"])]
CASES += [
    ("buildgraph unknown option", ["buildgraph", "--nosuch"]), ("buildgraph no host memory", ["buildgraph", "--read_lib_file", "x.lib"]),
    ("denovo unknown option", ["denovo", "--nosuch"]), ("findstart no file", ["findstart", "nosuch.faa", "x.bin", "45"]),
    # not an integer / not a number
    ("cluster dist_cutoff", ["cluster", "al.fa", "o", "abc", "10"]), ("cluster min_overlap", ["cluster", "al.fa", "o", "0.01", "1x"]),
    ("cluster min_overlap empty", ["cluster", "al.fa", "o", "0.01", ""]), ("clustertree min_overlap", ["clustertree", "al.fa", "o", "0.01,0.03", "ten"]),
    ("nearest gap_open", NEAREST + ["a", "1", "1,-1"]), ("nearest gap_extend", NEAREST + ["10", "2.5", "1,-1"]),
    ("chimera gap_open", CHIMERA + ["1e1", "1", "1,-1", "5", "5"]), ("chimera gap_extend", CHIMERA + ["10", "", "1,-1", "5", "5"]),
    ("chimera min_seg", CHIMERA + ["10", "1", "1,-1", "5 ", "5"]), ("chimera min_gain", CHIMERA + ["10", "1", "1,-1", "5", "x5"]),
    # ranges
    ("nearest gap_extend negative", NEAREST + ["10", "-1", "1,-1"]), ("nearest gap_extend above gap_open", NEAREST + ["5", "6", "1,-1"]),
    ("nearest gap_open large", NEAREST + ["1025", "1", "1,-1"]), ("chimera gap_extend negative", CHIMERA + ["10", "-1", "1,-1", "5", "5"]),
    ("chimera gap_extend above gap_open", CHIMERA + ["5", "6", "1,-1", "5", "5"]), ("chimera gap_open large", CHIMERA + ["1025", "1", "1,-1", "5", "5"]),
    ("chimera min_seg zero", CHIMERA + ["10", "1", "1,-1", "0", "5"]), ("chimera min_seg large", CHIMERA + ["10", "1", "1,-1", "4097", "5"]),
    ("chimera min_gain zero", CHIMERA + ["10", "1", "1,-1", "5", "0"]), ("chimera min_gain large", CHIMERA + ["10", "1", "1,-1", "5", "1048577"]),
    # scoring
    ("scoring three commas", NEAREST + ["10", "1", "1,-1,2,3"]), ("scoring outside int8", NEAREST + ["10", "1", "128,-1"]),
    ("scoring below int8", CHIMERA + ["10", "1", "1,-129", "5", "5"]), ("scoring unreadable", NEAREST + ["10", "1", "nosuch.txt"]),
    ("scoring bad header", NEAREST + ["10", "1", "m_header.txt"]), ("scoring bad row", CHIMERA + ["10", "1", "m_row.txt", "5", "5"]),
    ("scoring missing row", NEAREST + ["10", "1", "m_missing.txt"]),
    # clustertree cut-offs
    ("cutoff empty item", ["clustertree", "al.fa", "o", "0.01,,0.03", "10"]), ("cutoff empty list", ["clustertree", "al.fa", "o", "", "10"]),
    ("cutoff exponent", ["clustertree", "al.fa", "o", "1e-2", "10"]), ("cutoff above one", ["clustertree", "al.fa", "o", "0.01,1.5", "10"]),
    ("cutoff twice", ["clustertree", "al.fa", "o", "0.01,0.03,0.010", "10"]),
    # rows
    ("cluster uneven rows", ["cluster", "al_uneven.fa", "o", "0.01", "10"]), ("cluster zero width", ["cluster", "al_zero.fa", "o", "0.01", "10"]),
    ("clustertree uneven rows", ["clustertree", "al_uneven.fa", "o", "0.01,0.03", "10"]),
    # pileup options
    ("pileup unknown option", PILEUP + ["--nosuch", "3"]), ("pileup no value", PILEUP + ["--min-depth"]), ("pileup max-span alone", PILEUP + ["--max-span", "5"]),
    ("pileup max-gap alone", PILEUP + ["--max-gap", "2"]), ("pileup negative", PILEUP + ["--min-depth", "-3"]), ("pileup not a count", PILEUP + ["--min-anchors", "3x"]),
    ("pileup too large", PILEUP + ["--phase", "--min-link", "2147483648"]),
    # the library table
    ("samplecov table", ["samplecov", "g", "x.lib", "c.fa", "o"]), ("pileup --phase table", PILEUP + ["--phase"]),
    ("samplecov no library", ["samplecov", "g", "none.lib", "c.fa", "o"]), ("samplecov 257 libraries", ["samplecov", "g", "many.lib", "c.fa", "o"]),
    ("samplecov fewer reads", ["samplecov", "g", "two.lib", "c.fa", "o"]), ("pileup --phase no library", ["pileup", "g", "none.lib", "c.fa", "o", "--phase"]),
    ("pileup --phase 257 libraries", ["pileup", "g", "many.lib", "c.fa", "o", "--phase"]),
    ("pileup --phase fewer reads", ["pileup", "g", "two.lib", "c.fa", "o", "--phase"]),
]
# the nucleotide records that go with the protein records: one check, three commands
PAIRED = {"derep": lambda n: ["derep", "al.fa", "o", n, "no"], "cluster": lambda n: ["cluster", "al.fa", "o", "0.01", "10", n, "no"],
          "chimera": lambda n: CHIMERA + ["10", "1", "1,-1", "5", "5", n, "no"]}
CASES += [(f"{cmd} {what}", mk(f"n_{what}.fa")) for cmd, mk in PAIRED.items() for what in ("count", "name")]
CASES += [("clustertree name", ["clustertree", "al.fa", "o", "0.01", "10", "n_name.fa", "no"])]

TIMING = re.compile(r"Real:|\d\s*m?s\b")


def run_case(binary, argv):
    """-> dict(rc, stdout, stderr lines without timing, the files the command left behind)"""
    with tempfile.TemporaryDirectory() as d:
        for name, text in INPUTS.items():
            with open(os.path.join(d, name), "wb") as f:
                f.write(text if isinstance(text, bytes) else text.encode())
        r = subprocess.run([binary] + argv, cwd=d, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=60)
        new = sorted(set(os.listdir(d)) - set(INPUTS))
    err = [line.replace(binary, "{BIN}") for line in r.stderr.splitlines() if not TIMING.search(line)]
    return dict(rc=r.returncode, stdout=r.stdout, stderr=err, new_files=new)


def run_table(binary):
    return {name: dict(argv=argv, **run_case(binary, argv)) for name, argv in CASES}


if __name__ == "__main__":
    records = run_table(sys.argv[1] if len(sys.argv) > 1 else BIN)
    with open(GOLDEN, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(records)} records -> {GOLDEN}")
