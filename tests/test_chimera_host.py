"""Host side of the chimera check, no device: the files (writer and reader), the new symbols, the guards, the CLI's usage line and its
refusals, the driver's `--chimera` options, where the step's checkpoints go and what it is handed, and the restatement's suffix score
by reversal against the literal one."""
import ctypes
import importlib
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from megagta_amd import _lib, api
from megagta_amd import chimera as ch
from megagta_amd import nearest as nr
from tests import helpers as H
from tests.test_chimera_gpu import (cls, prefix_scores, random_seq, restate_chimera, row_maxima, score, suffix_scores_by_reversal, suffix_scores_literal, top_two,
                                    variant)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "megagta_amd", "bin", "megagta")
DRIVER = os.path.join(ROOT, "megagta_amd", "megagta.py")


def sample():
    """five contigs against three references: a chimera of r0 and r2, a clean one, an unchecked one that has a nearest reference, an
    empty one, and a chimera without a nearest reference"""
    headers, seqs = ["c0 len=9", "c1", "c2 x y", "c3 ", "c4"], ["MKVLAQWAM", "MKVLAAMK", "KVL", "", "AC"]
    ref_names = ["r0", "r1", "r2"]
    recs = np.array([(1, 0, 21, 5, 0, 25, 2, 20, 45, 24, 21), (0, 2, 31, 4, 2, 20, 0, 14, 34, 35, -1), (2, 1, 15, 0, -1, 0, -1, 0, 0, 0, 0), ch.UNCHECKED,
                     (1, -1, 0, 1, 0, 5, 1, 5, 10, 1, 9)], dtype=ch.REC)
    return headers, seqs, ref_names, dict(recs=recs)


def test_files_round_trip(tmp_path):
    headers, seqs, ref_names, result = sample()
    prefix = str(tmp_path / "prot_merged")
    ch.write_chimera(prefix, headers, seqs, ref_names, result)
    assert open(prefix + "_chimera.txt").read() == (
        "#contig\tstatus\tref\tscore\tlen\tbreak\tleft_ref\tleft_score\tright_ref\tright_score\ttwo\tone\tgain\n"
        "c0\tchimeric\tr0\t21\t9\t5\tr0\t25\tr2\t20\t45\t24\t21\n"
        "c1\tclean\tr2\t31\t8\t4\tr2\t20\tr0\t14\t34\t35\t-1\n"
        "c2\tunchecked\tr1\t15\t3\t0\t-\t0\t-\t0\t0\t0\t0\n"
        "c3\tunchecked\t-\t0\t0\t0\t-\t0\t-\t0\t0\t0\t0\n"
        "c4\tchimeric\t-\t0\t2\t1\tr0\t5\tr1\t5\t10\t1\t9\n")
    assert open(prefix + "_nochim.fasta").read() == ">c1\nMKVLAAMK\n>c2 x y\nKVL\n>c3 \n\n"
    back = ch.read_chimera(prefix + "_chimera.txt")
    assert back["names"] == ["c0", "c1", "c2", "c3", "c4"] and back["lens"].tolist() == [9, 8, 3, 0, 2]
    assert back["ref_names"] == ["r0", "r2", "r1", None, None] and back["left_names"] == ["r0", "r2", None, None, "r0"]
    assert back["right_names"] == ["r2", "r0", None, None, "r1"]
    first = nr.ref_index(ref_names)
    for f in ch.REC.names:
        want = result["recs"][f]
        col = {"ref": "ref_names", "left_ref": "left_names", "right_ref": "right_names"}.get(f)
        got = back["recs"][f] if col is None else np.array([-1 if x is None else first[x] for x in back[col]], dtype=np.int32)
        assert np.array_equal(got, want) and got.dtype == want.dtype, f
    assert ch.parse_chimera(ch.CHIMERA_HEADER)["names"] == [] and ch.parse_chimera(ch.CHIMERA_HEADER)["recs"].shape == (0,)
    assert ch.STATUS == ("clean", "chimeric", "unchecked") and ch.REC is api.CHIMERA_REC


def test_bad_lines_are_refused():
    H = ch.CHIMERA_HEADER
    good = "c0\tchimeric\tr0\t21\t9\t5\tr0\t25\tr2\t20\t45\t24\t21\n"
    unchecked = "c2\tunchecked\tr1\t15\t3\t0\t-\t0\t-\t0\t0\t0\t0\n"
    assert ch.parse_chimera(H + good + unchecked)["names"] == ["c0", "c2"]
    for bad in ("", good, H + good.replace("chimeric", "gone"), H + good[:-4] + "\n", H + good + "\n", H + good.replace("\t21\n", "\t20\n"),
                H + good.replace("\t45\t", "\t44\t"), H + good.replace("\t9\t5\t", "\t9\t9\t"), H + good.replace("\t9\t5\t", "\t9\t0\t"),
                H + good.replace("\tr2\t", "\t-\t"), H + good.replace("\t25\t", "\tx\t"), H + good.replace("\t9\t", "\t-9\t"),
                H + good.replace("\tr0\t21\t", "\t-\t21\t"), H + good.replace("\tr0\t21\t", "\t\t21\t"), H + unchecked.replace("\t0\t-\t0\t-", "\t1\t-\t0\t-"),
                H + unchecked.replace("\t-\t0\t-\t", "\tr0\t0\t-\t"), H + unchecked[:-2] + "3\n", H + good.replace("chimeric", "unchecked")):
        with pytest.raises(ValueError):
            ch.parse_chimera(bad)


def test_new_symbols_are_declared():
    new = {"mgta_seqs_chimera", "mgta_ctx_set_chimera_segment", "mgta_ctx_set_chimera_groups"}
    assert new <= set(_lib.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "megagta_hip.h")).read()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    for struct, mirror in (("mgta_chimera_stats", _lib.ChimeraStats), ("mgta_chimera_rec", _lib.ChimeraRec)):
        fields = [n for n, _ in mirror._fields_]
        names = H.header_fields(struct, hdr)
        assert names == fields, struct                                    # the ctypes mirror has the header's order
    assert [n for n, _ in _lib.ChimeraRec._fields_] == list(api.CHIMERA_REC.names) == list(ch.REC.names)
    assert [n for n, _ in _lib.ChimeraRec._fields_] == ["status", "ref", "score", "brk", "left_ref", "left_score", "right_ref", "right_score", "two", "one", "gain"]
    assert ctypes.sizeof(_lib.ChimeraRec) == api.CHIMERA_REC.itemsize == ch.REC.itemsize == 44
    for n in ("ms_top", "ms_parents", "n_cells", "n_items", "n_segments", "grid_blocks", "waves_per_block", "lds_bytes", "peak_bytes", "n_clean", "n_chimeric",
              "n_unchecked"):
        assert n in [f for f, _ in _lib.ChimeraStats._fields_]
    lib = _lib.load()                                                     # the library has them (dlopen needs no device)
    assert lib.mgta_seqs_chimera and lib.mgta_ctx_set_chimera_segment and lib.mgta_ctx_set_chimera_groups
    for m in ("chimera", "set_chimera_segment", "set_chimera_groups"):
        assert callable(getattr(api.Context, m))
    mk = open(os.path.join(ROOT, "megagta_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bchimera\.hip\b", mk, re.M)
    # the contract is in the header in full, and it says whose rule it is
    for word in ("min_seg", "min_gain", "P_r(b)", "S_r(b)", "unchecked", "not uchime's"):
        assert word in hdr, word


def test_guards_need_no_device():
    """the argument checks come before any device work: a NULL context and a setter's bad value are refused as such"""
    lib = _lib.load()
    assert lib.mgta_seqs_chimera(None, None, None, 0, None, None, 0, None, 10, 1, 10, 15, None, None, None) == -1 and b"ctx" in lib.mgta_last_error()
    assert lib.mgta_ctx_set_chimera_segment(None, 7) == -1 and b"ctx" in lib.mgta_last_error()
    assert lib.mgta_ctx_set_chimera_groups(None, 2) == -1 and b"ctx" in lib.mgta_last_error()


def test_guards_fire_in_order_without_a_device():
    """every guard of mgta_seqs_chimera comes before the context is used: a context pointer that is never dereferenced is enough to
    reach them (the first use of the context comes after the last guard and after the n = 0 return)"""
    lib = _lib.load()
    fake = ctypes.create_string_buffer(4096)                              # stands for a context; no guard reads it
    seqs, refs = b"ACDEACD", b"ACDEKACD"
    off, roff = np.array([0, 4, 7], dtype=np.uint64), np.array([0, 5, 8], dtype=np.uint64)
    sub = nr.match_mismatch(5, -4)
    recs = np.full(2 * 11, 77, dtype=np.int32)
    tops = np.full(7 * 8, 77, dtype=np.int32)
    stats = np.full(19, 77, dtype=np.int64)

    def refused(word, seqs_p=seqs, off_p=off.ctypes.data, n=2, refs_p=refs, roff_p=roff.ctypes.data, n_ref=2, sub_p=sub.ctypes.data, go=6, ge=1, min_seg=2,
                min_gain=5, recs_p=recs.ctypes.data):
        rc = lib.mgta_seqs_chimera(ctypes.addressof(fake), seqs_p, off_p, n, refs_p, roff_p, n_ref, sub_p, go, ge, min_seg, min_gain, recs_p, tops.ctypes.data,
                                   stats.ctypes.data)
        assert rc == -1 and word in lib.mgta_last_error(), (word, lib.mgta_last_error())

    refused(b"n = -1", n=-1)
    refused(b"n_ref = -1", n_ref=-1)
    refused(b"offsets", off_p=None)
    refused(b"ref_offsets", roff_p=None)
    refused(b"recs", recs_p=None)
    refused(b"sub", sub_p=None)
    refused(b"seqs", seqs_p=None)
    refused(b"refs", refs_p=None)
    for go, ge in ((6, 7), (6, -1), (1025, 1), (-1, -1)):
        refused(b"gap_open", go=go, ge=ge)
    for v in (0, -1, 4097):
        refused(b"min_seg", min_seg=v)
    for v in (0, -5, 2 ** 20 + 1):
        refused(b"min_gain", min_gain=v)
    down = np.array([0, 5, 4], dtype=np.uint64)
    refused(b"ascend", off_p=down.ctypes.data)
    refused(b"ascend", roff_p=down.ctypes.data)
    long_off = np.array([0, 4097, 4098], dtype=np.uint64)
    refused(b"4096 residues per contig", off_p=long_off.ctypes.data)
    refused(b"4096 residues per reference", roff_p=long_off.ctypes.data)
    many = np.arange(0, (2 ** 19 + 1) * 4096, 4096, dtype=np.uint64)       # 2^19 references of 4096 residues: 2^31 columns
    refused(b"2^31 residues", roff_p=many.ctypes.data, n_ref=many.size - 1)
    refused(b"2^31 contigs", n=2 ** 31)
    refused(b"2^31 references", n_ref=2 ** 31)
    assert lib.mgta_ctx_set_chimera_segment(ctypes.addressof(fake), -1) == -1 and b"columns" in lib.mgta_last_error()
    assert lib.mgta_ctx_set_chimera_groups(ctypes.addressof(fake), -1) == -1 and b"groups" in lib.mgta_last_error()
    # nothing was written by the refused calls
    assert (recs == 77).all() and (tops == 77).all() and (stats == 77).all()
    # n = 0: MGTA_OK, stats all zero, whatever else is NULL
    assert lib.mgta_seqs_chimera(ctypes.addressof(fake), None, None, 0, None, None, 0, None, 6, 1, 2, 5, None, None, stats.ctypes.data) == 0 and (stats == 0).all()


USAGE_LINE = "Usage: megagta chimera <ref.faa> <prot.fasta> <out_prefix> <gap_open> <gap_extend> <scoring> <min_seg> <min_gain> [<nucl.fasta> <nucl_out_prefix>]"


def test_cli_prints_the_usage_line():
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    r = subprocess.run([BIN, "chimera"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and USAGE_LINE in r.stderr
    for extra in (["a", "b", "c", "10", "1", "5,-4", "10"], ["a", "b", "c", "10", "1", "5,-4", "10", "15", "n.fa"]):
        r = subprocess.run([BIN, "chimera"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage: megagta chimera" in r.stderr
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and re.search(r"^\s+chimera\s", r.stderr, re.M)
    r = subprocess.run([BIN, "nosuchstep"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and re.search(r"is not built here \([^)]*\bchimera\b", r.stderr)


def test_cli_refuses_bad_parameters_before_any_device_work(tmp_path):
    """gap parameters, scoring, min_seg and min_gain are checked before a context is made: the step fails, names what is wrong and writes
    nothing"""
    assert os.path.exists(BIN), "megagta_amd/bin/megagta missing: run __graft_entry__.build()"
    (tmp_path / "ref.faa").write_text(">r0\nMKVLA\n")
    (tmp_path / "p.fa").write_text(">c0\nMKVLA\n")
    base = [BIN, "chimera", str(tmp_path / "ref.faa"), str(tmp_path / "p.fa"), str(tmp_path / "out")]
    for tail, word in ((["1", "2", "5,-4", "10", "15"], "gap_extend"), (["1025", "1", "5,-4", "10", "15"], "gap_open"), (["x", "1", "5,-4", "10", "15"], "gap_open"),
                       (["10", "1", "500,-4", "10", "15"], "int8"), (["10", "1", "5", "10", "15"], "scoring"), (["10", "1", "5,-4", "0", "15"], "min_seg"),
                       (["10", "1", "5,-4", "4097", "15"], "min_seg"), (["10", "1", "5,-4", "ten", "15"], "min_seg"), (["10", "1", "5,-4", "10", "0"], "min_gain"),
                       (["10", "1", "5,-4", "10", "1048577"], "min_gain"), (["10", "1", "5,-4", "10", "1.5"], "min_gain")):
        r = subprocess.run(base + tail, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "chimera" in r.stderr and word in r.stderr, (tail, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["p.fa", "ref.faa"]


def _fresh_driver(tmp_path, monkeypatch, calls):
    from megagta_amd import megagta as drv
    drv = importlib.reload(drv)
    monkeypatch.setattr(drv, "run_step", lambda cmd, what, stdin_path=None, stdout_path=None: calls.append(cmd))
    drv.opt.out_dir = str(tmp_path) + "/"
    drv.opt.temp_dir = drv.opt.out_dir + "tmp/"
    os.makedirs(drv.opt.temp_dir, exist_ok=True)
    drv.opt.lib = drv.opt.temp_dir + "reads.lib"
    drv.opt.gene_info = {"rplB": ("f_rplB.hmm", "r_rplB.hmm", "rplB.faa"), "nirK": ("f_nirK.hmm", "r_nirK.hmm", "nirK.faa")}
    return drv


def test_driver_accepts_the_options(tmp_path, monkeypatch):
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    assert drv.opt.chimera is False and (drv.opt.chimera_min_seg, drv.opt.chimera_min_gain) == (10, 15)
    out = str(tmp_path / "new_out")
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--chimera"])
    assert drv.opt.chimera is True and drv.opt.nearest is False and (drv.opt.chimera_min_seg, drv.opt.chimera_min_gain) == (10, 15)
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--chimera", "--chimera-min-seg", "12", "--chimera-min-gain", "30"])
    assert drv.opt.chimera is True and (drv.opt.chimera_min_seg, drv.opt.chimera_min_gain) == (12, 30)
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    drv.parse_opt(["-r", "reads.fa", "-g", "genes.txt", "-o", out, "--nearest"])
    assert drv.opt.chimera is False
    for word in ("--chimera ", "--chimera-min-seg", "--chimera-min-gain"):
        assert word in drv.USAGE
    assert drv.USAGE.count("this driver's own default, from a CPU trial") == 2 and "not uchime's" in drv.USAGE
    # what a finished run wrote into opts.txt brings the options back
    drv = _fresh_driver(tmp_path, monkeypatch, [])
    with open(drv.opt.out_dir + "opts.txt", "w") as fh:
        fh.write("\n".join(["-r", "reads.fa", "-g", "genes.txt", "--chimera", "--chimera-min-gain", "20"]) + "\n")
    drv.parse_opt(["--continue", "-o", str(tmp_path)])
    assert drv.opt.continue_mode and drv.opt.chimera is True and drv.opt.chimera_min_gain == 20 and drv.opt.chimera_min_seg == 10


def test_options_out_of_range_are_a_usage_error(tmp_path):
    base = [sys.executable, DRIVER, "-r", str(tmp_path / "reads.fa"), "-g", str(tmp_path / "genes.txt"), "-o", str(tmp_path / "out"), "--chimera"]
    for extra, word in ((["--chimera-min-seg", "0"], "--chimera-min-seg"), (["--chimera-min-seg", "4097"], "--chimera-min-seg"),
                        (["--chimera-min-gain", "0"], "--chimera-min-gain"), (["--chimera-min-gain", "1048577"], "--chimera-min-gain")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, extra
    assert not os.path.exists(tmp_path / "out")


OTHERS = ("coverage", "match_reads", "derep", "align", "cluster", "nearest")
COMBOS = [o for o in itertools.product([False, True], repeat=6) if o[3] or not o[4]]       # --cluster needs --align


@pytest.mark.parametrize("others", COMBOS, ids=lambda o: "".join("cmdaxn"[i] if x else "-" for i, x in enumerate(o)))
def test_checkpoints_of_the_flag_come_last(tmp_path, monkeypatch, others):
    """the steps of --chimera run behind every step of a run without the flag, for every combination of the other flags; one checkpoint
    per gene; the input is the representatives with --cluster, what --derep kept with --derep; without the flag the checkpoint list is
    unchanged"""
    def set_flags(drv, chimera):
        drv.opt.coverage, drv.opt.match_reads, drv.opt.derep, drv.opt.align, drv.opt.cluster, drv.opt.nearest = others
        drv.opt.chimera = chimera

    calls = []
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    set_flags(drv, False)
    drv.search_contigs(44)
    drv.after_search(44)
    before = [c[1] for c in calls]
    extra = [s for s, on in zip(("coverage", "matchreads", "derep", "align", "cluster", "nearest"), others) if on for _ in range(2)]
    assert before == ["search", "filterbylen", "translate", "filterbylen", "translate"] + extra
    cp_before = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp_before == "".join(f"{i}\tdone\n" for i in range(len(before)))                         # without the flag: what it was
    os.remove(drv.opt.temp_dir + "cp.txt")
    calls.clear()
    drv = _fresh_driver(tmp_path, monkeypatch, calls)
    set_flags(drv, True)
    drv.opt.nearest_scoring, drv.opt.nearest_gap_open, drv.opt.nearest_gap_extend, drv.opt.chimera_min_seg, drv.opt.chimera_min_gain = "3,-2", 7, 2, 12, 30
    drv.search_contigs(44)
    drv.after_search(44)
    assert [c[1] for c in calls] == before + ["chimera"] * 2
    d = drv.opt.out_dir + "contigs/"
    tail = "_merged" + ("_rmdup" if others[2] else "") + ("_rep_seqs" if others[4] else "")
    assert calls[-2:] == [[drv.opt.bin, "chimera", g + ".faa", d + g + "/prot" + tail + ".fasta", d + g + "/prot" + tail, "7", "2", "3,-2", "12", "30",
                           d + g + "/nucl" + tail + ".fasta", d + g + "/nucl" + tail] for g in ("rplB", "nirK")]
    if others[5]:
        near = [c for c in calls if c[1] == "nearest"][-1]
        assert near[2:4] == calls[-1][2:4] and near[5:8] == calls[-1][5:8]                          # the input and the scoring of --nearest
    if others[4]:
        clus = [c for c in calls if c[1] == "cluster"][-1]
        assert clus[3] + "_rep_seqs.fasta" == calls[-1][3] and clus[7] + "_rep_seqs.fasta" == calls[-1][10]      # it reads what --cluster wrote
    elif others[2]:
        derep = [c for c in calls if c[1] == "derep"][-1]
        assert derep[3] + "_rmdup.fasta" == calls[-1][3] and derep[5] + "_rmdup.fasta" == calls[-1][10]           # ... or what --derep kept
    cp = open(drv.opt.temp_dir + "cp.txt").read()
    assert cp.startswith(cp_before) and cp == "".join(f"{i}\tdone\n" for i in range(len(before) + 2))
    # continuing a finished run: nothing runs, every checkpoint is passed.  A search step that is skipped counts one checkpoint (its
    # filters' are written inside it), so past it the flag's two steps are number after + 1 and after + 2
    after = len(before) - 5
    for last_cp, want in ((len(before) + 1, []), (after + 2, []), (after + 1, ["chimera"]), (after, ["chimera"] * 2)):
        calls.clear()
        drv = _fresh_driver(tmp_path, monkeypatch, calls)
        set_flags(drv, True)
        drv.opt.continue_mode, drv.opt.last_cp = True, last_cp
        drv.search_contigs(44)
        drv.after_search(44)
        assert [c[1] for c in calls] == want and drv.cp == 1 + after + 2


def test_suffix_by_reversal_is_the_literal_suffix_score():
    """S_r(b) = score(x[b..L], y_r) scored on its own equals the prefix score of the reversed contig against the reversed reference at
    every b: with a symmetric sub, with one that is not, with free gaps, with R = 1 and R < L"""
    rng = np.random.default_rng(3)
    asym = rng.integers(-7, 8, (27, 27)).astype(np.int8)
    assert not np.array_equal(asym, asym.T)
    for trial in range(40):
        L, R = int(rng.integers(1, 16)), int(rng.integers(1, 16))
        base = random_seq(rng, 20)
        x, y = variant(rng, base, L), variant(rng, base, R)
        go = int(rng.integers(0, 9))
        ge = int(rng.integers(0, go + 1))
        for sub in (nr.match_mismatch(5, -4), asym):
            lit = suffix_scores_literal(x, y, sub, go, ge)
            assert suffix_scores_by_reversal(x, y, sub, go, ge) == lit, (trial, x, y, go, ge)
            assert lit[0] == score(x, y, sub, go, ge) == prefix_scores(x, y, sub, go, ge)[-1]     # the whole contig, from both ends
            assert lit[-1] == max(int(sub[cls(x[-1])][cls(c)]) for c in y)
    assert suffix_scores_literal(b"ACD", b"A", asym, 3, 1) == [None, None, int(asym[4][1])] == suffix_scores_by_reversal(b"ACD", b"A", asym, 3, 1)
    assert suffix_scores_by_reversal(b"ACD", b"", asym, 3, 1) == [None] * 3 == suffix_scores_literal(b"ACD", b"", asym, 3, 1)


def test_the_restatement_on_a_case_worked_by_hand():
    """AC against the references A and C with 5 / -4: left A on reference 0, right C on reference 1, no single parent for the whole"""
    sub = nr.match_mismatch(5, -4)
    assert row_maxima(b"AC", b"A", sub, 3, 1) == [5, None] and row_maxima(b"AC", b"CA", sub, 3, 1) == [5, -8]
    assert top_two([3, None, 7, 7]) == ((7, 2), (7, 3)) and top_two([None]) == ((-2 ** 31, -1),) * 2 and top_two([4]) == ((4, 0), (-2 ** 31, -1))
    recs, tops = restate_chimera([b"AC"], [b"A", b"C"], sub, 3, 1, 1, 1, literal=True)
    assert recs == [(1, -1, 0, 1, 0, 5, 1, 5, 10, 1, 9)]
    assert tops == [[(5, 0, -4, 1, -2 ** 31, -1, -2 ** 31, -1), (-2 ** 31, -1, -2 ** 31, -1, 5, 1, -4, 0)]]
    assert restate_chimera([b"AC"], [b"A", b"C"], sub, 3, 1, 1, 10, literal=True)[0][0][0] == 0                 # the same gain under a higher bar
    assert restate_chimera([b"AC"], [b"A", b"C"], sub, 3, 1, 2, 1)[0] == [ch.UNCHECKED]
    assert restate_chimera([b"AC", b""], [], sub, 3, 1, 1, 1) == ([ch.UNCHECKED] * 2, [[(-2 ** 31, -1) * 4] * 2, []])

