"""The layout of helpers.reads_behind_marks, checked on its numbers: a broken layout must not be able to hide a failure of the device
stages that tests/test_far_offsets_gpu.py runs on it.  About 2 GB of host memory per mode.  And the list of those stages, held against
the entry points of include/megagta_hip.h that take the reads."""
import os
import re

import numpy as np
import pytest

from megagta_amd import readlib
from tests import helpers as H

FILL_LEN = 44
SEED = 7


def unpack(packed, start, r):
    """read r of the layout as sequenced, base by base from the packed words (base q: word q >> 4, bits 30 - 2 (q & 15) and up)"""
    q = np.arange(int(start[r]), int(start[r + 1]), dtype=np.int64)
    stored = (packed[q >> 4] >> (30 - 2 * (q & 15)).astype(np.uint32)) & 3
    return stored[::-1].astype(np.uint8)


@pytest.fixture(scope="module")
def payload(golden_dir):
    return readlib.load_lib_bin(os.path.join(golden_dir, "toy", "reads.lib"))


@pytest.mark.parametrize("mode", ["straddle", "exact"])
def test_layout_on_the_numbers(payload, mode):
    packed, start, ids = H.reads_behind_marks(payload, FILL_LEN, mode, SEED)
    n = len(payload)
    n1, n2 = H.split_payload(n)
    assert packed.dtype == np.uint32 and start.dtype == np.uint64 and ids.shape == (n,)
    assert 0 < n1 < n2 < n and n1 % 2 == 0 and n2 % 2 == 0
    s = start.view(np.int64)
    lens = np.diff(s)
    # start ascends (strictly: no empty filler read) and ends inside the packed words
    assert s[0] == 0 and lens.min() > 0 and s[-1] <= 16 * packed.size and s[-1] > H.MARKS[1]
    # the payload reads are where ids says, in order, and unpack to themselves
    assert (np.diff(ids) > 0).all() and ids[-1] == s.size - 2
    assert np.array_equal(lens[ids], [r.size for r in payload])
    for i in list(range(0, n, 97)) + [n1 // 2, n1 // 2 + 1, n1 - 1, n1, (n1 + n2) // 2, n2 - 1, n2, n - 1]:
        assert np.array_equal(unpack(packed, start, int(ids[i])), payload[i]), i
    # three contiguous blocks: B1 alone, B3 directly behind B2
    assert (np.diff(ids[:n1]) == 1).all() and (np.diff(ids[n1:]) == 1).all() and ids[n1] > ids[n1 - 1] + 1 and ids[0] > 0
    # every other read is filler: no longer than fill_len, at most one shorter one in front of each block
    is_payload = np.zeros(lens.size, dtype=bool)
    is_payload[ids] = True
    fill = lens[~is_payload]
    assert fill.size > 90_000_000 and fill.max() == FILL_LEN
    short = np.flatnonzero(~is_payload & (lens != FILL_LEN))
    assert short.size <= 2 and set(short.tolist()) <= {int(ids[0]) - 1, int(ids[n1]) - 1}
    # the marks
    b0, e0 = s[ids], s[ids + 1]                                          # first base and one past the last base of every payload read
    for mark, lo, hi in ((H.MARKS[0], 0, n1), (H.MARKS[1], n1, n)):
        if mode == "straddle":
            inside = np.flatnonzero((b0 + 16 <= mark) & (mark + 16 <= e0))
            assert inside.size == 1 and lo <= inside[0] < hi, (mark, inside)
        else:
            i = np.flatnonzero(b0 == mark)
            assert i.size == 1 and lo < i[0] < hi and e0[i[0] - 1] == mark and ids[i[0] - 1] == ids[i[0]] - 1, (mark, i)
    if mode == "straddle":
        assert (b0[n2:] > H.MARKS[1]).all() and b0[n1] < H.MARKS[1]       # B3 entirely above 2^32
        assert b0[0] < H.MARKS[0] < e0[n1 - 1] and e0[n1 - 1] < b0[n1]
    else:
        assert int(start[ids[n2]]) & 0xFFFFFFFF == 0 and int(start[ids[n2]]) == H.MARKS[1]
    # the decoys: every filler word that a payload base offset wraps to is non-zero, every other filler word is zero
    own = np.unique(np.concatenate([np.arange(b >> 4, (e + 15) >> 4) for b, e in ((b0[0], e0[n1 - 1]), (b0[n1], e0[-1]))]))
    x = np.concatenate([np.arange(b, e) for b, e in ((b0[0], e0[n1 - 1]), (b0[n1], e0[-1]))])     # every payload base offset
    stored = ((packed[x >> 4] >> (30 - 2 * (x & 15)).astype(np.uint32)) & 3).astype(np.uint8)
    assert np.array_equal(stored, np.concatenate([r[::-1] for r in payload]))                      # every read, reversed, no padding between reads
    wraps = np.unique(np.concatenate([(x[x >= m] % m) >> 4 for m in H.MARKS]))
    decoy = np.setdiff1d(wraps, own)
    assert decoy.size > 10_000 and (packed[decoy] != 0).all()
    nz = np.flatnonzero(packed)
    assert np.isin(nz, np.concatenate([own, decoy])).all()
    assert not np.isin(decoy, own).any() and decoy.max() < own.min()      # the decoys lie in the first filler run
    assert np.unique(packed[decoy]).size > 0.99 * decoy.size               # random bits, not one pattern


def entry_points_taking_reads(hdr):
    """the functions of the header text that take a `const mgta_reads *`: comments dropped as helpers.header_structs drops them, a
    declaration = a name, its parameters up to the closing parenthesis (over any number of lines) and a semicolon"""
    hdr = re.sub(r"/\*.*?\*/|//[^\n]*", " ", hdr, flags=re.S)
    decls = re.findall(r"\b(mgta_\w+)\s*\(([^()]*)\)\s*;", hdr)
    return {name for name, params in decls if re.search(r"\bconst\s+mgta_reads\s*\*", params)}


def test_every_entry_point_that_takes_reads_is_covered_or_excused():
    """a new read-consuming entry point fails here until tests/test_far_offsets_gpu.py names the tests that run it behind the marks (or
    says why it never indexes bases by start[r])"""
    from tests import test_far_offsets_gpu as FG
    found = entry_points_taking_reads(H.header_text())
    assert {"mgta_sdbg_build_resident", "mgta_findstart", "mgta_reads_recruit", "mgta_reads_pileup_gapped"} <= found       # the parser finds them, over line breaks too
    assert "mgta_reads_free" not in found and "mgta_reads_upload" not in found
    assert entry_points_taking_reads(H.header_text() + "\nint mgta_x(const mgta_reads *);\n") == found | {"mgta_x"}
    assert entry_points_taking_reads(H.header_text() + "\nint mgta_y(mgta_ctx *,\n    const   mgta_reads\n*reads, int k);\n") == found | {"mgta_y"}
    assert set(FG.COVERED) | set(FG.NOT_READ) == found
    assert not set(FG.COVERED) & set(FG.NOT_READ)
    assert all(isinstance(why, str) and why.strip() for why in FG.NOT_READ.values())
    marks = FG.pytestmark if isinstance(FG.pytestmark, (list, tuple)) else [FG.pytestmark]
    assert any(m.name == "gpu" for m in marks)                            # the module's mark: every test of it carries it
    for entry, names in FG.COVERED.items():
        assert names, entry
        for name in names:
            assert name.startswith("test_") and callable(getattr(FG, name, None)), (entry, name)
    # and no test of the module is left out of the table
    tests = {name for name, f in vars(FG).items() if name.startswith("test_") and callable(f) and getattr(f, "__module__", None) == FG.__name__}
    assert tests == {name for names in FG.COVERED.values() for name in names}


def test_the_helper_refuses_what_it_cannot_lay_out(payload):
    with pytest.raises(ValueError):
        H.reads_behind_marks(payload, FILL_LEN, "sideways", SEED)
    with pytest.raises(ValueError):
        H.reads_behind_marks(payload[:4], FILL_LEN, "exact", SEED)
