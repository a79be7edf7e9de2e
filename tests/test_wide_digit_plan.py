"""Host logic of the wide-digit plan rule (MGTA_SORT_WIDE, no device): mgta_sort_plan_wide answers with the plan the build takes."""
import ctypes
import os

import pytest

from megagta_amd import _lib


def _plan(n_items, W, b0, b1, wide=None, bias=None):
    """(passes, skipped bits, widths in running order) under MGTA_SORT_WIDE = wide, MGTA_SORT_BIAS = bias (None: unset)"""
    L = _lib.load()
    names = {"MGTA_SORT_WIDE": wide, "MGTA_SORT_BIAS": bias}
    old = {n: os.environ.get(n) for n in names}
    try:
        for n, v in names.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = str(v)
        P, s, w = ctypes.c_int(), ctypes.c_int(), (ctypes.c_int * 4)()
        _lib.check(L.mgta_sort_plan_wide(n_items, W, b0, b1, ctypes.byref(P), ctypes.byref(s), w), "mgta_sort_plan_wide")
        assert all(x == 0 for x in w[P.value:])
        return P.value, s.value, tuple(w[:P.value])
    finally:
        for n, v in old.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v


def _segment(n_items, b0, b1, s, widths):
    """average keys per segment of equal leading s + sum(widths) bits: the keys of [b0, b1) fill (b1 - b0) / 65536 of the prefixes"""
    return n_items / max(1.0, 2.0 ** sum(widths) * min(1.0, (b1 - b0) / 65536 * 2.0 ** s))


def test_the_metric_takes_three_passes():
    """100 M x 150 bp at k = 44: three ranges of a third of the buckets, 7.2 G keys each: 8 + 9 + 9 bits below one skipped bit"""
    third = (65536 + 2) // 3
    for b0 in (0, third, 2 * third):
        b1 = min(65536, b0 + third)
        P, s, w = _plan(7_200_000_000, 3, b0, b1)
        assert (P, s, w) == (3, 1, (8, 9, 9))
        assert s + sum(w) == 27 and _segment(7_200_000_000, b0, b1, s, w) <= 256
        assert _plan(7_200_000_000, 3, b0, b1, wide=0) == (4, 0, (8, 8, 8, 8))
        assert _plan(7_200_000_000, 3, b0, b1, bias=0) == (4, 0, (8, 8, 8, 8))    # no skipped bit: 26 bits leave 322-key segments
        assert _plan(7_200_000_000, 4, b0, b1) == (4, 0, (8, 8, 8, 8))            # four key words: the wide scatter does not fit the LDS


def test_the_whole_build_of_ten_million_reads_is_unchanged():
    """2.16 G keys over every bucket need 23 bits: 8 + 9 bits would leave 16 479-key segments"""
    assert _plan(2_160_000_000, 3, 0, 65536) == (3, 0, (8, 8, 8))
    assert _plan(2_160_000_000, 3, 0, 65536, wide=0) == (3, 0, (8, 8, 8))
    assert _plan(2_160_000_000, 3, 0, 65536, wide=2) == (3, 0, (8, 9, 9))


def test_wide_digits_only_where_they_remove_a_pass():
    assert _plan(4_000_000, 3, 0, 65536) == (2, 0, (8, 8))                        # one 8-bit pass would not do
    assert _plan(4_000_000, 3, 0, 65536, wide=2) == (2, 0, (8, 9))
    assert _plan(20_000_000, 3, 0, 65536) == (2, 0, (8, 9))                       # 153-key segments in place of a third pass
    assert _plan(40_000_000, 3, 0, 65536) == (3, 0, (8, 8, 8))                    # 305
    assert _plan(100, 3, 0, 65536, wide=2) == (0, 0, ())


@pytest.mark.parametrize("wide", [0, 1, 2])
def test_invariants(wide):
    import numpy as np
    L = _lib.load()
    rng = np.random.default_rng(12 + wide)
    for _ in range(1500):
        b0 = int(rng.integers(0, 65536))
        b1 = int(rng.integers(b0 + 1, 65537))
        n = int(10 ** rng.uniform(1, 10.5))
        W = int(rng.integers(2, 10))
        for bias in (0, 1, 2):
            P, s, w = _plan(n, W, b0, b1, wide=wide, bias=bias)
            P8, s8 = ctypes.c_int(), ctypes.c_int()
            os.environ["MGTA_SORT_BIAS"] = str(bias)
            try:
                _lib.check(L.mgta_sort_plan(n, W, b0, b1, ctypes.byref(P8), ctypes.byref(s8)), "mgta_sort_plan")
            finally:
                os.environ.pop("MGTA_SORT_BIAS", None)
            assert 0 <= P <= P8.value <= 4 and s + sum(w) <= 32
            assert all(8 <= x <= 9 for x in w) and (not w or w[0] == 8)           # the pass that runs first keeps 8 bits
            if wide == 0 or W > 3:
                assert (P, s) == (P8.value, s8.value) and all(x == 8 for x in w)
            if wide == 1 and P < P8.value:
                assert P == P8.value - 1 and any(x > 8 for x in w) and _segment(n, b0, b1, s, w) <= 256
            if s:
                assert bias != 0 and s + sum(w) >= 16 and ((b1 - b0) << 16) - 1 < (1 << (32 - s))
