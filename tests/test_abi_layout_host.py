"""The Python mirrors of the C ABI's structs (megagta_amd/_lib.py: STRUCTS, RECORDS) against include/megagta_hip.h, without a device: the
same structs, the same members in the same order, and the sizes and offsets the C compiler gives them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from megagta_amd import _lib
from tests import helpers as H

DECLARED = H.header_structs()


def test_every_struct_of_the_header_has_one_mirror():
    assert len(DECLARED) >= 40 and set(DECLARED) == set(_lib.STRUCTS), set(DECLARED) ^ set(_lib.STRUCTS)
    classes = list(_lib.STRUCTS.values())
    assert len(set(classes)) == len(classes) and all(issubclass(c, _lib.Struct) for c in classes)


def test_the_parser_reads_commas_arrays_and_comments():
    got = H.header_structs("typedef struct mgta_x { int32_t a, b; /* a; comment, */ uint8_t pad[2]; // int c;\n int64_t n[6], m; } mgta_x; int mgta_f(void);")
    assert got == {"mgta_x": [("int32_t", "a", None), ("int32_t", "b", None), ("uint8_t", "pad", 2), ("int64_t", "n", 6), ("int64_t", "m", None)]}
    assert H.header_fields("mgta_recruit_rec")[-3:] == ["frame", "status", "pad"] and ("int64_t", "n_recruited_frame", 6) in DECLARED["mgta_recruit_stats"]


@pytest.mark.parametrize("struct", list(DECLARED))
def test_members_are_the_headers_in_order(struct):
    cls = _lib.STRUCTS[struct]
    assert [name for name, _ in cls._fields_] == [name for _, name, _ in DECLARED[struct]]
    for (name, ctype), (_, _, length) in zip(cls._fields_, DECLARED[struct]):
        assert (ctype._length_ if issubclass(ctype, ctypes.Array) else None) == length, name


def test_sizes_and_offsets_are_the_c_compilers(tmp_path):
    """a C program prints sizeof of every struct of STRUCTS and offsetof + size of every member, from the header itself"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "megagta_hip.h"', 'int main(void) {']
    want = []
    for struct, cls in _lib.STRUCTS.items():
        lines.append(f'    printf("{struct} %zu\\n", sizeof({struct}));')
        want.append(f"{struct} {ctypes.sizeof(cls)}")
        for name, _ in cls._fields_:
            lines.append(f'    printf("{struct}.{name} %zu %zu\\n", offsetof({struct}, {name}), sizeof((({struct} *)0)->{name}));')
            want.append(f"{struct}.{name} {getattr(cls, name).offset} {getattr(cls, name).size}")
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "abi_layout.c", tmp_path / "abi_layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(H.HEADER), str(src), "-o", str(exe)])
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(got) == len(want) > 400
    assert [g for g, w in zip(got, want) if g != w] == []


@pytest.mark.parametrize("cls", list(_lib.RECORDS), ids=lambda c: c.__name__)
def test_record_dtype_has_the_layout_of_its_mirror(cls):
    dt = _lib.RECORDS[cls]
    assert cls in _lib.STRUCTS.values() and dt.itemsize == ctypes.sizeof(cls) and list(dt.names) == [name for name, _ in cls._fields_]
    for name, _ in cls._fields_:
        sub, offset = dt.fields[name][:2]
        assert (offset, sub.itemsize) == (getattr(cls, name).offset, getattr(cls, name).size), name
    assert np.zeros(3, dtype=dt).nbytes == 3 * ctypes.sizeof(cls)
