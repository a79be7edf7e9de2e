"""What the Python bindings hand the C ABI, without a device: every case of tests/golden/api_calls/make_api_calls.py makes the C calls, with
the arguments, and returns or raises what was recorded from the bindings before they were reshaped (api_calls.json).  The table reaches
every library function that api.py and findstart.py call."""
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "tests", "golden", "api_calls", "make_api_calls.py")
spec = importlib.util.spec_from_file_location("make_api_calls", GEN)
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

WANT = gen.load_golden()
CASES = {name: (script, world, fn) for name, script, world, fn in gen.CASES}
text = lambda rec: json.dumps(rec, sort_keys=True)


def test_the_table_is_the_recorded_table():
    assert len(CASES) == len(gen.CASES), "two cases of one name"
    assert sorted(WANT) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_call_is_what_it_was(name):
    assert os.path.exists(gen._lib.LIB_PATH), "megagta_amd/libmegagta_hip.so missing: run __graft_entry__.build()"
    got, want = gen.run_case(*CASES[name]), WANT[name]
    assert len(got["calls"]) == len(want["calls"]) and [c["fn"] for c in got["calls"]] == [c["fn"] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        for i, (ga, wa) in enumerate(zip(g["args"], w["args"])):
            assert text(ga) == text(wa), f"{g['fn']}: argument {i}"
    assert text(got) == text(want)


def test_every_library_function_the_bindings_call_is_recorded():
    called = set()
    for name in ("api.py", "findstart.py"):
        called |= set(re.findall(r"\.(mgta_\w+)\(", open(os.path.join(ROOT, "megagta_amd", name)).read()))
    recorded = {c["fn"] for rec in WANT.values() for c in rec["calls"]}
    assert len(called) > 70 and not called - recorded, sorted(called - recorded)
    assert set(gen.HOST_ONLY) <= recorded
