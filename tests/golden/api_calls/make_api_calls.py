"""What every wrapper of megagta_amd/api.py (and findstart.find_hits) hands the C ABI, without a device: a table of calls made against a
recording stand-in for the loaded library, and for each the C calls it made -- name, and per argument the scalar, the bytes (length +
digest), NULL, the struct behind a byref (type, size; the bytes of a *Params struct), or the array behind a data pointer (dtype, shape,
digest) -- and what the wrapper returned (keys in order, types, dtypes, shapes, digests), or the exception it raised.
`python make_api_calls.py` records them into api_calls.json beside this file; tests/test_api_calls_host.py replays the same table on the
working tree and compares record by record.  The records were taken from the code of commit 5b2f5d1 ("Test every HMM-consuming kernel
on position-specific profile HMMs"), the last one before the bindings were reshaped around one mirror per struct and a few marshalling
helpers, so they pin that reshaping and whatever follows it.

The stand-in answers 0 unless the case scripts an answer.  The array behind a data pointer is found by its address among the numpy arrays
alive in the frames of the call stack; a pointer that is not NULL and cannot be found fails the recording, so no argument drops out of
the comparison unnoticed.  The host-only entries (mgta_phase_pairs, mgta_pairs_link, mgta_tree_cut) are passed on to the built library."""
import ctypes as C
import hashlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(HERE, "api_calls.json")

from megagta_amd import _lib, api, findstart  # noqa: E402

HOST_ONLY = ("mgta_phase_pairs", "mgta_pairs_link", "mgta_tree_cut")
# output buffers that the wrapper takes from np.empty: their contents before the call are not defined (function -> argument positions)
UNINITIALISED = {"mgta_sdbg_outgoing": (3, 4), "mgta_sdbg_index_edges": (3,), "mgta_sdbg_edge_multiplicity": (3,), "mgta_stream_download": (1, 2)}


def sha(b) -> str:
    return hashlib.sha1(bytes(b)).hexdigest()[:16]


class Handle:
    """what stands for a mgta_ctx / mgta_sdbg / mgta_reads / mgta_hmm"""

    def __init__(self, name):
        self.name = name


class FakeTensor:
    """what torch.empty gives export_records_to_torch here: the few members that wrapper uses, over a numpy array"""

    def __init__(self, a):
        self.array = a

    def data_ptr(self):
        return self.array.ctypes.data

    def numel(self):
        return self.array.size

    def __getitem__(self, s):
        return FakeTensor(self.array[s])


FAKE_TORCH = types.SimpleNamespace(uint8="uint8", empty=lambda n, dtype, device: FakeTensor(np.zeros(n, dtype=dtype)))


def dtype_of(dt: np.dtype):
    if dt.names is None:
        return dt.str
    return dict(itemsize=dt.itemsize, names=list(dt.names), offsets=[int(dt.fields[n][1]) for n in dt.names])


def array_record(a: np.ndarray, contents: bool = True) -> dict:
    return dict(dtype=dtype_of(a.dtype), shape=list(a.shape), sha=sha(np.ascontiguousarray(a).tobytes()) if contents else "not defined")


def arrays_in(v, depth=0):
    if isinstance(v, (np.ndarray, C.Array)):
        yield v
    elif isinstance(v, FakeTensor):
        yield v.array
    elif isinstance(v, (list, tuple)) and depth < 2 and len(v) <= 16:
        for x in v:
            yield from arrays_in(x, depth + 1)


def address_of(a) -> int:
    return a.ctypes.data if isinstance(a, np.ndarray) else C.addressof(a)


def resolve(addr: int):
    """the array at `addr` among the locals of the frames above the stand-in, the table's own frames left out; the largest, then the innermost"""
    best, f = None, sys._getframe(1)
    while f is not None:
        if f.f_globals.get("__name__") != __name__:
            for v in list(f.f_locals.values()):
                for a in arrays_in(v):
                    if address_of(a) == addr and (best is None or nbytes(a) > nbytes(best)):
                        best = a
        f = f.f_back
    return best


def nbytes(a) -> int:
    return a.nbytes if isinstance(a, np.ndarray) else C.sizeof(a)


def struct_record(obj) -> dict:
    rec = dict(type=type(obj).__name__, size=C.sizeof(obj))
    if type(obj).__name__.endswith("Params"):
        rec["bytes"] = bytes(obj).hex()
    return rec


def data_record(a, contents=True) -> dict:
    if isinstance(a, np.ndarray):
        return dict(array=array_record(a, contents))
    return dict(ctypes_array=type(a)._type_.__name__, length=len(a), size=C.sizeof(a))


def describe(fn: str, i: int, a, argtype):
    """-> (the JSON record of argument i, the object a script may write through)"""
    contents = i not in UNINITIALISED.get(fn, ())
    if a is None:
        return "null", None
    if isinstance(a, Handle):
        return dict(handle=a.name), a                            # (a script may ask WHICH handle of that name it was given)
    if isinstance(a, (bytes, bytearray)):
        return dict(bytes=len(a), sha=sha(a)), None
    if isinstance(a, C._CFuncPtr):
        return ("callback" if a else "null callback"), a
    if type(a).__name__ == "CArgObject":                         # C.byref(x)
        return dict(byref=struct_record(a._obj)), a._obj
    if isinstance(a, C.Array):
        return data_record(a, contents), a
    if isinstance(a, C.c_void_p):                                # a handle the stand-in gave out, or C.cast(array, c_void_p)
        if a.value is None:
            return dict(pointer="c_void_p", value="null"), a
        found = resolve(a.value)
        if found is None:
            return dict(pointer="c_void_p", value="set"), a
        return data_record(found, contents), found
    if isinstance(a, (bool, int, np.integer)) and argtype is C.c_void_p:
        if int(a) == 0:
            return "null", None
        found = resolve(int(a))
        if found is None:
            raise LookupError(f"{fn}: argument {i} is a pointer to no array of the call stack")
        return data_record(found, contents), found
    if isinstance(a, (bool, int, float, np.integer, np.floating)):
        return (float(a) if isinstance(a, (float, np.floating)) else int(a)), None
    raise TypeError(f"{fn}: argument {i} of type {type(a).__name__}")


class Recorder:
    """stands for the loaded library: every mgta_* call is written down, answered by the case's script (a value, or a function of
    (the objects behind the arguments, the number of earlier calls of that function) that may write through them), else by 0"""

    def __init__(self, script=None):
        self.script, self.calls, self.seen = dict(script or {}), [], {}
        self.recording = True

    def __getattr__(self, fn):
        if not fn.startswith("mgta_"):
            raise AttributeError(fn)

        def call(*args):
            argtypes = _lib.SYMBOLS[fn][1]
            if len(args) != len(argtypes):
                raise TypeError(f"{fn} takes {len(argtypes)} arguments, got {len(args)}")
            if not self.recording:
                return None
            recs, objs = zip(*[describe(fn, i, a, t) for i, (a, t) in enumerate(zip(args, argtypes))]) if args else ((), ())
            self.calls.append(dict(fn=fn, args=list(recs)))
            nth = self.seen.get(fn, 0)
            self.seen[fn] = nth + 1
            if fn in HOST_ONLY:
                return getattr(REAL(), fn)(*args)
            answer = self.script.get(fn, b"scripted error" if fn == "mgta_last_error" else 0)
            return answer(objs, nth) if callable(answer) else answer
        return call


_REAL = []


def REAL():
    if not _REAL:
        _REAL.append(_LOAD())
    return _REAL[0]


_LOAD = _lib.load


def value_record(v):
    """what a wrapper returned: keys in order; arrays with dtype, shape and digest; str by value; other scalars by type"""
    if isinstance(v, dict):
        return dict(dict=[[k, value_record(x)] for k, x in v.items()])
    if isinstance(v, (list, tuple)):
        return {type(v).__name__: [value_record(x) for x in v]}
    if isinstance(v, np.ndarray):
        return dict(array=array_record(v))
    if isinstance(v, FakeTensor):
        return dict(tensor=array_record(v.array))
    if isinstance(v, C.Array):
        return data_record(v)
    if isinstance(v, str):
        return dict(str=v)
    if isinstance(v, api.SeedResult):
        return dict(SeedResult=value_record(dict(left=v.left, right=v.right, right_side=v.right_side, left_side=v.left_side)))
    if isinstance(v, (api.Graph, api.Reads, api.DeviceHmm, api.Context, api.EdgeStream)):
        keys = [k for k in ("k", "size", "keep_multiplicity", "n_reads", "M", "A", "words_per_tip", "bucket_items", "records", "large", "tips", "bucket_large",
                            "bucket_tips", "stats", "_keep") if hasattr(v, k)]
        return {type(v).__name__: value_record({k: getattr(v, k) for k in keys})}
    return type(v).__name__


# ---- what the cases are made of -------------------------------------------------------------------------------------------------
class World:
    """one case's stand-ins: lib (the Recorder), ctx, graph (k = 4, as mgta_sdbg_k answers), reads (5 reads), hmm (M = 3)"""

    def __init__(self, script=None, n_reads=5, M=3):
        self.lib = Recorder({"mgta_sdbg_k": 4, **(script or {})})
        self.ctx = api.Context.__new__(api.Context)
        self.ctx._L, self.ctx.h = self.lib, Handle("ctx")
        self.graph = api.Graph.__new__(api.Graph)
        self.graph.ctx, self.graph.h, self.graph.k, self.graph.size = self.ctx, Handle("graph"), 4, 130
        self.reads = api.Reads(self.ctx, Handle("reads"), n_reads)
        self.hmm = types.SimpleNamespace(h=Handle("hmm"), M=M)
        self.rev = types.SimpleNamespace(h=Handle("hmm_rev"), M=M)


CASES = []


def case(name, script=None, **world):
    def add(fn):
        CASES.append((name, script, world, fn))
        return fn
    return add


def each(prefix, variants, script=None, **world):
    """one case per (tag, function of the World)"""
    for tag, fn in variants:
        CASES.append((f"{prefix} {tag}", script, world, fn))


SUB = np.arange(27 * 27, dtype=np.int8).reshape(27, 27)
SEQS = {"none": [], "str": ["MKV", "ML"], "bytes": [b"MKV", bytearray(b"ML")], "non-ascii": ["MKé", "L"], "one": ["ACGTAC"]}
CONTIGS = {"none": [], "two": ["ACGTACG", "acgtn"], "short": ["ACG", "AC"], "bytes": [b"ACGTAC"], "non-ascii": ["ACGTéCG"]}


def set_value(i, v):
    """script: write v through the byref argument i"""
    def answer(objs, nth):
        objs[i].value = v
        return 0
    return answer


# ---- the context's switches: one int each -----------------------------------------------------------------------------------------
each("switch", [
    ("set_full_lsd", lambda w: w.ctx.set_full_lsd(3)), ("set_mem_limit", lambda w: w.ctx.set_mem_limit(1 << 33)), ("keep_stream", lambda w: w.ctx.keep_stream()),
    ("keep_stream 2", lambda w: w.ctx.keep_stream(2)), ("keep_multiplicity", lambda w: (w.ctx.keep_multiplicity(), w.ctx._keep_multiplicity)),
    ("keep_multiplicity off", lambda w: (w.ctx.keep_multiplicity(0), w.ctx._keep_multiplicity)), ("set_coverage_batch", lambda w: w.ctx.set_coverage_batch(7)),
    ("set_coverage_batch default", lambda w: w.ctx.set_coverage_batch()), ("set_share_hash_bits", lambda w: w.ctx.set_share_hash_bits(3)),
    ("set_share_hash_bits default", lambda w: w.ctx.set_share_hash_bits()), ("set_pileup_chunk", lambda w: w.ctx.set_pileup_chunk(2)),
    ("set_phase_chunk", lambda w: w.ctx.set_phase_chunk(2)), ("set_recruit_chunk", lambda w: w.ctx.set_recruit_chunk(2)),
    ("set_derep_hash_bits", lambda w: w.ctx.set_derep_hash_bits(5)), ("set_align_batch", lambda w: w.ctx.set_align_batch(9)),
    ("set_posterior_batch", lambda w: w.ctx.set_posterior_batch(9)), ("set_cluster_tile", lambda w: w.ctx.set_cluster_tile(2)),
    ("set_nearest_batch", lambda w: w.ctx.set_nearest_batch(9)), ("set_chimera_segment", lambda w: w.ctx.set_chimera_segment(1)),
    ("set_chimera_groups", lambda w: w.ctx.set_chimera_groups(2)), ("release_scratch", lambda w: w.ctx.release_scratch()),
    ("set_search_arena", lambda w: w.ctx.set_search_arena(10, 1 << 20)), ("set_search_arena default", lambda w: w.ctx.set_search_arena()),
    ("set_search_page_limit", lambda w: w.ctx.set_search_page_limit(3)), ("last_counting", lambda w: w.ctx.last_counting()),
    ("set_search_share", lambda w: w.ctx.set_search_share(1, 2)), ("set_search_share default", lambda w: w.ctx.set_search_share()),
    ("close", lambda w: (w.ctx.close(), w.ctx.h, w.ctx.close())), ("graph free", lambda w: (w.graph.free(), w.graph.h, w.graph.free())),
    ("reads free", lambda w: (w.reads.free(), w.reads.h, w.reads.free())),
])
each("switch fails", [("set_mem_limit", lambda w: w.ctx.set_mem_limit(1))], script={"mgta_ctx_set_mem_limit": -2})
each("switch fails", [("set_search_share", lambda w: w.ctx.set_search_share(2, 1))], script={"mgta_ctx_set_search_share": -2})


@case("context create", script={"mgta_ctx_create": Handle("ctx")})
def _(w):
    c = api.Context(2)
    return c.h.name


@case("context create fails")
def _(w):
    return api.Context(0)


def probe_answer(objs, nth):
    if len(objs[2]) > 1:
        objs[2][1].gb_per_s, objs[2][1].pad_ = 2.5, 7
    return 0


each("probe_random_lines", [("none", lambda w: w.ctx.probe_random_lines(1 << 20, [])),
                            ("two", lambda w: w.ctx.probe_random_lines(1 << 20, iter([(1, 2, 3, 0, 100), (4.0, 5, 6, 1, 200)])))],
     script={"mgta_probe_random_lines": probe_answer})

each("detach_stream", [("empty", lambda w: w.ctx.detach_stream())])


def stream_sizes(objs, nth):
    objs[1].value, objs[2].value = 3, 2
    return 0


each("detach_stream", [("sized", lambda w: tuple(a.shape + (str(a.dtype),) for a in w.ctx.detach_stream()))], script={"mgta_stream_sizes": stream_sizes})
each("detach_stream", [("download fails", lambda w: w.ctx.detach_stream())], script={"mgta_stream_download": -1})

# ---- phase ------------------------------------------------------------------------------------------------------------------------
SITES = [[1, 4, 6], [], [2]]
each("phase_pairs", [("none", lambda w: api.Context.phase_pairs([])), ("sites", lambda w: api.Context.phase_pairs(SITES)),
                     ("max_span", lambda w: api.Context.phase_pairs(SITES, 3)), ("no sites", lambda w: api.Context.phase_pairs([[], []])),
                     ("negative site", lambda w: api.Context.phase_pairs([[-1]])), ("site too large", lambda w: api.Context.phase_pairs([[1 << 32]]))])


def place(w, n):
    from megagta_amd.pileup import READ_DTYPE
    return np.zeros(n, dtype=READ_DTYPE)


LIBS = [(3, True), (5, False)]
each("phase", [
    ("none", lambda w: w.ctx.phase(w.reads, place(w, 0), [], [], [])),
    ("lens", lambda w: w.ctx.phase(w.reads, place(w, 5), LIBS, [8, 3, np.int64(5)], SITES)),
    ("seqs", lambda w: w.ctx.phase(w.reads, place(w, 5), LIBS, ["ACGTACGT", b"ACG", "ACGTA"], SITES, params={}, reads_reversed=False)),
    ("records as a list", lambda w: w.ctx.phase(w.reads, [tuple(range(6))] * 5, LIBS, [8, 3, 5], SITES)),
    ("max_span", lambda w: w.ctx.phase(w.reads, place(w, 5), LIBS, [8, 3, 5], SITES, params={"max_span": 3})),
    ("joint_cap", lambda w: w.ctx.phase(w.reads, place(w, 5), LIBS, [8, 3, 5], SITES, joint_cap=7)),
    ("joint_cap 0", lambda w: w.ctx.phase(w.reads, place(w, 5), LIBS, [8, 3, 5], SITES, joint_cap=0)),
    ("libs empty", lambda w: w.ctx.phase(w.reads, place(w, 0), [], [8, 3, 5], SITES)),
    ("no sites", lambda w: w.ctx.phase(w.reads, place(w, 5), LIBS, [8, 3], [[], []])),
    ("unknown parameter", lambda w: w.ctx.phase(w.reads, place(w, 5), LIBS, [8, 3, 5], SITES, params={"max_span": 3, "min_span": 1, "a": 2})),
    ("sites and contigs differ", lambda w: w.ctx.phase(w.reads, place(w, 5), LIBS, [8, 3], SITES)),
    ("too few records", lambda w: w.ctx.phase(w.reads, place(w, 4), LIBS, [8, 3, 5], SITES)),
    ("other context", lambda w: w.ctx.phase(World().reads, place(w, 5), LIBS, [8, 3, 5], SITES)),
])


def phase_answer(objs, nth):
    objs[12][-1] = 2
    return 0


each("phase", [("pairs filled", lambda w: w.ctx.phase(w.reads, place(w, 5), LIBS, [8, 3, 5], SITES))], script={"mgta_reads_phase": phase_answer})

# ---- recruit ----------------------------------------------------------------------------------------------------------------------
each("recruit", [
    ("defaults", lambda w: w.ctx.recruit(w.hmm, w.reads)), ("no reads", lambda w: w.ctx.recruit(w.hmm, w.reads, n_short_reads=0)),
    ("n_short_reads", lambda w: w.ctx.recruit(w.hmm, w.reads, n_short_reads=3, reads_reversed=False)),
    ("no recs", lambda w: w.ctx.recruit(w.hmm, w.reads, recs=False)), ("no cols", lambda w: w.ctx.recruit(w.hmm, w.reads, cols=False)),
    ("neither", lambda w: w.ctx.recruit(w.hmm, w.reads, 70, recs=False, cols=False)), ("params {}", lambda w: w.ctx.recruit(w.hmm, w.reads, params={})),
    ("min_score", lambda w: w.ctx.recruit(w.hmm, w.reads, params={"min_aa": 7, "min_score": 2.5})),
    ("min_bits", lambda w: w.ctx.recruit(w.hmm, w.reads, params={"min_bits": 3})),
    ("both", lambda w: w.ctx.recruit(w.hmm, w.reads, params={"min_bits": 3, "min_score": 1.0})),
    ("unknown parameter", lambda w: w.ctx.recruit(w.hmm, w.reads, params={"min_bits": 3, "min_nats": 1.0})),
])


def recruit_answer(objs, nth):
    objs[6][0] = 0b10110
    objs[9].n_recruited_frame[2] = 3
    return 0


each("recruit", [("bits set", lambda w: w.ctx.recruit(w.hmm, w.reads))], script={"mgta_reads_recruit": recruit_answer})
each("recruit", [("model of no column", lambda w: w.ctx.recruit(w.hmm, w.reads))], M=0)

# ---- derep, align, posterior ----------------------------------------------------------------------------------------------------------
each("derep", [(tag, lambda w, s=s: w.ctx.derep(s)) for tag, s in SEQS.items()] + [("generator", lambda w: w.ctx.derep(iter(["AC", 5])))])
each("derep fails", [("str", lambda w: w.ctx.derep(["AC"]))], script={"mgta_seqs_derep": -3, "mgta_last_error": b"the library's sentence"})

each("align", [(f"{tag} cols={c:d} paths={p:d}", lambda w, s=s, c=c, p=p: w.ctx.align(w.hmm, s, cols=c, paths=p))
               for tag, s in SEQS.items() for c, p in ((True, False), (False, True))] +
     [("defaults", lambda w: w.ctx.align(w.hmm, SEQS["str"])), ("all", lambda w: w.ctx.align(w.hmm, SEQS["str"], True, True)),
      ("nothing", lambda w: w.ctx.align(w.hmm, SEQS["str"], False, False))])


def align_paths(objs, nth):
    p, plen = objs[7], objs[8]
    p[:3], plen[0] = list(b"MID"), 3
    p[3 + 3:3 + 3 + 2], plen[1] = list(b"MM"), 2                 # sequence 1 starts at offsets[1] + 1 * M
    return 0


each("align", [("paths filled", lambda w: w.ctx.align(w.hmm, SEQS["str"], paths=True))], script={"mgta_seqs_align": align_paths})

LABELS = [[1, -1, 2], [0, 3]]
each("posterior", [(f"{tag} cols={c:d}", lambda w, s=s, c=c: w.ctx.posterior(w.hmm, s, cols=c)) for tag, s in SEQS.items() for c in (True, False)] + [
    ("labels", lambda w: w.ctx.posterior(w.hmm, SEQS["str"], labels=LABELS)), ("labels no cols", lambda w: w.ctx.posterior(w.hmm, SEQS["bytes"], LABELS, cols=False)),
    ("labels none", lambda w: w.ctx.posterior(w.hmm, [], labels=[])), ("labels empty sequences", lambda w: w.ctx.posterior(w.hmm, ["", ""], labels=[[], []])),
    ("labels arrays", lambda w: w.ctx.posterior(w.hmm, SEQS["str"], labels=[np.array(l) for l in LABELS])),
    ("labels too few", lambda w: w.ctx.posterior(w.hmm, SEQS["str"], labels=LABELS[:1])),
    ("labels too short", lambda w: w.ctx.posterior(w.hmm, SEQS["str"], labels=[[1, 2], [0, 3]]))])


def posterior_pp(objs, nth):
    objs[7][:5] = [0.5, 0.25, 1.0, 0.75, 0.125]
    return 0


each("posterior", [("pp filled", lambda w: w.ctx.posterior(w.hmm, SEQS["str"], labels=LABELS))], script={"mgta_seqs_posterior": posterior_pp})

# ---- rows: pairs, clusters, trees ---------------------------------------------------------------------------------------------------
ROWS = {"array": np.frombuffer(b"MK-VMKLV-KLV", dtype=np.uint8).reshape(3, 4), "strings": ["MK-V", b"MKLV", "-KLV"], "none": [], "no rows array": np.zeros((0, 4), np.uint8),
        "non-ascii": ["MKéV", "MKLV"], "int64 array": np.arange(6, dtype=np.int64).reshape(2, 3), "strided": np.frombuffer(b"MK-VMKLV-KLV", dtype=np.uint8).reshape(3, 4)[:, ::2]}
BAD_ROWS = {"unequal": ["MK-V", "MKL"], "flat array": np.zeros(4, np.uint8), "wide character": ["MKŁV"]}
each("row_pairs", [(tag, lambda w, r=r: w.ctx.row_pairs(r, 2, 0.25)) for tag, r in {**ROWS, **BAD_ROWS}.items()])


def pairs_answer(second):
    def answer(objs, nth):
        objs[8].value = 3 if nth == 0 else second
        return 0
    return answer


each("row_pairs", [("count then fill", lambda w: w.ctx.row_pairs(ROWS["array"], 2, 0.25))], script={"mgta_rows_pairs": pairs_answer(3)})
each("row_pairs", [("counts differ", lambda w: w.ctx.row_pairs(ROWS["array"], 2, 0.25))], script={"mgta_rows_pairs": pairs_answer(2)})


def lens_of(r):
    return [4, 5, 6][:len(r)]


each("cluster", [(tag, lambda w, r=r: w.ctx.cluster(r, lens_of(r), 2, 0.03)) for tag, r in {**ROWS, "unequal": BAD_ROWS["unequal"]}.items()] + [
    ("lens array", lambda w: w.ctx.cluster(ROWS["array"], np.array([4, 5, 6], np.int32), 2, 0.03)), ("lens too few", lambda w: w.ctx.cluster(ROWS["array"], [4, 5], 2, 0.03)),
    ("lens 2-D", lambda w: w.ctx.cluster(ROWS["array"], [[4, 5, 6]], 2, 0.03))])
each("clusters", [(tag, lambda w, r=r: w.ctx.clusters(r, lens_of(r), 2, [0.01, 0.03])) for tag, r in {**ROWS, "unequal": BAD_ROWS["unequal"]}.items()] + [
    ("no cutoffs", lambda w: w.ctx.clusters(ROWS["array"], [4, 5, 6], 2, [])), ("one cutoff", lambda w: w.ctx.clusters(ROWS["strings"], [4, 5, 6], 2, np.array([0.5]))),
    ("cutoff a number", lambda w: w.ctx.clusters(ROWS["array"], [4, 5, 6], 2, 0.03)), ("lens too few", lambda w: w.ctx.clusters(ROWS["array"], [4, 5], 2, [0.03]))])
each("clusters", [("merges filled", lambda w: w.ctx.clusters(ROWS["array"], [4, 5, 6], 2, [0.01, 0.03]))], script={"mgta_rows_clusters": set_value(13, 2)})

PAIRS = [(0, 1, 1, 4), (0, 2, 0, 3), (1, 2, 2, 3)]
PAIR_ARRAY = np.array(PAIRS, dtype=api.ROW_PAIR)
MERGES = [(0, 2, 0, 1), (0, 1, 2, 3)]
each("pairs_tree", [("tuples", lambda w: w.ctx.pairs_tree(PAIRS, [4, 4, 3])), ("array", lambda w: w.ctx.pairs_tree(PAIR_ARRAY, np.array([4, 4, 3]))),
                    ("no pairs", lambda w: w.ctx.pairs_tree([], [4, 4, 3])), ("none", lambda w: w.ctx.pairs_tree([], [])),
                    ("n_residues 2-D", lambda w: w.ctx.pairs_tree(PAIRS, [[4, 4, 3]]))])
each("pairs_tree", [("merges filled", lambda w: w.ctx.pairs_tree(PAIRS, [4, 4, 3]))], script={"mgta_pairs_tree": set_value(7, 2)})
each("link_pairs", [("tuples", lambda w: api.link_pairs(PAIRS, [4, 4, 3], [9, 8, 7])), ("array", lambda w: api.link_pairs(PAIR_ARRAY, np.array([4, 4, 3]), np.array([9, 8, 7]))),
                    ("no pairs", lambda w: api.link_pairs([], [4, 0, 3], [9, 8, 7])), ("none", lambda w: api.link_pairs([], [], [])),
                    ("lens too few", lambda w: api.link_pairs(PAIRS, [4, 4, 3], [9, 8])), ("n_residues 2-D", lambda w: api.link_pairs(PAIRS, [[4, 4, 3]], [9, 8, 7]))])
each("tree_cut", [("tuples", lambda w: api.tree_cut(PAIRS, MERGES, [4, 4, 3], [9, 8, 7], 0.5)),
                  ("arrays", lambda w: api.tree_cut(PAIR_ARRAY, np.array(MERGES, dtype=api.TREE_MERGE), np.array([4, 4, 3]), np.array([9, 8, 7]), 0.7)),
                  ("no merges", lambda w: api.tree_cut(PAIRS, [], [4, 4, 3], [9, 8, 7], 0)), ("none", lambda w: api.tree_cut([], [], [], [], 0.5)),
                  ("lens too few", lambda w: api.tree_cut(PAIRS, MERGES, [4, 4, 3], [9, 8], 0.5))])

# ---- nearest, frameshift, chimera ----------------------------------------------------------------------------------------------------
REFS = {"none": [], "str": ["MKLV", "MK"], "bytes": [b"MKLV"], "non-ascii": ["Mé"]}
SEQ_REF = [("none", "none"), ("none", "str"), ("str", "none"), ("str", "str"), ("bytes", "bytes"), ("non-ascii", "non-ascii")]
each("nearest", [(f"{s}/{r} scores={sc:d} paths={p:d}", lambda w, s=s, r=r, sc=sc, p=p: w.ctx.nearest(SEQS[s], REFS[r], SUB, 11, 1, scores=sc, paths=p))
                 for s, r in SEQ_REF for sc, p in ((False, False), (True, True))] +
     [("scores", lambda w: w.ctx.nearest(SEQS["str"], REFS["str"], SUB, 11, 1, scores=True)), ("paths", lambda w: w.ctx.nearest(SEQS["str"], REFS["str"], SUB, 11, 1, paths=True)),
      ("table int64", lambda w: w.ctx.nearest(SEQS["str"], REFS["str"], SUB.astype(np.int64), 11.0, True)), ("table 26", lambda w: w.ctx.nearest(SEQS["str"], REFS["str"], SUB[:26, :26], 11, 1)),
      ("wide character", lambda w: w.ctx.nearest(["MŁ"], REFS["str"], SUB, 11, 1))])
each("frameshift", [(f"{s}/{r} scores={sc:d} paths={p:d}", lambda w, s=s, r=r, sc=sc, p=p: w.ctx.frameshift(CONTIGS[s], REFS[r], SUB, 11, 1, 15, scores=sc, paths=p))
                    for s, r in (("none", "none"), ("none", "str"), ("two", "none"), ("two", "str"), ("bytes", "bytes"), ("non-ascii", "non-ascii")) for sc, p in ((False, False), (True, True))] +
     [("scores", lambda w: w.ctx.frameshift(CONTIGS["two"], REFS["str"], SUB, 11, 1, 15, scores=True)), ("paths", lambda w: w.ctx.frameshift(CONTIGS["two"], REFS["str"], SUB, 11, 1, 15, paths=True)),
      ("table 26", lambda w: w.ctx.frameshift(CONTIGS["two"], REFS["str"], SUB[:26], 11, 1, 15))])
each("chimera", [(f"{s}/{r} tops={t:d}", lambda w, s=s, r=r, t=t: w.ctx.chimera(SEQS[s], REFS[r], SUB, 11, 1, 5, 6, tops=t)) for s, r in SEQ_REF for t in (False, True)] +
     [("table 26", lambda w: w.ctx.chimera(SEQS["str"], REFS["str"], SUB.T[:, :26], 11, 1, 5, 6))])


def nearest_paths(objs, nth):
    p, plen = objs[-3], objs[-2]
    p[:2], plen[0] = list(b"MD"), 2
    p[3 + 4096:3 + 4096 + 3], plen[1] = list(b"I<>"), 3
    return 0


each("nearest", [("paths filled", lambda w: w.ctx.nearest(SEQS["str"], REFS["str"], SUB, 11, 1, paths=True))], script={"mgta_seqs_nearest": nearest_paths})
each("frameshift", [("paths filled", lambda w: w.ctx.frameshift(["ACG", "AC"], REFS["str"], SUB, 11, 1, 15, paths=True))], script={"mgta_seqs_frameshift": nearest_paths})

# ---- reads and the build --------------------------------------------------------------------------------------------------------------
each("upload_reads", [("none", lambda w: w.ctx.upload_reads(np.zeros(0, np.uint32), [0])), ("two", lambda w: w.ctx.upload_reads([7, 9], np.array([0, 20, 31]))),
                      ("adopt", lambda w: w.ctx.adopt_reads(0, 5, 0, 2, keepalive="kept"))])


def build_sink(objs, nth):
    sink = objs[8]
    if sink:
        bc = (C.c_int64 * 6)(2, 1, 1, 1, 0, 0)
        r, lg, tp = (C.c_uint16 * 3)(5, 6, 7), (C.c_uint16 * 1)(300), (C.c_uint32 * 3)(1, 2, 3)
        sink(None, 4, 6, bc, r, 3, lg, 1, tp, 3)
        sink(None, 6, 7, bc, C.cast(None, C.POINTER(C.c_uint16)), 0, lg, 0, C.cast(None, C.POINTER(C.c_uint32)), 0)
    objs[10].n_edges = 3
    return 0


each("build_sdbg", [("defaults", lambda w: w.ctx.build_sdbg(w.reads, 5)), ("not collected", lambda w: w.ctx.build_sdbg(w.reads, 5, collect=False)),
                    ("all arguments", lambda w: w.ctx.build_sdbg(w.reads, 21, 2, True, True, 3, (16, 32)))], script={"mgta_sdbg_last_emit_fused": set_value(1, 4)})
each("build_sdbg", [("sink called", lambda w: w.ctx.build_sdbg(w.reads, 5))], script={"mgta_sdbg_build_resident": build_sink})
each("export_records_to_torch", [("none", lambda w: api.export_records_to_torch(w.ctx))])
each("export_records_to_torch", [("three", lambda w: api.export_records_to_torch(w.ctx))], script={"mgta_sdbg_export_records_device": set_value(3, 3)})

# ---- the graph ------------------------------------------------------------------------------------------------------------------------
STREAM = api.EdgeStream(k=4, words_per_tip=1, bucket_items=np.arange(65536) < 3, records=[5, 6, 7], large=np.array([300]), tips=np.array([9], np.uint64))
each("graph", [(f"{tag} multiplicity={m:d}", fn) for m in (False, True) for tag, fn in (
    ("resident", lambda w, m=m: api.Graph(w.ctx, None, 9, keep_multiplicity=m)), ("stream", lambda w, m=m: api.Graph(w.ctx, STREAM, keep_multiplicity=m)),
    ("files", lambda w, m=m: api.Graph.from_files(w.ctx, "some/prefix", keep_multiplicity=m)))] + [
    ("stream, context keeps multiplicity", lambda w: (w.ctx.keep_multiplicity(True), api.Graph(w.ctx, STREAM))[1]),
    ("files, context keeps multiplicity", lambda w: (w.ctx.keep_multiplicity(True), api.Graph.from_files(w.ctx, "p", True))[1])],
     script={"mgta_sdbg_size": 130})
each("graph load fails", [("files", lambda w: api.Graph.from_files(w.ctx, "p", True))], script={"mgta_sdbg_load_files": -1})
each("outgoing", [("none", lambda w: w.graph.outgoing([])), ("three", lambda w: tuple(a.shape + (str(a.dtype),) for a in w.graph.outgoing([3, 1, 2])))])
each("navigate", [("rank_last", lambda w: w.graph.navigate("rank_last", [3, 4])), ("rank_w scalar symbol", lambda w: w.graph.navigate("rank_w", [3, 4], 2)),
                  ("select_w symbols", lambda w: w.graph.navigate("select_w", np.array([[3], [4]]), [1, 2])), ("outgoing", lambda w: w.graph.navigate("outgoing", [3, 4, 5])),
                  ("incoming", lambda w: w.graph.navigate("incoming", 7)), ("out_fd", lambda w: w.graph.navigate("out_fd", [3, 4], [0, 1], -1)),
                  ("label", lambda w: w.graph.navigate("label", [3, 4])), ("none", lambda w: w.graph.navigate("forward", [])), ("label none", lambda w: w.graph.navigate("label", [])),
                  ("unknown", lambda w: w.graph.navigate("sideways", [1]))])
each("index_edges", [("none", lambda w: w.graph.index_edges([]).shape), ("two", lambda w: w.graph.index_edges(["ACGTA", "acgnxTT"]).shape)])
each("invalid_bits", [("130 edges", lambda w: w.graph.invalid_bits())])
each("edge_multiplicity", [("none", lambda w: w.graph.edge_multiplicity([]).shape), ("two", lambda w: w.graph.edge_multiplicity(np.array([1, 2], np.int32)).shape)])
each("contig_coverage", [(f"{tag} per_window={pw:d} abundance={ab:d}", lambda w, s=s, pw=pw, ab=ab: w.graph.contig_coverage(s, per_window=pw, abundance=ab))
                         for tag, s in CONTIGS.items() for pw, ab in ((False, True), (True, False))] + [("defaults", lambda w: w.graph.contig_coverage(CONTIGS["two"]))])
each("contig_share_coverage", [(f"{tag} per_window={pw:d}", lambda w, s=s, pw=pw: w.graph.contig_share_coverage(s, per_window=pw)) for tag, s in CONTIGS.items() for pw in (False, True)])
each("match_reads", [(f"{tag} counts={c:d}", lambda w, s=s, c=c: w.graph.match_reads(w.reads, s, counts=c)) for tag, s in CONTIGS.items() for c in (False, True)] + [
    ("n_short_reads", lambda w: w.graph.match_reads(w.reads, CONTIGS["two"], 3, counts=True, reads_reversed=False)),
    ("no reads", lambda w: w.graph.match_reads(w.reads, CONTIGS["two"], 0, counts=True)), ("70 reads", lambda w: w.graph.match_reads(w.reads, CONTIGS["two"], 70))])


def match_answer(objs, nth):
    objs[7][0] = 0b01001
    return 0


each("match_reads", [("bits set", lambda w: w.graph.match_reads(w.reads, CONTIGS["two"]))], script={"mgta_reads_match_contigs": match_answer})
each("contig_sample_coverage", [(f"{tag} per_window={pw:d}", lambda w, s=s, pw=pw: w.graph.contig_sample_coverage(w.reads, [2, 5], s, per_window=pw)) for tag, s in CONTIGS.items() for pw in (False, True)] + [
    (f"lib_end empty, {tag} per_window={pw:d}", lambda w, s=s, pw=pw: w.graph.contig_sample_coverage(w.reads, [], s, per_window=pw, reads_reversed=False)) for tag, s in (("none", []), ("two", CONTIGS["two"])) for pw in (False, True)] + [
    ("lib_end array", lambda w: w.graph.contig_sample_coverage(w.reads, np.array([5], np.int32), CONTIGS["two"])), ("lib_end 2-D", lambda w: w.graph.contig_sample_coverage(w.reads, [[2, 5]], CONTIGS["two"]))])

FULL_PILEUP = {"min_anchors": 2, "min_overlap": 30, "max_mismatch_permille": 50}
FULL_GAPPED = {**FULL_PILEUP, "max_gap": 3, "gap_open": 4, "gap_extend": 1}
for name, full in (("pileup", FULL_PILEUP), ("pileup_gapped", FULL_GAPPED)):
    each(name, [(f"{tag} per_read={pr:d}", lambda w, s=s, pr=pr, name=name: getattr(w.graph, name)(w.reads, s, per_read=pr)) for tag, s in CONTIGS.items() for pr in (False, True)] + [
        ("n_short_reads", lambda w, name=name: getattr(w.graph, name)(w.reads, CONTIGS["two"], 3, per_read=True, reads_reversed=False)),
        ("no reads", lambda w, name=name: getattr(w.graph, name)(w.reads, CONTIGS["two"], 0, per_read=True)),
        ("params {}", lambda w, name=name: getattr(w.graph, name)(w.reads, CONTIGS["two"], params={})),
        ("params full", lambda w, name=name, full=full: getattr(w.graph, name)(w.reads, CONTIGS["two"], params=full)),
        ("params one", lambda w, name=name: getattr(w.graph, name)(w.reads, CONTIGS["two"], params={"min_overlap": 25.0})),
        ("unknown parameter", lambda w, name=name, full=full: getattr(w.graph, name)(w.reads, CONTIGS["two"], params={**full, "max_gaps": 1, "Min_anchors": 2}))])
each("pileup", [("gapped parameter", lambda w: w.graph.pileup(w.reads, CONTIGS["two"], params={"max_gap": 3}))])


def gapped_answer(objs, nth):
    objs[14].n_gap_placements = 40 if nth == 0 else 3
    return -1 if nth == 0 else 0


each("pileup_gapped", [("gap_cap", lambda w: w.graph.pileup_gapped(w.reads, CONTIGS["two"], gap_cap=8)), ("gap_cap 0", lambda w: w.graph.pileup_gapped(w.reads, CONTIGS["two"], gap_cap=0)),
                       ("400 reads", lambda w: w.graph.pileup_gapped(w.reads, CONTIGS["two"], 400))])
each("pileup_gapped", [("one retry", lambda w: w.graph.pileup_gapped(w.reads, CONTIGS["two"], per_read=True)), ("gap_cap given, no retry", lambda w: w.graph.pileup_gapped(w.reads, CONTIGS["two"], gap_cap=8))],
     script={"mgta_reads_pileup_gapped": gapped_answer})
each("pileup_gapped", [("fails twice", lambda w: w.graph.pileup_gapped(w.reads, CONTIGS["two"]))], script={"mgta_reads_pileup_gapped": lambda objs, nth: (setattr(objs[14], "n_gap_placements", 40), -1)[1]})
each("pileup_gapped", [("fails otherwise", lambda w: w.graph.pileup_gapped(w.reads, CONTIGS["two"]))], script={"mgta_reads_pileup_gapped": -2})

TEXT = C.create_string_buffer(b">c\nACGT\n", 8)


def denovo_answer(objs, nth):
    objs[4].value, objs[5].value, objs[6].n_contigs = C.addressof(TEXT), 8, 1
    return 0


each("denovo", [("no text", lambda w: w.graph.denovo()), ("arguments", lambda w: w.graph.denovo(20, True, 46))])
each("denovo", [("text", lambda w: w.graph.denovo())], script={"mgta_denovo": denovo_answer})

# ---- models and the search ------------------------------------------------------------------------------------------------------------
MODEL = types.SimpleNamespace(M=2, A=20, msc=np.zeros((3, 20)), tsc=[[0.5] * 7] * 3, max_match=np.zeros(3, np.float32), h=np.zeros(3), alpha=np.arange(26))
each("hmm", [("load", lambda w: api.DeviceHmm(w.ctx, MODEL))])
each("hmm", [("free", lambda w: (lambda m: (m.free(), m.h, m.free()))(api.DeviceHmm(w.ctx, MODEL)))], script={"mgta_hmm_load": set_value(8, 0x1000)})
KMERS = ["ACGTA", "ccgtaTT"]


def astar_sink(objs, nth):
    side = _lib.AstarSide()
    side.ok, side.state, side.length, side.real_score = 1, ord("m"), 4, 1.5
    objs[9](None, 1, b"ACxx", 2, b"GTT", 3, C.byref(side), C.byref(_lib.AstarSide()))
    objs[9](None, 0, b"", 0, b"", 0, C.byref(_lib.AstarSide()), C.byref(side))
    objs[11].n_seeds = 2
    return 0


def search(fn, w, kmers, states, *a, **kw):
    return fn(w.graph, w.hmm, w.rev, kmers, states, *a, **kw)


for name, fn in (("astar_search", api.astar_search), ("astar_search_packed", api.astar_search_packed)):
    each(name, [("none", lambda w, fn=fn: search(fn, w, [], [])), ("two", lambda w, fn=fn: search(fn, w, KMERS, [3, 7])),
                ("arguments", lambda w, fn=fn: search(fn, w, KMERS, np.array([3, 7]), 25, 0.25, 4, 1000)), ("cost rate negative", lambda w, fn=fn: search(fn, w, KMERS, [3, 7], cost_rate=-2)),
                ("cost curve", lambda w, fn=fn: search(fn, w, KMERS, [3, 7], cost_rate=(1000, 5000, 100))), ("cost curve without knee", lambda w, fn=fn: search(fn, w, KMERS, [3, 7], cost_rate=[1000, 0, 100])),
                ("short k-mer", lambda w, fn=fn: search(fn, w, ["ACGTA", "ACGT"], [3, 7])), ("non-ascii k-mer", lambda w, fn=fn: search(fn, w, ["ACGéA"], [3]))])
each("astar_search", [("sink called", lambda w: search(api.astar_search, w, KMERS, [3, 7]))], script={"mgta_astar_batch": astar_sink})


def search_on(w, kmers, states, *a, own=False, answer=None, **kw):
    """astar_search(..., run=): on a second context of the world's library (own: on the graph's own, named).  Its handle is another object
    of the same name, so the records cannot tell the two contexts apart; the stand-in does: it answers MGTA_EINVAL (-2) unless the cost
    rate is set on the run context and the batch is given the run context's handle first and the graph's second."""
    run = w.ctx
    if not own:
        run = api.Context.__new__(api.Context)
        run._L, run.h = w.lib, Handle("ctx")

    def cost(objs, nth):
        return 0 if objs[0] is run.h else -2

    def batch(objs, nth):
        if objs[0] is not run.h or objs[1] is not w.graph.h:
            return -2
        return answer(objs[1:], nth) if answer else 0

    w.lib.script.update(mgta_ctx_set_search_cost_rate=cost, mgta_ctx_set_search_cost_curve=cost, mgta_astar_batch_on=batch)
    return api.astar_search(w.graph, w.hmm, w.rev, kmers, states, *a, run=run, **kw)


each("astar_search on", [("none", lambda w: search_on(w, [], [])), ("two", lambda w: search_on(w, KMERS, [3, 7])),
                         ("arguments", lambda w: search_on(w, KMERS, np.array([3, 7]), 25, 0.25, 4, 1000)),
                         ("cost curve", lambda w: search_on(w, KMERS, [3, 7], cost_rate=(1000, 5000, 100))),
                         ("the graph's own context", lambda w: search_on(w, KMERS, [3, 7], cache_mode=1, own=True)),
                         ("short k-mer", lambda w: search_on(w, ["ACGTA", "ACGT"], [3, 7])),
                         ("sink called", lambda w: search_on(w, KMERS, [3, 7], answer=astar_sink)),
                         ("fails", lambda w: search_on(w, KMERS, [3, 7], answer=lambda objs, nth: -6))])
PACKED_TEXT = C.create_string_buffer(b"ACacgtaGTT", 10)


def packed_answer(objs, nth):
    objs[9].value = C.addressof(PACKED_TEXT)
    objs[10][:] = [0, 7, 10]
    return 0


each("astar_search_packed", [("sides", lambda w: search(api.astar_search_packed, w, KMERS, [3, 7], want_sides=True)), ("no seeds, sides", lambda w: search(api.astar_search_packed, w, [], [], want_sides=True))])
each("astar_search_packed", [("text", lambda w: search(api.astar_search_packed, w, KMERS, [3, 7])), ("text and sides", lambda w: search(api.astar_search_packed, w, KMERS, [3, 7], want_sides=True))],
     script={"mgta_astar_batch_packed": packed_answer})

# ---- findstart ------------------------------------------------------------------------------------------------------------------------
WORDS = np.array([[1, 0], [2, 0], [3, 4]], dtype=np.uint64)


def findstart_answer(total):
    def answer(objs, nth):
        hits = objs[6]
        if total <= len(hits):
            for i in range(total):
                hits[i].read, hits[i].pos_strand, hits[i].ref = 10 + i, 2 * i + 1, i % 3
        objs[8].value, objs[9].value = total, 0.5
        return 0
    return answer


each("find_hits", [("none", lambda w: findstart.find_hits(w.ctx, w.reads, True, 45, np.zeros((0, 2), np.uint64))), ("no hits", lambda w: findstart.find_hits(w.ctx, w.reads, False, 45, WORDS))])
each("find_hits", [("three hits", lambda w: findstart.find_hits(w.ctx, w.reads, True, 45, WORDS.astype(np.int64)))], script={"mgta_findstart": findstart_answer(3)})
each("find_hits", [("more hits than the capacity", lambda w: findstart.find_hits(w.ctx, w.reads, True, 45, WORDS))], script={"mgta_findstart": findstart_answer((1 << 16) + 5)})


# ---- recording ------------------------------------------------------------------------------------------------------------------------
def run_case(script, world, fn) -> dict:
    w = World(script, **world)
    saved = _lib.load, sys.modules.get("torch")
    _lib.load, sys.modules["torch"] = (lambda: w.lib), FAKE_TORCH
    try:
        try:
            out = dict(returned=value_record(fn(w)))
        except Exception as e:                                       # (what a wrapper raises is part of what it does)
            out = dict(raised=type(e).__name__, message=str(e))
    finally:
        _lib.load = saved[0]
        if saved[1] is None:
            del sys.modules["torch"]
        else:
            sys.modules["torch"] = saved[1]
        w.lib.recording = False                                       # (the stand-ins free themselves later: not part of the case)
    return dict(calls=w.lib.calls, **out)


def run_table() -> dict:
    return {name: run_case(script, world, fn) for name, script, world, fn in CASES}


def text_of(records: dict) -> str:
    """the file: the same few hundred argument and value records recur in every case, so each is written once under "values" and a case
    names it by [its index]: a call is [name, argument, ...], an argument a scalar, "null" or such a reference; what was returned is a
    reference, its members (one level down) references too.  One value, one case per line."""
    values = {}

    def ref(rec):
        return [values.setdefault(json.dumps(rec, sort_keys=True), len(values))] if isinstance(rec, dict) else rec

    def returned(v):
        kind, body = next(iter(v.items())) if isinstance(v, dict) and len(v) == 1 else (None, None)
        if kind == "dict":
            return ref({"dict": [[k, ref(x)] for k, x in body]})
        return ref({kind: [ref(x) for x in body]}) if kind in ("list", "tuple") else ref(v)

    cases = []
    for name in sorted(records):
        rec = records[name]
        out = dict(calls=[[c["fn"]] + [ref(a) for a in c["args"]] for c in rec["calls"]])
        out.update(dict(returned=returned(rec["returned"])) if "returned" in rec else dict(raised=rec["raised"], message=rec["message"]))
        cases.append(f'  {json.dumps(name)}: {json.dumps(out, sort_keys=True, separators=(",", ":"))}')
    return '{\n "values": [\n' + ",\n".join("  " + json.dumps(json.loads(v), sort_keys=True, separators=(",", ":")) for v in values) + '\n ],\n "cases": {\n' + ",\n".join(cases) + "\n }\n}\n"


def load_golden(path: str = GOLDEN) -> dict:
    """the records of the file as run_table() gives them"""
    with open(path) as f:
        packed = json.load(f)
    values = packed["values"]

    def deref(x):
        return values[x[0]] if isinstance(x, list) else x

    def returned(x):
        v = deref(x)
        kind, body = next(iter(v.items())) if isinstance(v, dict) and len(v) == 1 else (None, None)
        if kind == "dict":
            return {"dict": [[k, deref(m)] for k, m in body]}
        return {kind: [deref(m) for m in body]} if kind in ("list", "tuple") else v

    records = {}
    for name, rec in packed["cases"].items():
        out = dict(calls=[dict(fn=c[0], args=[deref(a) for a in c[1:]]) for c in rec["calls"]])
        out.update(dict(returned=returned(rec["returned"])) if "returned" in rec else dict(raised=rec["raised"], message=rec["message"]))
        records[name] = out
    return records


if __name__ == "__main__":
    records = run_table()
    with open(GOLDEN, "w") as f:
        f.write(text_of(records))
    print(f"{len(records)} records, {sum(len(r['calls']) for r in records.values())} calls -> {GOLDEN}")
