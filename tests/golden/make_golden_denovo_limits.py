"""Golden vectors for `megagta denovo` on the designed graphs of tests/denovo_shapes.py (GOLDEN_SHAPES), made like those of
make_golden_denovo.py, with the reference binary run with ONE thread:
    python tests/golden/make_golden_denovo_limits.py          (build container only: needs oracle/_ref/megagta)
Writes tests/golden/denovo_limits/<shape>.fa.gz (the reads) and tests/golden/denovo_limits/expected.json:
{shape: {"k", "min_count", "runs": [{"max_tip_len", "no_bubble", "min_contig", "contigs": text of PREFIX.contigs.fa, "info": text of .info}]}}
A text of more than 16 KB (the fans: thousands of random continuations) is kept as "contigs_sha256", the SHA-256 of its bytes, instead."""
import gzip, hashlib, json, os, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import denovo_shapes  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "megagta")
OUT = os.path.join(HERE, "denovo_limits")


def main():
    run = lambda cmd: subprocess.run(cmd, check=True, capture_output=True)
    os.makedirs(OUT, exist_ok=True)
    out = {}
    for name in denovo_shapes.GOLDEN_SHAPES:
        reads, info = denovo_shapes.make(name)
        k = info["k"]
        w = tempfile.mkdtemp()
        fa = os.path.join(w, "reads.fa")
        with open(fa, "w") as f:
            for i, r in enumerate(reads):
                f.write(f">{i}\n{r}\n")
        with open(fa, "rb") as f, gzip.GzipFile(os.path.join(OUT, name + ".fa.gz"), "wb", compresslevel=9, mtime=0) as z:
            z.write(f.read())
        with open(os.path.join(w, "reads.lib"), "w") as f:
            f.write(f"reads.fa\nse {fa}\n")
        run([REF, "buildlib", os.path.join(w, "reads.lib"), os.path.join(w, "reads.lib")])
        run([REF, "buildgraph", "-k", str(k), "-m", "1", "--host_mem", "4000000000", "--mem_flag", "1", "--gpu_mem", "0", "--num_cpu_threads", "4",
             "--num_output_threads", "1", "--read_lib_file", os.path.join(w, "reads.lib"), "--output_prefix", os.path.join(w, "g")])
        runs = []
        for tip, nob, minc in info["runs"]:
            run([REF, "denovo", "-s", os.path.join(w, "g"), "-o", os.path.join(w, "o"), "-t", "1", "--max_tip_len", str(tip), "--min_contig", str(minc)]
                + (["--no_bubble"] if nob else []))
            text = open(os.path.join(w, "o.contigs.fa")).read()
            kept = dict(contigs=text) if len(text) <= 16384 else dict(contigs_sha256=hashlib.sha256(text.encode()).hexdigest())
            runs.append(dict(max_tip_len=tip, no_bubble=nob, min_contig=minc, **kept, info=open(os.path.join(w, "o.contigs.fa.info")).read()))
            print(name, tip, nob, minc, runs[-1]["info"].strip())
        out[name] = dict(k=k, min_count=1, runs=runs)
    with open(os.path.join(OUT, "expected.json"), "w") as f:
        json.dump(out, f, indent=0)


if __name__ == "__main__":
    main()
