#!/usr/bin/env python3
"""tools/bench_overlap.py [out.json] -- what cutting a pair's adapter read-through from the mates' overlap on the device costs (LiME_fasta
--trim-overlap, lime_docs_trim_overlap_dev: DESIGN.md section 9 f16), a side benchmark (bench.py stays the yardstick).  One session, one box,
the page cache warm.  The input is tools/bench_fasta.py's reads_1 (750 000 reads of 100 bases of 10 random genomes) made into 750 000 pairs
the way tests/test_overlap_sample_gpu.py makes them, drawn in numpy: the fragment is the read's first I symbols (random bases behind it), I in
20 .. 140; mate 1 reads it into the R1 TruSeq adapter and random bases, mate 2 reads its reverse complement into the R2 adapter; 2 % of mate
1's symbols are changed.  Overlap 30, error rate 10 %.
  (a) on the parsed pair in HBM, HIP events, alternating, best of 5 rounds after a warm-up: one docs_trim_overlap call on the pair next to one
      docs_trim_adapter call (tools/bench_adapter.py's: overlap 3, 10 %) on mate 1 alone, in the same process
  (b) the kernels alone: a child process, `bench_overlap.py --calls DIR`, makes six calls of each, alternating, under `rocprofv3 --kernel-trace
      --stats`, a run of its own; k_overlap_bounds, k_adapter_bounds and k_trim_copy are read from its kernel statistics (absent where there is
      no rocprofv3)
  (c) `LiME_fasta --readlen auto --trim-overlap 30` on the raw pair against `LiME_fasta --readlen auto` on the pair cut beforehand: whole
      processes (the HIP runtime's start included), alternating, best of 5 after a warm-up; the two classification files are compared
Prints one JSON line (and writes it to out.json if given)."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lime_amd import api  # noqa: E402
import bench_adapter as BA  # noqa: E402
import bench_fasta as BF  # noqa: E402
import bench_trim as BT  # noqa: E402

OVERLAP, ERROR = 30, 10
REPS = 5
TRACED_CALLS = 6


def pairs(rng, reads):
    """uint8 [n][L] -> (mate 1, mate 2), uint8 [n][L] each: read-through pairs of the fragment reads[:, :I] (random bases behind L)"""
    n, L = reads.shape
    sym = np.frombuffer(b"ACGT", np.uint8)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    ext = np.concatenate([reads, sym[rng.integers(0, 4, size=(n, 40))]], axis=1)
    insert = rng.integers(20, L + 41, size=n)[:, None]
    j = np.arange(L)[None, :]
    mates = []
    for m, frag in enumerate((ext[:, :L], comp[np.take_along_axis(ext, np.clip(insert - 1 - j, 0, L + 39), axis=1)])):
        M = len(BA.ADAPTERS[m])
        ad = np.frombuffer(BA.ADAPTERS[m], np.uint8)[np.clip(j - insert, 0, M - 1)]
        filler = sym[rng.integers(0, 4, size=(n, L))]
        mates.append(np.where(j < insert, frag, np.where(j - insert < M, ad, filler)).astype(np.uint8))
    mates[0] = np.where(rng.random((n, L)) < 0.02, sym[rng.integers(0, 4, size=(n, L))], mates[0]).astype(np.uint8)
    return mates


def calls(ctx, d1, d2):
    """(a): the two calls, alternating, the best of REPS rounds each after a warm-up round"""
    n1, n2 = d1.info()[1], d2.info()[1]
    best = {}
    for k in range(REPS + 1):
        for key, fn in (("overlap_trim", lambda: [x.close() for x in ctx.docs_trim_overlap(d1, d2, OVERLAP, ERROR)[:2]]),
                        ("adapter_trim", lambda: ctx.docs_trim_adapter(d1, BA.ADAPTERS[0], BA.OVERLAP, BA.ERROR)[0].close())):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if k:
                best[key] = min(best.get(key, 1e30), a.elapsed_time(b))
    res = {"overlap_trim": BF.rate(n1 + n2, best["overlap_trim"]), "adapter_trim": BF.rate(n1, best["adapter_trim"])}
    res["overlap_trim_over_adapter_trim"] = round(best["overlap_trim"] / best["adapter_trim"], 3)
    return res


def traced_calls(d):
    """the child of (b): TRACED_CALLS calls of each, alternating, on the raw pair of directory d"""
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    d1, d2 = (ctx.docs_from_file(os.path.join(d, f"raw_{m}.fastq")) for m in (1, 2))
    for _ in range(TRACED_CALLS):
        for x in ctx.docs_trim_overlap(d1, d2, OVERLAP, ERROR)[:2]:
            x.close()
        ctx.docs_trim_adapter(d1, BA.ADAPTERS[0], BA.OVERLAP, BA.ERROR)[0].close()
    ctx.close()


def kernel_trace(d):
    """(b): per kernel the calls and the average, smallest and largest time in microseconds"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return {"skipped": "no rocprofv3"}
    out = os.path.join(d, "trace")
    p = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--calls", d],
                       capture_output=True, cwd=d)
    found = glob.glob(out + "/**/*kernel_stats.csv", recursive=True)
    if p.returncode != 0 or not found:
        return {"skipped": f"rocprofv3 ended with {p.returncode}: {p.stderr.decode()[-300:]}"}
    res = {}
    for row in csv.DictReader(open(max(found, key=os.path.getmtime))):
        for name in ("k_overlap_bounds", "k_adapter_bounds", "k_trim_copy"):
            if name in row["Name"]:
                res[name] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 1), "min_us": round(float(row["MinNs"]) / 1e3, 1),
                             "max_us": round(float(row["MaxNs"]) / 1e3, 1)}
    if "k_overlap_bounds" in res and "k_adapter_bounds" in res:
        res["k_overlap_bounds_over_k_adapter_bounds"] = round(res["k_overlap_bounds"]["avg_us"] / res["k_adapter_bounds"]["avg_us"], 2)
    return res


def end_to_end(d):
    exe = os.path.join(BF.BIN, "LiME_fasta")
    tail = ["--gidx", os.path.join(d, "g.gidx"), "--lineage", os.path.join(d, "LineageFile.csv"), "--readlen", "auto"]
    runs = [("trim_overlap_on_raw", [exe, os.path.join(d, "raw_1.fastq"), os.path.join(d, "raw_2.fastq")] + tail + ["--trim-overlap", f"{OVERLAP},{ERROR}"]),
            ("readlen_auto_on_precut", [exe, os.path.join(d, "cut_1.fastq"), os.path.join(d, "cut_2.fastq")] + tail)]
    best = {}
    for k in range(REPS + 1):
        for key, cmd in runs:
            ms = BF.timed(cmd + ["--out", os.path.join(d, key + ".txt")], d)
            if k:
                best[key] = min(best.get(key, ms), ms)
    files = [open(os.path.join(d, key + ".txt"), "rb").read() for key, _ in runs]
    return {"ms": best, "over_precut": round(best["trim_overlap_on_raw"] / best["readlen_auto_on_precut"], 3), "classification_equal": files[0] == files[1],
            "classification_lines": files[0].count(b"\n") - 1}


def main():
    args = sys.argv[1:]
    if args[:1] == ["--calls"]:
        return traced_calls(args[1])
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    res = {"overlap": OVERLAP, "error": ERROR, "adapter_overlap": BA.OVERLAP, "adapter_error": BA.ERROR}
    genomes, reads, lineage = BF.synthetic()
    rng = np.random.default_rng(316)
    with tempfile.TemporaryDirectory() as d:
        mates = pairs(rng, np.asarray(reads[0]))
        for m, rows in enumerate(mates):
            open(os.path.join(d, f"raw_{m + 1}.fastq"), "wb").write(BF.fastq_of_reads(rows))
        d1, d2 = (ctx.docs_from_file(os.path.join(d, f"raw_{m}.fastq")) for m in (1, 2))
        res["n_pairs"], res["n_text"] = d1.info()[0], d1.info()[1] + d2.info()[1]
        o1, o2, res["overlap_info"] = ctx.docs_trim_overlap(d1, d2, OVERLAP, ERROR)
        for m, o in enumerate((o1, o2)):
            open(os.path.join(d, f"cut_{m + 1}.fastq"), "wb").write(BT.fastq_of_docs(*o.get()))
            o.close()
        print("the pair is written and cut; timing the calls", file=sys.stderr, flush=True)
        res["calls"] = calls(ctx, d1, d2)
        d1.close(); d2.close()
        ctx.close()
        print("calls:", res["calls"], "; tracing the kernels", file=sys.stderr, flush=True)
        res["kernels"] = kernel_trace(d)
        print("kernels:", res["kernels"], "; the whole programs", file=sys.stderr, flush=True)
        open(os.path.join(d, "refs.fasta"), "wb").write(BF.fasta_of_genomes(genomes))
        open(os.path.join(d, "LineageFile.csv"), "wb").write(lineage)
        res["index_ms"] = BF.timed([os.path.join(BF.BIN, "BuildIndex"), "--refs", os.path.join(d, "refs.fasta"), os.path.join(d, "g")], d)
        res["end_to_end"] = end_to_end(d)
    line = json.dumps(res)
    print(line, flush=True)
    if len(args) > 0:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
