#!/usr/bin/env python3
"""tools/bench_qc.py [out.json] -- what the per-position read statistics cost on the device (LiME_fasta --qc-report, lime_docs_qc_dev: DESIGN.md
section 9 f17), a side benchmark (bench.py stays the yardstick).  One session, one box, the page cache warm.  The input is tools/bench_trim.py's
FASTQ pair: bench_fasta.py's two files of 750 000 reads of 100 bases with that file's qualities and seed.
  (a) one call, on reads_1 parsed with its qualities, HIP events, the three alternating, best of 5 rounds after a warm-up round: one docs_qc
      call (256 positions), one docs_filter call with bench_filter.py's parameters (the nearest per-read pass there is), and a device-to-device
      copy of the text and the quality bytes (the bytes the statistics must read: the floor)
  (b) the kernel alone: a child process, `bench_qc.py --calls DIR`, makes six docs_qc calls under `rocprofv3 --kernel-trace --stats`, a run of
      its own ("skipped" with the reason where there is no rocprofv3)
  (c) `LiME_fasta --readlen auto --trim-qual 20,20 --trim-polyx G --min-len 30` on the pair with and without `--qc-report`: whole processes
      (the HIP runtime's start included), alternating, best of 5 after a warm-up; the two classification files are compared
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

from lime_amd import _lib, api  # noqa: E402
import bench_fasta as BF  # noqa: E402
import bench_filter as BL  # noqa: E402
import bench_trim as BT  # noqa: E402

N_POS = 256
REPS = 5
TRACED_CALLS = 6
STAGES = ["--trim-qual", f"{BT.Q5},{BT.Q3}", "--trim-polyx", "G", "--min-len", "30"]


def calls(ctx, d):
    """(a): the three calls, alternating, the best of REPS rounds each after a warm-up round"""
    nd, nt = d.info()
    text, _ = d.device()
    qual = d.qual_device()
    dst = torch.empty(2 * nt, dtype=torch.uint8, device="cuda")
    tables = np.zeros(api.qc_words(N_POS), dtype=np.uint64)

    def copy():
        _lib.hip_memcpy_d2d(dst.data_ptr(), text, nt)
        _lib.hip_memcpy_d2d(dst.data_ptr() + nt, qual, nt)

    best = {}
    for k in range(REPS + 1):
        for key, fn in (("qc", lambda: ctx.docs_qc(d, N_POS, tables=tables)), ("filter", lambda: ctx.docs_filter(d, **BL.FLT)[0].close()), ("d2d_copy_text_and_qual", copy)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if k:
                best[key] = min(best.get(key, 1e30), a.elapsed_time(b))
    res = {"n_docs": nd, "n_text": nt, "positions": N_POS, "qc": BF.rate(2 * nt, best["qc"]), "filter": BF.rate(nt, best["filter"]),
           "d2d_copy_text_and_qual": BF.rate(2 * nt, best["d2d_copy_text_and_qual"])}
    res["qc_over_filter"] = round(best["qc"] / best["filter"], 3)
    res["qc_over_copy"] = round(best["qc"] / best["d2d_copy_text_and_qual"], 3)
    return res


def traced_calls(d):
    """the child of (b): TRACED_CALLS calls on reads_1 of directory d"""
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    docs = ctx.docs_from_fastq_qual(os.path.join(d, "raw_1.fastq"))
    for _ in range(TRACED_CALLS):
        ctx.docs_qc(docs, N_POS)
    docs.close()
    ctx.close()


def kernel_trace(d):
    """(b): the kernel's calls and its average, smallest and largest time in microseconds"""
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
        if "k_qc_reads" in row["Name"]:
            res["k_qc_reads"] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 1), "min_us": round(float(row["MinNs"]) / 1e3, 1),
                                 "max_us": round(float(row["MaxNs"]) / 1e3, 1)}
    return res or {"skipped": "no k_qc_reads in the trace"}


def end_to_end(d):
    exe = os.path.join(BF.BIN, "LiME_fasta")
    base = [exe, os.path.join(d, "raw_1.fastq"), os.path.join(d, "raw_2.fastq"), "--gidx", os.path.join(d, "g.gidx"), "--lineage", os.path.join(d, "LineageFile.csv"),
            "--readlen", "auto"] + STAGES
    runs = [("stages_with_qc_report", base + ["--qc-report", os.path.join(d, "qc.json")]), ("stages_alone", base)]
    best = {}
    for k in range(REPS + 1):
        for key, cmd in runs:
            ms = BF.timed(cmd + ["--out", os.path.join(d, key + ".txt")], d)
            if k:
                best[key] = min(best.get(key, ms), ms)
    files = [open(os.path.join(d, key + ".txt"), "rb").read() for key, _ in runs]
    rep = json.load(open(os.path.join(d, "qc.json")))
    return {"ms": best, "with_over_without": round(best["stages_with_qc_report"] / best["stages_alone"], 3), "classification_equal": files[0] == files[1],
            "classification_lines": files[0].count(b"\n") - 1, "report_bytes": os.path.getsize(os.path.join(d, "qc.json")),
            "report_reads": [[f["before"]["reads"], f["after"]["reads"]] for f in rep["files"]],
            "report_symbols": [[f["before"]["symbols"], f["after"]["symbols"]] for f in rep["files"]]}


def main():
    args = sys.argv[1:]
    if args[:1] == ["--calls"]:
        return traced_calls(args[1])
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    res = {"stages": STAGES}
    genomes, reads, lineage = BF.synthetic()
    rng = np.random.default_rng(313)                                        # bench_trim.py's seed: its pair
    with tempfile.TemporaryDirectory() as d:
        for m, rows in enumerate(reads):
            open(os.path.join(d, f"raw_{m + 1}.fastq"), "wb").write(BT.fastq_with(rows, BT.qualities(rng, len(rows))))
        docs = ctx.docs_from_fastq_qual(os.path.join(d, "raw_1.fastq"))
        print("the pair is written; timing the calls", file=sys.stderr, flush=True)
        res["calls"] = calls(ctx, docs)
        docs.close()
        ctx.close()
        print("calls:", res["calls"], "; tracing the kernel", file=sys.stderr, flush=True)
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
