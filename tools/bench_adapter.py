#!/usr/bin/env python3
"""tools/bench_adapter.py [out.json] -- what cutting the reads at their adapters on the device costs (LiME_fasta --trim-adapter,
lime_docs_trim_adapter_dev: DESIGN.md section 9 f14), a side benchmark (bench.py stays the yardstick).  One session, one box, the page cache warm.
The input is tools/bench_fasta.py's `reads` (10 random genomes of 2.5 * 10^6 bases, two files of 750 000 reads of 100 bases) with read-through
planted the way tests/test_adapter_sample_gpu.py plants it, drawn in numpy: every read's insert is cut at a length in 20 .. 100, the TruSeq
adapter of its mate with 5 % of its symbols changed follows, then random bases up to 100 symbols.  Overlap 3, error rate 10 %.
  (a) on reads_1 in HBM, HIP events, best of 5 after a warm-up: one docs_trim_adapter call on the parsed documents against
      docs_from_fastq_bytes_dev of the file's bytes (the plain parse), against docs_trim (the quality trim, cutoffs 20,20, of the same reads
      with tools/bench_trim.py's qualities) and against a device-to-device hipMemcpy of the documents' text
  (b) `LiME_fasta --readlen auto --trim-adapter A1,A2` on the raw pair against `LiME_fasta --readlen auto` on the pair trimmed beforehand:
      whole processes (the HIP runtime's start included), alternating, best of 5 after a warm-up; the two classification files are compared
Prints one JSON line (and writes it to out.json if given)."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lime_amd import _lib, api  # noqa: E402
import bench_fasta as BF  # noqa: E402
import bench_trim as BT  # noqa: E402

ADAPTERS = (b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT")
OVERLAP, ERROR = 3, 10
REPS = 5


def planted(rng, reads, adapter):
    """uint8 [n][L] -> the same with read-through: the insert, the adapter with 5 % of its symbols changed, random bases"""
    n, L = reads.shape
    M = len(adapter)
    sym = np.frombuffer(b"ACGT", np.uint8)
    insert = rng.integers(20, L + 1, size=n)[:, None]
    j = np.arange(L)[None, :] - insert                                      # the place in the adapter, where 0 <= j < M
    ad = np.frombuffer(adapter, np.uint8)[np.clip(j, 0, M - 1)]
    other = np.frombuffer(bytes(adapter).translate(bytes.maketrans(b"ACGT", b"CATG")), np.uint8)[np.clip(j, 0, M - 1)]
    ad = np.where(rng.random((n, L)) < 0.05, other, ad)
    filler = sym[rng.integers(0, 4, size=(n, L))]
    return np.where(j < 0, reads, np.where(j < M, ad, filler)).astype(np.uint8)


def trimmed_docs(ctx, data, adapter):
    d = ctx.docs_from_fastq_bytes(data)
    out, info = ctx.docs_trim_adapter(d, adapter, OVERLAP, ERROR)
    got = out.get()
    out.close(); d.close()
    return got, info


def kernels(ctx, rows, adapter, rng):
    data = BF.fastq_of_reads(rows)
    n = len(data)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    res = {"input_bytes": n}
    res["plain_parse"] = BF.rate(n, BT.event_ms(lambda: ctx.docs_from_fastq_bytes_dev(t).close()))
    d = ctx.docs_from_fastq_bytes_dev(t)
    res["n_docs"], res["n_text"] = d.info()
    nt = res["n_text"]
    res["adapter_trim"] = BF.rate(nt, BT.event_ms(lambda: ctx.docs_trim_adapter(d, adapter, OVERLAP, ERROR)[0].close()))
    out, info = ctx.docs_trim_adapter(d, adapter, OVERLAP, ERROR)
    res["adapter_info"] = info
    # what the call must move: the text and 8 bytes of doc_off per read in; 8 bytes of bounds per read out and in again, 4 of new offsets out
    # and in; the kept text in and out, 8 bytes of doc_off per read out
    res["adapter_trim_bytes"] = {"bounds_kernel": nt + 16 * res["n_docs"], "whole_call": nt + 16 * res["n_docs"] + 24 * res["n_docs"] + 2 * info["symbols_out"] + 8 * res["n_docs"]}
    out.close()
    src = torch.from_numpy(rows.reshape(-1).copy()).cuda()
    dst = torch.empty_like(src)
    res["d2d_memcpy_of_the_text"] = BF.rate(nt, BT.event_ms(lambda: _lib.hip_memcpy_d2d(dst.data_ptr(), src.data_ptr(), nt)))
    qd = ctx.docs_from_fastq_qual_bytes(BT.fastq_with(rows, BT.qualities(rng, len(rows))))
    res["quality_trim"] = BF.rate(nt, BT.event_ms(lambda: ctx.docs_trim(qd, BT.Q5, BT.Q3)[0].close()))
    qd.close(); d.close()
    for k in ("plain_parse", "quality_trim", "d2d_memcpy_of_the_text"):
        res["adapter_trim_over_" + k] = round(res["adapter_trim"]["ms"] / res[k]["ms"], 3)
    return res


def end_to_end(d):
    exe = os.path.join(BF.BIN, "LiME_fasta")
    tail = ["--gidx", os.path.join(d, "g.gidx"), "--lineage", os.path.join(d, "LineageFile.csv"), "--readlen", "auto"]
    runs = [("trim_adapter_on_raw", [exe, os.path.join(d, "raw_1.fastq"), os.path.join(d, "raw_2.fastq")] + tail + ["--trim-adapter", (ADAPTERS[0] + b"," + ADAPTERS[1]).decode()]),
            ("readlen_auto_on_pretrimmed", [exe, os.path.join(d, "cut_1.fastq"), os.path.join(d, "cut_2.fastq")] + tail)]
    best = {}
    for k in range(REPS + 1):
        for key, cmd in runs:
            ms = BF.timed(cmd + ["--out", os.path.join(d, key + ".txt")], d)
            if k:
                best[key] = min(best.get(key, ms), ms)
    files = [open(os.path.join(d, key + ".txt"), "rb").read() for key, _ in runs]
    return {"ms": best, "over_pretrimmed": round(best["trim_adapter_on_raw"] / best["readlen_auto_on_pretrimmed"], 3), "classification_equal": files[0] == files[1],
            "classification_lines": files[0].count(b"\n") - 1}


def main():
    args = sys.argv[1:]
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    res = {"adapters": [a.decode() for a in ADAPTERS], "overlap": OVERLAP, "error": ERROR}
    genomes, reads, lineage = BF.synthetic()
    rng = np.random.default_rng(314)
    with tempfile.TemporaryDirectory() as d:
        for m, rows in enumerate(reads):
            rows = planted(rng, np.asarray(rows), ADAPTERS[m])
            data = BF.fastq_of_reads(rows)
            open(os.path.join(d, f"raw_{m + 1}.fastq"), "wb").write(data)
            if m == 0:
                res["kernels"] = kernels(ctx, rows, ADAPTERS[m], rng)
            (text, off), info = trimmed_docs(ctx, data, ADAPTERS[m])
            res[f"reads_{m + 1}"] = info
            open(os.path.join(d, f"cut_{m + 1}.fastq"), "wb").write(BT.fastq_of_docs(text, off))
        open(os.path.join(d, "refs.fasta"), "wb").write(BF.fasta_of_genomes(genomes))
        open(os.path.join(d, "LineageFile.csv"), "wb").write(lineage)
        res["index_ms"] = BF.timed([os.path.join(BF.BIN, "BuildIndex"), "--refs", os.path.join(d, "refs.fasta"), os.path.join(d, "g")], d)
        res["end_to_end"] = end_to_end(d)
    ctx.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
