#!/usr/bin/env python3
"""tools/bench_filter.py [out.json] -- what filtering the reads on the device costs (LiME_fasta --trim-polyx / --max-n / --min-complexity /
--min-len, lime_docs_filter_dev: DESIGN.md section 9 f15), a side benchmark (bench.py stays the yardstick).  One session, one box, the page cache warm.
  (a) the filter pass alone, on the documents tools/bench_adapter.py times its pass on -- bench_fasta.py's reads_1 with that file's
      read-through planted by its `planted` and its seed, parsed by docs_from_fastq_bytes_dev -- HIP events, best of 5 after a warm-up: one
      docs_filter call with every step on (poly-G tails of 10, at most 5 N's, 30 % complexity, 30 symbols) against one docs_trim_adapter
      call on the same documents in the same process, and the same filter call on those reads with G tails and N's planted
  (b) `LiME_fasta --readlen auto --trim-polyx G --max-n 5 --min-complexity 30 --min-len 30` on a raw pair against `LiME_fasta --readlen auto`
      on the pair filtered beforehand: bench_fasta.py's two files with a G tail of 15 .. 50 symbols (5 % of them wrong) on every fourth read,
      six N's in the middle of every fiftieth and every hundredth only A; whole processes (the HIP runtime's start included), alternating,
      best of 5 after a warm-up; the two classification files are compared
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

from lime_amd import api  # noqa: E402
import bench_adapter as BA  # noqa: E402
import bench_fasta as BF  # noqa: E402
import bench_trim as BT  # noqa: E402

FLT = dict(polyx="G", polyx_min=10, max_len=0, min_len=30, max_n=5, min_complexity=30)
FLAGS = ["--trim-polyx", "G", "--max-n", "5", "--min-complexity", "30", "--min-len", "30"]
REPS = 5


def with_tails(rng, reads):
    """uint8 [n][L] -> the same with a G tail of 15 .. 50 symbols (5 % of them other bases, never the first) on every fourth read, six N's
    in the middle of every fiftieth and every hundredth only A"""
    n, L = reads.shape
    out = reads.copy()
    t = rng.integers(15, 51, size=n)[:, None]
    j = np.arange(L)[None, :] - (L - t)                                     # the place in the tail, where j >= 0
    miss = (rng.random((n, L)) < 0.05) & (j > 0)
    tail = np.where(miss, ord("A"), ord("G")).astype(np.uint8)
    rows = (np.arange(n) % 4 == 0)[:, None]
    out = np.where(rows & (j >= 0), tail, out)
    out[1::50, L // 2 - 3:L // 2 + 3] = ord("N")
    out[2::100, :] = ord("A")
    return out.astype(np.uint8)


def filtered_docs(ctx, data):
    d = ctx.docs_from_fastq_bytes(data)
    out, info = ctx.docs_filter(d, **FLT)
    got = out.get()
    out.close(); d.close()
    return got, info


def kernels(ctx, rows, tailed):
    res = {}
    for key, r in (("adapter_bench_documents", rows), ("tails_planted", tailed)):
        t = torch.from_numpy(np.frombuffer(BF.fastq_of_reads(r), np.uint8).copy()).cuda()
        d = ctx.docs_from_fastq_bytes_dev(t)
        nd, nt = d.info()
        one = {"n_docs": nd, "n_text": nt}
        one["filter"] = BF.rate(nt, BT.event_ms(lambda: ctx.docs_filter(d, **FLT)[0].close()))
        one["adapter_trim"] = BF.rate(nt, BT.event_ms(lambda: ctx.docs_trim_adapter(d, BA.ADAPTERS[0], BA.OVERLAP, BA.ERROR)[0].close()))
        one["tail_only"] = BF.rate(nt, BT.event_ms(lambda: ctx.docs_filter(d, polyx="G")[0].close()))
        one["counts_only"] = BF.rate(nt, BT.event_ms(lambda: ctx.docs_filter(d, max_n=5, min_complexity=30)[0].close()))
        out, info = ctx.docs_filter(d, **FLT)
        one["filter_info"] = info
        out.close(); d.close()
        one["filter_over_adapter_trim"] = round(one["filter"]["ms"] / one["adapter_trim"]["ms"], 3)
        res[key] = one
    return res


def end_to_end(d):
    exe = os.path.join(BF.BIN, "LiME_fasta")
    tail = ["--gidx", os.path.join(d, "g.gidx"), "--lineage", os.path.join(d, "LineageFile.csv"), "--readlen", "auto"]
    runs = [("filter_on_raw", [exe, os.path.join(d, "raw_1.fastq"), os.path.join(d, "raw_2.fastq")] + tail + FLAGS),
            ("readlen_auto_on_prefiltered", [exe, os.path.join(d, "done_1.fastq"), os.path.join(d, "done_2.fastq")] + tail)]
    best = {}
    for k in range(REPS + 1):
        for key, cmd in runs:
            ms = BF.timed(cmd + ["--out", os.path.join(d, key + ".txt")], d)
            if k:
                best[key] = min(best.get(key, ms), ms)
    files = [open(os.path.join(d, key + ".txt"), "rb").read() for key, _ in runs]
    return {"ms": best, "over_prefiltered": round(best["filter_on_raw"] / best["readlen_auto_on_prefiltered"], 3), "classification_equal": files[0] == files[1],
            "classification_lines": files[0].count(b"\n") - 1}


def main():
    args = sys.argv[1:]
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    res = {"filter": FLT}
    genomes, reads, lineage = BF.synthetic()
    rng_a = np.random.default_rng(314)                                      # bench_adapter.py's seed: its documents of reads_1
    rng = np.random.default_rng(315)
    with tempfile.TemporaryDirectory() as d:
        for m, rows in enumerate(reads):
            tailed = with_tails(rng, np.asarray(rows))
            if m == 0:
                res["kernels"] = kernels(ctx, BA.planted(rng_a, np.asarray(rows), BA.ADAPTERS[0]), tailed)
            data = BF.fastq_of_reads(tailed)
            open(os.path.join(d, f"raw_{m + 1}.fastq"), "wb").write(data)
            (text, off), info = filtered_docs(ctx, data)
            res[f"reads_{m + 1}"] = info
            open(os.path.join(d, f"done_{m + 1}.fastq"), "wb").write(BT.fastq_of_docs(text, off))
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
