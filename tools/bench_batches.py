#!/usr/bin/env python3
"""tools/bench_batches.py [out.json] -- what classifying a sample in batches of reads costs (LiME_fasta --batch-reads, lime_seq_reader,
lime_classify_sample_stream: DESIGN.md section 9 f10), a side benchmark (bench.py stays the yardstick).  One session, one box, the page
cache warm.  The input is tools/bench_fasta.py's `reads`: 10 random genomes of 2.5 * 10^6 bases, two files of 750 000 reads of 100
bases, written as four-line FASTQ and as FASTA; the genome index is built once and not counted.
  (a) wall clock of `LiME_fasta reads_1.fastq reads_2.fastq --gidx` whole and with --batch-reads 750 000, 250 000, 50 000 and 10 000:
      whole processes (the HIP runtime's start included), alternating, best of 3 after a warm-up; every classification file is compared
      with the whole run's in the same run
  (b) the reader alone against docs_from_file on reads_1, FASTQ and FASTA: the file read to its end in batches of 750 000 and 50 000
      records (the extra count pass, the cut's read-back and the parse per batch), best of 3 after a warm-up
  (c) the per-batch fixed cost: classify_sample on the FIRST read pair alone against the same index (the genome-side pass of the merge and
      the scan over the genome positions, times four collections), best of 3 after a warm-up; and the slope of (a) over the batch count
Prints one JSON line (and writes it to out.json if given)."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from lime_amd import api  # noqa: E402
import bench_fasta as BF  # noqa: E402

BATCHES = (750_000, 250_000, 50_000, 10_000)
N_READS = 750_000


def end_to_end(d):
    exe = os.path.join(BF.BIN, "LiME_fasta")
    base = [exe, os.path.join(d, "reads_1.fastq"), os.path.join(d, "reads_2.fastq"), "--gidx", os.path.join(d, "g.gidx"), "--lineage",
            os.path.join(d, "LineageFile.csv"), "--readlen", str(BF.READ_LEN)]
    runs = [("whole", [])] + [(str(b), ["--batch-reads", str(b)]) for b in BATCHES]
    best = {}
    for k in range(4):
        for key, extra in runs:
            ms = BF.timed(base + ["--out", os.path.join(d, "out_" + key + ".txt")] + extra, d)
            if k:
                best[key] = min(best.get(key, ms), ms)
    whole = open(os.path.join(d, "out_whole.txt"), "rb").read()
    res = {"ms": best, "over_whole": {key: round(best[key] / best["whole"], 3) for key, _ in runs[1:]},
           "classification_equal": {key: open(os.path.join(d, "out_" + key + ".txt"), "rb").read() == whole for key, _ in runs[1:]},
           "classification_lines": whole.count(b"\n") - 1}
    # the slope over the batch count between the two smallest batch sizes: what one more batch costs
    n = lambda b: -(-N_READS // b)
    res["ms_per_extra_batch"] = round((best["10000"] - best["50000"]) / (n(10_000) - n(50_000)), 3)
    return res


def reader_alone(ctx, path):
    def read_all(batch):
        r = ctx.seq_reader(path)
        n = 0
        while True:
            b = r.next(batch)
            if b is None:
                break
            n += b[0].info()[0]
            b[0].close()
        r.close()
        assert n == N_READS
    size = os.path.getsize(path)
    res = {"input_bytes": size, "docs_from_file": BF.rate(size, BF.best_of(lambda: ctx.docs_from_file(path).close()))}
    for batch in (750_000, 50_000):
        res["reader_batches_of_%d" % batch] = BF.rate(size, BF.best_of(lambda: read_all(batch)))
    return res


def fixed_cost(ctx, d):
    gi = ctx.load_genome_index(os.path.join(d, "g.gidx"))
    tx = api.Taxonomy(os.path.join(d, "LineageFile.csv"), 1, False, gi.info()["n_docs"])
    readers = [ctx.seq_reader(os.path.join(d, f), 1 << 20) for f in ("reads_1.fastq", "reads_2.fastq")]
    one = [r.next(1)[0] for r in readers]
    for r in readers:
        r.close()
    assert one[0].info()[0] == 1
    ms = BF.best_of(lambda: ctx.classify_sample(one, gi, tx, 16, BF.READ_LEN + 1 - 16, 0.25))
    res = {"classify_sample_on_one_pair_ms": round(ms, 3), "genome_positions": gi.info()["positions"]}
    for x in one:
        x.close()
    gi.close()
    tx.close()
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    res = {"bench": "batches", "device": torch.cuda.get_device_name(0), "reads": 2 * N_READS, "batch_reads": list(BATCHES)}
    genomes, reads, lineage = BF.synthetic()
    with tempfile.TemporaryDirectory() as d:
        for name, rows in zip(("reads_1", "reads_2"), reads):
            open(os.path.join(d, name + ".fasta"), "wb").write(BF.fasta_of_reads(rows))
            open(os.path.join(d, name + ".fastq"), "wb").write(BF.fastq_of_reads(rows))
        open(os.path.join(d, "refs.fasta"), "wb").write(BF.fasta_of_genomes(genomes))
        open(os.path.join(d, "LineageFile.csv"), "wb").write(lineage)
        res["index_ms"] = BF.timed([os.path.join(BF.BIN, "BuildIndex"), "--refs", os.path.join(d, "refs.fasta"), os.path.join(d, "g")], d)
        res["reader"] = {"fastq": reader_alone(ctx, os.path.join(d, "reads_1.fastq")), "fasta": reader_alone(ctx, os.path.join(d, "reads_1.fasta"))}
        res["per_batch_fixed"] = fixed_cost(ctx, d)
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
