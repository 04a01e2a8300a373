#!/usr/bin/env python3
"""tools/bench_trim.py [out.json] -- what trimming the reads by quality on the device costs (LiME_fasta --trim-qual, lime_docs_from_fastq_qual*,
lime_docs_trim_dev: DESIGN.md section 9 f13), a side benchmark (bench.py stays the yardstick).  One session, one box, the page cache warm.
The input is tools/bench_fasta.py's `reads` (10 random genomes of 2.5 * 10^6 bases, two files of 750 000 reads of 100 bases) written as
four-line FASTQ with the qualities of tests/trim_cases.py's generator, drawn in numpy: the middle 30 .. 40, a low tail of 1 .. 60 symbols on
55 % of the reads (a third of them with a low head of 1 .. 8), 5 % low throughout, 5 % low on all but 5 symbols.  Cutoffs 20,20.
  (a) on reads_1's bytes in HBM, HIP events, best of 5 after a warm-up: docs_from_fastq_qual_bytes_dev + docs_trim (and each alone) against
      docs_from_fastq_bytes_dev of the same bytes and against a device-to-device hipMemcpy of them
  (b) `LiME_fasta --readlen auto --trim-qual 20,20` on the raw pair against `LiME_fasta --readlen auto` on the pair trimmed beforehand: whole
      processes (the HIP runtime's start included), alternating, best of 5 after a warm-up; the two classification files are compared
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

Q5, Q3 = 20, 20
REPS = 5


def qualities(rng, n, L=BF.READ_LEN):
    """the generator's shape, a matrix at a time -> uint8 [n][L] of Phred+33 bytes"""
    q = rng.integers(30, 41, size=(n, L))
    low = rng.integers(2, 15, size=(n, L))
    u = rng.random(n)
    pos = np.arange(L)[None, :]
    all_low = u < 0.05
    but5 = (u >= 0.05) & (u < 0.10)
    keep5 = np.zeros((n, L), dtype=bool)                                    # 5 positions per such read
    rows = np.nonzero(but5)[0]
    keep5[rows] = rng.random((len(rows), L)).argsort(axis=1) < 5
    tail = (u >= 0.10) & (u < 0.65)
    k = rng.integers(1, 61, size=n)[:, None]
    head = tail & (rng.random(n) < 1 / 3)
    h = rng.integers(1, 9, size=n)[:, None]
    is_low = all_low[:, None] | (but5[:, None] & ~keep5) | (tail[:, None] & (pos >= L - k)) | (head[:, None] & (pos < h))
    return (np.where(is_low, low, q) + 33).astype(np.uint8)


def fastq_with(reads, quals):
    """bench_fasta.fastq_of_reads with these quality bytes"""
    n = len(reads)
    rec = np.frombuffer(BF.fastq_of_reads(reads), np.uint8).reshape(n, -1).copy()
    rec[:, 113:113 + BF.READ_LEN] = quals
    return rec.tobytes()


def fastq_of_docs(text, off):
    """variable-length reads as four-line FASTQ with constant qualities"""
    raw = text.tobytes()
    return b"".join(b"@r%07d\n%s\n+\n%s\n" % (i, raw[int(off[i]):int(off[i + 1])], b"I" * int(off[i + 1] - off[i])) for i in range(len(off) - 1))


def event_ms(fn):
    """best of REPS after a warm-up, HIP events on the default stream"""
    best = None
    for k in range(REPS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if k and (best is None or ms < best):
            best = ms
    return best


def trimmed_docs(ctx, data):
    d = ctx.docs_from_fastq_qual_bytes(data)
    out, _ = ctx.docs_trim(d, Q5, Q3)
    got = out.get()
    out.close(); d.close()
    return got


def kernels(ctx, data):
    n = len(data)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    dst = torch.empty_like(t)
    res = {"input_bytes": n}

    def both():
        d = ctx.docs_from_fastq_qual_bytes_dev(t)
        out, _ = ctx.docs_trim(d, Q5, Q3)
        out.close(); d.close()

    res["plain_parse"] = BF.rate(n, event_ms(lambda: ctx.docs_from_fastq_bytes_dev(t).close()))
    res["parse_with_qualities"] = BF.rate(n, event_ms(lambda: ctx.docs_from_fastq_qual_bytes_dev(t).close()))
    d = ctx.docs_from_fastq_qual_bytes_dev(t)
    res["trim"] = BF.rate(n, event_ms(lambda: ctx.docs_trim(d, Q5, Q3)[0].close()))
    out, info = ctx.docs_trim(d, Q5, Q3)
    res["trim_info"] = info
    res["n_docs"], res["n_text"] = d.info()
    res["parse_with_qualities_and_trim"] = BF.rate(n, event_ms(both))
    res["d2d_memcpy"] = BF.rate(n, event_ms(lambda: _lib.hip_memcpy_d2d(dst.data_ptr(), t.data_ptr(), n)))
    res["over_plain_parse"] = round(res["parse_with_qualities_and_trim"]["ms"] / res["plain_parse"]["ms"], 3)
    res["over_d2d_memcpy"] = round(res["parse_with_qualities_and_trim"]["ms"] / res["d2d_memcpy"]["ms"], 3)
    out.close(); d.close()
    return res


def end_to_end(d):
    exe = os.path.join(BF.BIN, "LiME_fasta")
    tail = ["--gidx", os.path.join(d, "g.gidx"), "--lineage", os.path.join(d, "LineageFile.csv"), "--readlen", "auto"]
    runs = [("trim_qual_on_raw", [exe, os.path.join(d, "raw_1.fastq"), os.path.join(d, "raw_2.fastq")] + tail + ["--trim-qual", f"{Q5},{Q3}"]),
            ("readlen_auto_on_pretrimmed", [exe, os.path.join(d, "cut_1.fastq"), os.path.join(d, "cut_2.fastq")] + tail)]
    best = {}
    for k in range(REPS + 1):
        for key, cmd in runs:
            ms = BF.timed(cmd + ["--out", os.path.join(d, key + ".txt")], d)
            if k:
                best[key] = min(best.get(key, ms), ms)
    files = [open(os.path.join(d, key + ".txt"), "rb").read() for key, _ in runs]
    return {"ms": best, "over_pretrimmed": round(best["trim_qual_on_raw"] / best["readlen_auto_on_pretrimmed"], 3), "classification_equal": files[0] == files[1],
            "classification_lines": files[0].count(b"\n") - 1}


def main():
    args = sys.argv[1:]
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    res = {"cutoffs": [Q5, Q3]}
    genomes, reads, lineage = BF.synthetic()
    rng = np.random.default_rng(313)
    with tempfile.TemporaryDirectory() as d:
        for m, rows in enumerate(reads):
            data = fastq_with(rows, qualities(rng, len(rows)))
            open(os.path.join(d, f"raw_{m + 1}.fastq"), "wb").write(data)
            if m == 0:
                res["kernels"] = kernels(ctx, data)
            text, off = trimmed_docs(ctx, data)
            open(os.path.join(d, f"cut_{m + 1}.fastq"), "wb").write(fastq_of_docs(text, off))
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
