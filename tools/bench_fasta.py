#!/usr/bin/env python3
"""tools/bench_fasta.py [out.json] [--skip-big-chain] -- FASTA to documents on the device (lime_docs_from_*, lime_docs_revcomp) next to
the host parser (lime_fasta_read), and bin/LiME_fasta end to end next to the chain it replaces (BuildIndex --gidx four times, then
LiME_paired), a side benchmark (bench.py stays the yardstick).  One session, one box, the page cache warm, best of 3 after a warm-up.

Two inputs:
  example   the reads of tests/golden/example_full.npz (2 x 10 000 reads of 100 bases) and its three surrogate genomes
  reads     10 random genomes of 2.5 * 10^6 bases; two files of 750 000 reads of 100 bases sampled from them with 1 % substitutions
Per input:
  (a) device parse of reads_1 from bytes resident in HBM (lime_docs_from_bytes_dev), from the file (lime_docs_from_fasta: file -> pinned
      staging -> HBM -> parse) and the device reverse complement: ms, and GB/s of input bytes
  (b) lime_fasta_read on the same file with rc 0 and rc 1: ms, GB/s
  (c) wall clock of `LiME_fasta reads_1 reads_2 --gidx` and of every step of the chain on the same files (whole processes, the HIP
      runtime's start included); the two classification files are compared; LiME_fasta's own phases from one more run.  --skip-big-chain leaves (c) out for `reads` (its chain writes 3.6 GB of .ebwt / .lcp / .da files).
  (d) the same reads written as four-line FASTQ (222 bytes per record), in the same run: (a) without the reverse complement and (b) with
      lime_docs_from_fastq* / lime_fastq_read, under "fastq"; and `LiME_fasta reads_1.fastq reads_2.fastq --gidx` next to the FASTA pair's run,
      alternating, the two classification files compared, under "fastq_end_to_end_ms" (measured for both inputs, with or without the chain)
Prints one JSON line after each input, the last one complete (and writes it to out.json if given)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lime_amd import _lib, api  # noqa: E402
import make_golden_classify as MC  # noqa: E402
import make_golden_example as G  # noqa: E402

BIN = os.path.join(ROOT, "lime_amd", "bin")
READ_LEN = 100


def now():
    torch.cuda.synchronize()
    return time.perf_counter()


def best_of(fn, reps=3):
    best = None
    for k in range(reps + 1):
        t0 = now()
        fn()
        dt = now() - t0
        if k and (best is None or dt < best):
            best = dt
    return best * 1e3


def rate(n_bytes, ms):
    return {"ms": round(ms, 3), "GBps": round(n_bytes / ms / 1e6, 3)}


def fasta_of_reads(reads):
    """uint8 [n][100] -> the bytes of a FASTA file with a 10-byte header line per read (111 bytes per record)"""
    n = len(reads)
    rec = np.empty((n, 10 + READ_LEN + 1), dtype=np.uint8)
    rec[:, 0] = ord(">")
    rec[:, 1] = ord("r")
    idx = np.arange(n)
    for k in range(7):
        rec[:, 8 - k] = ord("0") + (idx // 10 ** k) % 10
    rec[:, 9] = 10
    rec[:, 10:10 + READ_LEN] = reads
    rec[:, -1] = 10
    return rec.tobytes()


def fastq_of_reads(reads):
    """the same reads as four-line FASTQ: the same 10-byte header line with '@', '+', qualities that cycle through '!' .. 'I' (222 bytes per record)"""
    n = len(reads)
    rec = np.empty((n, 10 + READ_LEN + 1 + 2 + READ_LEN + 1), dtype=np.uint8)
    rec[:, :10 + READ_LEN + 1] = np.frombuffer(fasta_of_reads(reads), np.uint8).reshape(n, -1)
    rec[:, 0] = ord("@")
    rec[:, 111] = ord("+")
    rec[:, 112] = 10
    rec[:, 113:113 + READ_LEN] = 33 + (np.arange(n)[:, None] * 7 + np.arange(READ_LEN)[None, :]) % 41
    rec[:, -1] = 10
    return rec.tobytes()


def fasta_of_genomes(genomes):
    out = []
    for k, g in enumerate(genomes):
        out.append(b">genome%d\n" % k)
        out.extend(g[o:o + 60] + b"\n" for o in range(0, len(g), 60))
    return b"".join(out)


def synthetic():
    rng = np.random.default_rng(31)
    n_gen, gen_len, n_reads = 10, 2_500_000, 750_000
    sym = np.frombuffer(b"ACGT", np.uint8)
    genomes = sym[rng.integers(0, 4, size=(n_gen, gen_len))]
    flat = genomes.reshape(-1)
    files = []
    for _ in range(2):
        start = rng.integers(0, n_gen, size=n_reads) * gen_len + rng.integers(0, gen_len - READ_LEN, size=n_reads)
        reads = flat[start[:, None] + np.arange(READ_LEN)[None, :]]
        subst = rng.random(reads.shape) < 0.01
        reads = np.where(subst, sym[rng.integers(0, 4, size=reads.shape)], reads).astype(np.uint8)
        files.append(reads)
    return [g.tobytes() for g in genomes], files, MC.taxonomy(n_gen, rng, False)


def parsers(ctx, path, fastq=False):
    lib = _lib.load()
    from_dev, from_file, host_read = ((ctx.docs_from_fastq_bytes_dev, ctx.docs_from_fastq, lib.lime_fastq_read) if fastq else
                                      (ctx.docs_from_bytes_dev, ctx.docs_from_fasta, lib.lime_fasta_read))
    data = open(path, "rb").read()
    n = len(data)
    t = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    res = {"input_bytes": n}
    res["device_parse_from_hbm"] = rate(n, best_of(lambda: from_dev(t).close()))
    res["device_parse_from_file"] = rate(n, best_of(lambda: from_file(path).close()))
    d = from_dev(t)
    res["n_docs"], res["n_text"] = d.info()
    if not fastq:
        res["device_revcomp"] = rate(n, best_of(lambda: d.revcomp().close()))
    dev = {False: d.get(), True: d.revcomp().get()}
    d.close()

    def host(rc):
        pt, po, nd = C.c_void_p(), C.c_void_p(), C.c_uint32(0)
        assert host_read(os.fsencode(path), int(rc), C.byref(pt), C.byref(po), C.byref(nd)) == 0
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(nd.value + 1,)).copy()
        text = np.frombuffer(C.string_at(pt, int(off[-1])), np.uint8)
        lib.lime_free(pt); lib.lime_free(po)
        return text, off

    for rc in (False, True):
        key = ("lime_fastq_read_rc%d" if fastq else "lime_fasta_read_rc%d") % rc
        pt, po, nd = C.c_void_p(), C.c_void_p(), C.c_uint32(0)
        def call():
            assert host_read(os.fsencode(path), int(rc), C.byref(pt), C.byref(po), C.byref(nd)) == 0
            lib.lime_free(pt); lib.lime_free(po)
        res[key] = rate(n, best_of(call))
        text, off = host(rc)
        res["equal_rc%d" % rc] = bool(np.array_equal(text, dev[rc][0]) and np.array_equal(off, dev[rc][1]))
    return res


def timed(cmd, cwd):
    t0 = time.perf_counter()
    p = subprocess.run(cmd, capture_output=True, cwd=cwd)
    ms = (time.perf_counter() - t0) * 1e3
    if p.returncode != 0:
        raise RuntimeError(f"{cmd}: exit {p.returncode}: {p.stderr.decode()[-1000:]}")
    return round(ms, 1)


def chains(d, n_reads, n_refs):
    """LiME_fasta --gidx against BuildIndex --gidx x 4 + LiME_paired, best of 3 whole runs each after a warm-up, alternating"""
    r1, r2, gidx, tax = (os.path.join(d, f) for f in ("reads_1.fasta", "reads_2.fasta", "g.gidx", "LineageFile.csv"))
    best = {}
    for k in range(4):
        one = {"LiME_fasta": timed([os.path.join(BIN, "LiME_fasta"), r1, r2, "--gidx", gidx, "--lineage", tax, "--readlen", str(READ_LEN), "--out",
                                    os.path.join(d, "one.txt")], d)}
        steps = {}
        bases = []
        for name, reads, flags in (("F1", r1, []), ("F1RC", r1, ["--rc"]), ("F2", r2, []), ("F2RC", r2, ["--rc"])):
            base = os.path.join(d, name)
            steps["BuildIndex " + name] = timed([os.path.join(BIN, "BuildIndex"), reads, "--gidx", gidx, base] + flags, d)
            bases.append(base)
        steps["LiME_paired"] = timed([os.path.join(BIN, "LiME_paired")] + bases + [os.path.join(d, "chain.txt"), str(n_reads), str(n_refs), tax, str(READ_LEN), "8"], d)
        steps["chain"] = round(sum(steps.values()), 1)
        one.update(steps)
        if k:
            for key, v in one.items():
                best[key] = min(best.get(key, v), v)
    # LiME_fasta's own phases (LIME_CLI_TIMING: wall-clock marks on stderr), one more run
    p = subprocess.run([os.path.join(BIN, "LiME_fasta"), r1, r2, "--gidx", gidx, "--lineage", tax, "--readlen", str(READ_LEN), "--out", os.path.join(d, "one.txt")],
                       env=dict(os.environ, LIME_CLI_TIMING="1"), capture_output=True, cwd=d)
    best["LiME_fasta_phases"] = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[cli\] (.+?)\s+([\d.]+) ms \(at", p.stderr.decode())}
    best["classification_equal"] = open(os.path.join(d, "one.txt"), "rb").read() == open(os.path.join(d, "chain.txt"), "rb").read()
    best["array_file_bytes"] = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith((".ebwt", ".lcp", ".da")))
    return best


def fastq_end_to_end(d):
    """LiME_fasta --gidx on the FASTQ pair next to the FASTA pair, best of 3 whole runs each after a warm-up, alternating"""
    gidx, tax = os.path.join(d, "g.gidx"), os.path.join(d, "LineageFile.csv")
    best = {}
    for k in range(4):
        for key, ext in (("LiME_fasta on FASTA", "fasta"), ("LiME_fasta on FASTQ", "fastq")):
            ms = timed([os.path.join(BIN, "LiME_fasta"), os.path.join(d, "reads_1." + ext), os.path.join(d, "reads_2." + ext), "--gidx", gidx, "--lineage", tax,
                        "--readlen", str(READ_LEN), "--out", os.path.join(d, "e2e_" + ext + ".txt")], d)
            if k:
                best[key] = min(best.get(key, ms), ms)
    p = subprocess.run([os.path.join(BIN, "LiME_fasta"), os.path.join(d, "reads_1.fastq"), os.path.join(d, "reads_2.fastq"), "--gidx", gidx, "--lineage", tax,
                        "--readlen", str(READ_LEN), "--out", os.path.join(d, "e2e_fastq.txt")], env=dict(os.environ, LIME_CLI_TIMING="1"), capture_output=True, cwd=d)
    best["LiME_fasta_on_FASTQ_phases"] = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[cli\] (.+?)\s+([\d.]+) ms \(at", p.stderr.decode())}
    best["classification_equal"] = open(os.path.join(d, "e2e_fasta.txt"), "rb").read() == open(os.path.join(d, "e2e_fastq.txt"), "rb").read()
    return best


def one_input(ctx, genomes, reads, lineage, chain):
    with tempfile.TemporaryDirectory() as d:
        for name, rows in zip(("reads_1", "reads_2"), reads):
            open(os.path.join(d, name + ".fasta"), "wb").write(fasta_of_reads(rows))
            open(os.path.join(d, name + ".fastq"), "wb").write(fastq_of_reads(rows))
        open(os.path.join(d, "refs.fasta"), "wb").write(fasta_of_genomes(genomes))
        open(os.path.join(d, "LineageFile.csv"), "wb").write(lineage)
        res = parsers(ctx, os.path.join(d, "reads_1.fasta"))
        res["fastq"] = parsers(ctx, os.path.join(d, "reads_1.fastq"), fastq=True)
        res["index_ms"] = timed([os.path.join(BIN, "BuildIndex"), "--refs", os.path.join(d, "refs.fasta"), os.path.join(d, "g")], d)
        res["fastq_end_to_end_ms"] = fastq_end_to_end(d)
        if chain:
            res["end_to_end_ms"] = chains(d, res["n_docs"], len(genomes))
        else:
            res["end_to_end_ms"] = "not measured"
        return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    res = {"bench": "fasta", "device": torch.cuda.get_device_name(0), "fasta_block": api.FASTA_BLOCK}
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_full.npz"))
    genomes, sets = G.collections(z["reads_1"], z["reads_2"], z["src"])
    as_rows = lambda reads: np.frombuffer(b"".join(reads), np.uint8).reshape(-1, READ_LEN)

    def emit():
        line = json.dumps(res)
        print(line, flush=True)
        if args:
            with open(args[0], "w") as f:
                f.write(line + "\n")

    res["example"] = one_input(ctx, genomes, [as_rows(sets["F1"]), as_rows(sets["F2"])], bytes(z["lineage"]), True)
    emit()                                       # (the large input's chain takes minutes: what is measured so far is on record)
    res["reads"] = one_input(ctx, *synthetic(), "--skip-big-chain" not in sys.argv)
    ctx.close()
    emit()


if __name__ == "__main__":
    main()
