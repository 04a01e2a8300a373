#!/usr/bin/env python3
"""tools/bench_shards.py [out.json] [--kernels-only | --sample-only] -- what classifying against a genome database cut into index shards
costs (lime_lists_concat_dev, lime_classify_sample_shards_dev, LiME_fasta with --gidx given several times: DESIGN.md section 9 f11), a
side benchmark (bench.py stays the yardstick).  One session, one box, the page cache warm.
  (a) the kernels: the table of BASELINE.json configs[2]'s input (10^9 synthetic symbols, 10^6 reads x 5000 genomes, alpha 16, no ebwt) is
      built once on the device, its 2 and its 4 column shards are made into lists with beta -1 (lime_choose_lists_dev on contiguous
      copies of the column slices), and lime_lists_concat_dev makes the whole table's list at beta 0.02: HIP-event ms of k_lc_rows, of the
      prefix sum and of k_lc_copy (lime_get_concat_info, best of 5 after a warm-up), the call's wall clock, and a device-to-device
      hipMemcpy of the output pairs' bytes in the same session: the yardstick.  The result is compared with lime_choose_lists_dev of
      the whole table in the same run.
  (b) the sample: `LiME_fasta reads_1.fastq reads_2.fastq --gidx ...` on tools/bench_fasta.py's input (10 random genomes of 2.5 * 10^6
      bases, 2 x 750 000 reads of 100 bases as FASTQ) with the genomes' index cut into 1, 2 and 5 shards (BuildIndex --refs
      --shard-positions): whole processes, alternating, best of 3 after a warm-up; the comparison is the one-shard run of the same
      session; every classification file is compared with the one-shard run's.
No database above 2^32 positions is run here.  Prints one JSON line (and writes it to out.json if given)."""
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

N, N_READS, N_REFS, ALPHA, NORM, BETA = 1_000_000_000, 1_000_000, 5000, 16, 85, 0.02


def kernels(ctx):
    dev = torch.device("cuda:0")
    lcp = torch.empty(N, dtype=torch.int32, device=dev)
    da = torch.empty_like(lcp)
    ctx.synth_dev(42, 0, N, N_READS, N_REFS, ALPHA, 0, lcp, da, None)
    table = torch.zeros(api.sim_bytes(N_READS, N_REFS), dtype=torch.uint8, device=dev)
    ctx.fused_dev(lcp, da, None, N, N, 1, N_READS, N_REFS, ALPHA, table)
    s, rc = ctx.stats()
    assert rc == 0, rc
    del lcp, da
    torch.cuda.empty_cache()
    whole = ctx.choose_lists_dev(table, N_READS, N_REFS, NORM, BETA)
    want = whole.get()
    n_pairs = whole.info()[1]
    res = {"table": f"{N_READS}x{N_REFS}", "symbols": N, "beta": BETA, "table_updates": int(s.n_updates), "output_pairs": n_pairs, "output_bytes": 8 * n_pairs}
    # the yardstick: a device-to-device copy of the output pairs' bytes
    src = torch.empty(8 * n_pairs, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = BF.best_of(lambda: _lib.hip_memcpy_d2d(dst.data_ptr(), src.data_ptr(), 8 * n_pairs), reps=5)
    res["memcpy_dtod"] = {"ms": round(ms, 3), "GBps_read_plus_write": round(2 * 8 * n_pairs / ms / 1e6, 1)}
    del src, dst
    view = table[:N_READS * N_REFS].view(N_READS, N_REFS)
    ctx.set_timing(True)
    for n_parts in (2, 4):
        cuts = [N_REFS * k // n_parts for k in range(n_parts + 1)]
        parts = []
        for a, b in zip(cuts, cuts[1:]):
            t = torch.zeros(api.sim_bytes(N_READS, b - a), dtype=torch.uint8, device=dev)
            t[:N_READS * (b - a)].view(N_READS, b - a).copy_(view[:, a:b])
            torch.cuda.synchronize()
            parts.append(ctx.choose_lists_dev(t, N_READS, b - a, NORM, -1.0))
            del t
        best, wall = None, None
        for k in range(6):
            t0 = BF.now()
            li = ctx.lists_concat(parts, cuts[:-1], np.diff(cuts), BETA)
            dt = (BF.now() - t0) * 1e3
            info = ctx.concat_info()
            if k == 0:
                got = li.get()
                equal = all(np.array_equal(x, y) for x, y in zip(got, want))
                del got
            li.close()
            if k and (best is None or info["rows_ms"] + info["copy_ms"] < best["rows_ms"] + best["copy_ms"]):
                best = info
            if k and (wall is None or dt < wall):
                wall = dt
        kern = best["rows_ms"] + best["copy_ms"]
        res[f"{n_parts}_shards"] = {"input_pairs": sum(p.info()[1] for p in parts), "k_lc_rows_ms": round(best["rows_ms"], 3), "scan_ms": round(best["scan_ms"], 3),
                                    "k_lc_copy_ms": round(best["copy_ms"], 3), "rows_plus_copy_ms": round(kern, 3), "call_wall_ms": round(wall, 3),
                                    "over_memcpy_dtod": round(kern / ms, 2), "equal_to_the_whole_tables_list": bool(equal)}
        for p in parts:
            p.close()
    ctx.set_timing(False)
    whole.close()
    return res


def sample(d):
    exe = os.path.join(BF.BIN, "LiME_fasta")
    genomes, reads, lineage = BF.synthetic()
    for name, rows in zip(("reads_1", "reads_2"), reads):
        open(os.path.join(d, name + ".fastq"), "wb").write(BF.fastq_of_reads(rows))
    open(os.path.join(d, "refs.fasta"), "wb").write(BF.fasta_of_genomes(genomes))
    open(os.path.join(d, "LineageFile.csv"), "wb").write(lineage)
    per = len(genomes[0]) + 1
    shards, res = {}, {"reads": 2 * len(reads[0]), "genomes": len(genomes), "genome_positions": per * len(genomes), "index_ms": {}}
    for n_shards in (1, 2, 5):
        base = os.path.join(d, "g%d" % n_shards)
        res["index_ms"][str(n_shards)] = round(BF.timed([os.path.join(BF.BIN, "BuildIndex"), "--refs", os.path.join(d, "refs.fasta"), base, "--shard-positions",
                                                         str(per * (len(genomes) // n_shards))], d), 1)
        shards[n_shards] = [f"{base}.{s:03d}.gidx" for s in range(n_shards)]
        assert all(os.path.exists(p) for p in shards[n_shards]) and not os.path.exists(f"{base}.{n_shards:03d}.gidx")
    base = [exe, os.path.join(d, "reads_1.fastq"), os.path.join(d, "reads_2.fastq"), "--lineage", os.path.join(d, "LineageFile.csv"), "--readlen", str(BF.READ_LEN)]
    best = {}
    for k in range(4):
        for n_shards, files in shards.items():
            ms = BF.timed(base + ["--out", os.path.join(d, "out_%d.txt" % n_shards)] + [x for f in files for x in ("--gidx", f)], d)
            if k:
                best[str(n_shards)] = round(min(best.get(str(n_shards), ms), ms), 1)
    one = open(os.path.join(d, "out_1.txt"), "rb").read()
    res["ms"] = best
    res["over_one_shard"] = {k: round(v / best["1"], 3) for k, v in best.items() if k != "1"}
    res["classification_equal"] = {str(n): open(os.path.join(d, "out_%d.txt" % n), "rb").read() == one for n in (2, 5)}
    res["classification_lines"] = one.count(b"\n") - 1
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    torch.cuda.set_device(0)
    res = {"bench": "shards", "device": torch.cuda.get_device_name(0), "above_2^32_positions_run": False}
    if "--sample-only" not in sys.argv:
        ctx = api.Context(0)
        res["kernels"] = kernels(ctx)
        ctx.close()
        api.trim_cache()
        torch.cuda.empty_cache()
    if "--kernels-only" not in sys.argv:
        with tempfile.TemporaryDirectory() as d:
            res["sample"] = sample(d)
    line = json.dumps(res)
    print(line, flush=True)
    if args:
        os.makedirs(os.path.dirname(os.path.abspath(args[0])), exist_ok=True)
        with open(args[0], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
