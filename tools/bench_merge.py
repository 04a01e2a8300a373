#!/usr/bin/env python3
"""tools/bench_merge.py [out.json] -- reads merged into a genome index built once (lime_gindex_build_dev + lime_merge_index_dev) against
the index built from scratch per read set (lime_build_index_dev), a side benchmark (bench.py stays the yardstick).

The three collections of tools/bench_index.py, all device-resident before the clock starts:
  example   tests/golden/example_full.npz: the genomes and the four read sets F1, F1RC, F2, F2RC
  reads     10 random genomes of 2.5 * 10^6 bases; two sets of 750 000 reads of 100 bases sampled from them with 1 % substitutions, each
            forward and reverse-complemented
  twins     the same with genome 1 a copy of genome 0 that differs in 1 % of its positions
Per collection: lime_gindex_build_dev once after a warm-up (wall ms and the builder's phases), then for each of the four read sets the wall ms of
lime_merge_index_dev (best of 3 after a warm-up; its phases) and of lime_build_index_dev on the concatenation, in this process; the
outputs of both are compared on the device.  "four_merges_plus_index_ms" against "four_builds_ms" is what indexing the genomes once buys.
Prints one JSON line (and writes it to out.json if given)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lime_amd import api  # noqa: E402
import make_golden_example as G  # noqa: E402


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


def run(ctx, genomes_t, g_off_t, read_sets, lcp_cap=0):
    """genomes_t / g_off_t: the genomes' text and offsets on the device; read_sets: {name: (text_t, off_t)}"""
    n_refs, g_text = len(g_off_t) - 1, int(g_off_t[-1])
    res = {"genome_positions": g_text + n_refs, "lcp_cap": lcp_cap}
    ctx.build_genome_index_dev(genomes_t, g_off_t, n_refs, g_text, 0, lcp_cap).close()      # warm-up: code objects, the block cache
    t0 = now()
    gi = ctx.build_genome_index_dev(genomes_t, g_off_t, n_refs, g_text, 0, lcp_cap)
    res["index_ms"] = round((now() - t0) * 1e3, 3)
    info = ctx.index_info()
    res["index_phases"] = {"rounds": info["rounds"], "unresolved": info["unresolved"], "sort_ms": round(info["sort_ms"], 3),
                           "doubling_ms": round(info["doubling_ms"], 3), "lcp_ms": round(info["lcp_ms"], 3)}
    res["sets"] = {}
    merges = builds = 0.0
    for name, (r_t, r_off_t) in read_sets.items():
        n_reads, r_text = len(r_off_t) - 1, int(r_off_t[-1])
        n = r_text + n_reads + g_text + n_refs
        out_m = (torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"))
        out_b = tuple(torch.empty_like(t) for t in out_m)
        ms_m = best_of(lambda: ctx.merge_index_dev(r_t, r_off_t, n_reads, r_text, gi, lcp_cap, out=out_m))
        mi = ctx.merge_info()
        all_t = torch.cat([r_t[:r_text], genomes_t[:g_text]])
        off_t = torch.cat([r_off_t, g_off_t[1:] + r_text])
        ms_b = best_of(lambda: ctx.build_index_dev(all_t, off_t, n_reads + n_refs, r_text + g_text, 0, lcp_cap, out=out_b))
        bi = ctx.index_info()
        res["sets"][name] = {"positions": n, "read_positions": r_text + n_reads, "merge_ms": round(ms_m, 3), "build_ms": round(ms_b, 3),
                             "equal": all(bool(torch.equal(a, b)) for a, b in zip(out_m, out_b)),
                             "merge_phases": {"reads_rounds": mi["reads_rounds"], "read_runs": mi["read_runs"], "reads_build_ms": round(mi["reads_build_ms"], 3),
                                              "rank_ms": round(mi["rank_ms"], 3), "place_ms": round(mi["place_ms"], 3)},
                             "build_phases": {"rounds": bi["rounds"], "sort_ms": round(bi["sort_ms"], 3), "doubling_ms": round(bi["doubling_ms"], 3),
                                              "lcp_ms": round(bi["lcp_ms"], 3)}}
        merges += ms_m
        builds += ms_b
        del out_m, out_b, all_t, off_t
    gi.close()
    res["four_merges_ms"] = round(merges, 3)
    res["four_merges_plus_index_ms"] = round(merges + res["index_ms"], 3)
    res["four_builds_ms"] = round(builds, 3)
    return res


def dev_docs(docs):
    text = np.frombuffer(b"".join(docs), np.uint8).copy()
    off = np.concatenate(([0], np.cumsum([len(d) for d in docs]))).astype(np.int64)
    return torch.from_numpy(text).cuda(), torch.from_numpy(off).cuda()


def synthetic(twins):
    g = torch.Generator(device="cuda"); g.manual_seed(31)
    n_gen, gen_len, n_reads, read_len = 10, 2_500_000, 750_000, 100
    sym = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    genomes = sym[torch.randint(0, 4, (n_gen, gen_len), device="cuda", generator=g)]
    if twins:
        change = torch.rand(gen_len, device="cuda", generator=g) < 0.01
        genomes[1] = torch.where(change, sym[torch.randint(0, 4, (gen_len,), device="cuda", generator=g)], genomes[0])
    comp = torch.arange(256, dtype=torch.uint8, device="cuda")
    for a, b in (b"AT", b"TA", b"CG", b"GC"):
        comp[a] = b
    r_off = (torch.arange(n_reads + 1, dtype=torch.int64) * read_len).cuda()
    sets = {}
    for name in ("F1", "F2"):
        src = torch.randint(0, n_gen, (n_reads,), device="cuda", generator=g)
        start = torch.randint(0, gen_len - read_len, (n_reads,), device="cuda", generator=g)
        reads = genomes.reshape(-1)[(src * gen_len + start)[:, None] + torch.arange(read_len, device="cuda")[None, :]]
        subst = torch.rand(reads.shape, device="cuda", generator=g) < 0.01
        reads = torch.where(subst, sym[torch.randint(0, 4, reads.shape, device="cuda", generator=g)], reads)
        sets[name] = (reads.reshape(-1).contiguous(), r_off)
        sets[name + "RC"] = (comp[reads.flip(1).to(torch.int64)].reshape(-1).contiguous(), r_off)
    g_off = (torch.arange(n_gen + 1, dtype=torch.int64) * gen_len).cuda()
    return genomes.reshape(-1).contiguous(), g_off, sets


def main():
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    ctx.set_timing(True)
    res = {"bench": "merge", "device": torch.cuda.get_device_name(0)}
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_full.npz"))
    genomes, sets = G.collections(z["reads_1"], z["reads_2"], z["src"])
    g_t, g_off = dev_docs(genomes)
    res["example"] = run(ctx, g_t, g_off, {name: dev_docs(sets[name]) for name in G.SETS})
    res["reads"] = run(ctx, *synthetic(False))
    tw = synthetic(True)
    res["twins"] = run(ctx, *tw)
    res["twins_trlcp32"] = run(ctx, *tw, lcp_cap=32)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
