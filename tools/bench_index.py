#!/usr/bin/env python3
"""tools/bench_index.py [out.json] -- the index builder (lime_build_index_dev), a side benchmark (bench.py stays the yardstick).

Workloads, all device-resident (text and doc_off uploaded before the clock starts):
  example   the four collections of tests/golden/example_full.npz (2.5 * 10^6 symbols each), and lime_amd.builder.build_arrays_sa's wall
            time on the first of them on the same box
  reads     ~10^8 symbols: 10 random genomes of 2.5 * 10^6 bases, 750 000 reads of 100 bases sampled from them with 1 % substitutions
  twins     the same with genome 1 a copy of genome 0 that differs in 1 % of its positions, full lcp and lcp_cap 32 (eGap's --trlcp 32)
Per workload: symbols/s (best of 3 after one warm-up, wall clock around the call), the doubling rounds, the suffixes left after the first
rounds and the phases' HIP-event ms.  Prints one JSON line (and writes it to out.json if given)."""
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
from lime_amd.builder import build_arrays_sa  # noqa: E402
import make_golden_example as G  # noqa: E402


def now():
    torch.cuda.synchronize()
    return time.perf_counter()


def measure(ctx, text_t, off_t, n_docs, n_text, lcp_cap=0, reps=3):
    n = n_text + n_docs
    out = (torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"))
    best, info = None, None
    for k in range(reps + 1):
        t0 = now()
        ctx.build_index_dev(text_t, off_t, n_docs, n_text, 0, lcp_cap, out=out)
        dt = now() - t0
        if k and (best is None or dt < best):
            best, info = dt, ctx.index_info()
    lcp = out[1]
    return {"positions": n, "ms": round(best * 1e3, 3), "symbols_per_s": round(n / best), "rounds": info["rounds"], "unresolved": info["unresolved"],
            "sort_ms": round(info["sort_ms"], 3), "doubling_ms": round(info["doubling_ms"], 3), "lcp_ms": round(info["lcp_ms"], 3),
            "lcp_cap": lcp_cap, "lcp_sum": int(lcp.to(torch.int64).sum()), "lcp_max": int(lcp.max())}


def synthetic(twins):
    g = torch.Generator(device="cuda"); g.manual_seed(31)
    n_gen, gen_len, n_reads, read_len = 10, 2_500_000, 750_000, 100
    sym = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    genomes = sym[torch.randint(0, 4, (n_gen, gen_len), device="cuda", generator=g)]
    if twins:
        change = torch.rand(gen_len, device="cuda", generator=g) < 0.01
        genomes[1] = torch.where(change, sym[torch.randint(0, 4, (gen_len,), device="cuda", generator=g)], genomes[0])
    src = torch.randint(0, n_gen, (n_reads,), device="cuda", generator=g)
    start = torch.randint(0, gen_len - read_len, (n_reads,), device="cuda", generator=g)
    reads = genomes.reshape(-1)[(src * gen_len + start)[:, None] + torch.arange(read_len, device="cuda")[None, :]]
    subst = torch.rand(reads.shape, device="cuda", generator=g) < 0.01
    reads = torch.where(subst, sym[torch.randint(0, 4, reads.shape, device="cuda", generator=g)], reads)
    text_t = torch.cat([reads.reshape(-1), genomes.reshape(-1)]).contiguous()
    lens = torch.cat([torch.full((n_reads,), read_len, dtype=torch.int64), torch.full((n_gen,), gen_len, dtype=torch.int64)])
    off_t = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)]).cuda()
    return text_t, off_t, n_reads + n_gen, int(off_t[-1])


def main():
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    ctx.set_timing(True)
    res = {"bench": "index", "device": torch.cuda.get_device_name(0)}
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_full.npz"))
    genomes, sets = G.collections(z["reads_1"], z["reads_2"], z["src"])
    res["example"] = {}
    for name in G.SETS:
        text, off = api.pack_documents(sets[name], genomes)
        r = measure(ctx, torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), len(off) - 1, int(off[-1]))
        res["example"][name] = r
    t0 = time.perf_counter()
    build_arrays_sa(sets["F1"], genomes, 0)
    res["example"]["build_arrays_sa_F1_s"] = round(time.perf_counter() - t0, 2)
    res["reads"] = measure(ctx, *synthetic(False))
    tw = synthetic(True)
    res["twins"] = measure(ctx, *tw)
    res["twins_trlcp32"] = measure(ctx, *tw, lcp_cap=32)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
