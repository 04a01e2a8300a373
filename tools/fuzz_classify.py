#!/usr/bin/env python3
"""tools/fuzz_classify.py [seconds] [seed] -- random collections through lime_classify_lists_dev against lime_classify_mem and the model of
tests/classify_cases.py (every field of every verdict, and the classification file's bytes), on the GPU box: the generator of
tests/test_classify_edges_gpu.py::test_200_fuzz_seeds (classify_cases.fuzz_collection) in a time-boxed loop.  2 or 4 lists, up to 300 genomes,
near-ties, counts on the 0.02 tolerance, beta 0, any rank / HIGHER / BIN; stops at the first difference with the call that reproduces it.
Not part of the test suite (a soak)."""
import os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import lime_amd
from lime_amd import api
import classify_cases as CC

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 1
t_end = time.time() + budget
t_print = time.time()
stats = {"cases": 0, "reads": 0, "C": 0, "U": 0, "A": 0, "H": 0}
ctx = lime_amd.Context()
tmp = tempfile.mkdtemp()
try:
    case = 0
    while time.time() < t_end:
        seed = 1000 * seed0 + case
        col, rank, higher, binary = CC.fuzz_collection(seed)
        n_files, n_targ, (n_reads, _) = len(col["sims"]), col["n_targ"], col["sims"][0].shape
        tables = []
        for s in col["sims"]:
            t = torch.zeros(api.sim_bytes(n_reads, n_targ), dtype=torch.uint8, device="cuda")
            t[:n_reads * n_targ] = torch.from_numpy(np.ascontiguousarray(s).reshape(-1)).cuda()
            tables.append(t)
        dev = [ctx.choose_lists_dev(t, n_reads, n_targ, col["norm"], col["beta"]) for t in tables]
        host = CC.collection_lists(col)
        tax = os.path.join(tmp, "lineage.csv")
        open(tax, "wb").write(col["tax"])
        tx = api.load_taxonomy(tax, rank, higher, n_targ)
        v, _ = ctx.classify_lists_dev(dev, n_targ, tx, binary)
        vm, _ = api.classify_mem(host, [col["norm"]] * n_files, [col["beta"]] * n_files, n_targ, tx, binary)
        rep = CC.model_decide(host, [col["norm"]] * n_files, [col["beta"]] * n_files, n_targ, CC.Tax(col["tax"], rank, higher, n_targ), binary)
        outp = os.path.join(tmp, "dev.txt")
        api.write_classification(outp, v)
        diff = CC.same_verdicts(rep, v) or CC.same_verdicts(rep, vm) or (None if open(outp, "rb").read() == CC.classification_bytes(rep) else "file bytes")
        if diff is not None:
            sys.exit(f"fuzz_classify: tests.classify_cases.fuzz_collection({seed}) [{col['name']}, rank {rank}, HIGHER {higher}, BIN {binary}]: {diff}")
        tx.close()
        for li in dev:
            li.close()
        stats["cases"] += 1; stats["reads"] += n_reads
        for x in rep:
            stats[x.type] += 1
        case += 1
        if time.time() - t_print > 30:                   # a line now and then: a silent GPU run is taken for hung
            print("fuzz_classify ...", stats, flush=True); t_print = time.time()
finally:
    ctx.close()
print("fuzz_classify ok:", stats, "in", round(budget), "s, seed", seed0)
