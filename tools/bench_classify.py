#!/usr/bin/env python3
"""tools/bench_classify.py [out.json] -- Classify on the device against today's chain, a side benchmark (bench.py stays the yardstick).

Workload: four collections at BASELINE.json configs[2]'s shape (10^9 symbols, 10^6 reads x 5000 genomes, EBWT=0, alpha 16, norm 85) made
by lime_synth_dev with four seeds -- a paired-end sample's F, F_RC, R, R_RC --, at beta 0.25 and 0.02, and a generated lineage file
(tests/golden/make_golden_classify.taxonomy: shared species and genera).  Per beta:
  lists    per collection: lime_fused_choose_lists_dev (scan + clusterAnalyze + clusterChoose, the lists left in HBM), ms and pairs
  kernel   k_classify alone (HIP events, lime_get_host_times[7]) in ms and GB/s over its algorithmic bytes: the pairs, the row offsets and
           maxima of the four lists, the verdicts
  new      end to end: the four lists passes + lime_classify_lists_dev (verdicts to the host) + lime_write_classification
  old      today's chain: per collection lime_fused_choose_dev (pairs to the host) + lime_write_res_bin_pairs, then lime_classify over the
           four .res.bin files -- and the two classification files must be the same bytes.
Prints one JSON line (and writes it to out.json if given).

tools/bench_classify.py --per-read [out.json] -- the per-read norm on the same collections at beta 0.02, without
the .res chain: k_classify on the four lists made with norm 85 (the figure `kernel_ms` above: the fixed-norm path, which a per-read call
never touches) against k_classify_norms on the same rows made per read with constant norms of 85 (unfiltered lists, beta -1, then
lime_lists_concat_norms_dev: the extra pass of the per-read sample path, timed by lime_get_concat_info), the verdicts byte for byte the
same; and that extra pass once more at the example's size (10^4 reads x 3 genomes)."""
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lime_amd import _lib, api  # noqa: E402
import make_golden_classify as M  # noqa: E402

N, NR, NG, ALPHA, NORM = 1_000_000_000, 1_000_000, 5000, 16, 85
SEEDS = (42, 43, 44, 45)


def now():
    torch.cuda.synchronize()
    return time.perf_counter()


def per_read(out_path):
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    dev = torch.device("cuda:0")
    work = tempfile.mkdtemp(prefix="bench_classify_")
    tax = os.path.join(work, "lineage.csv")
    open(tax, "wb").write(M.taxonomy(NG, np.random.default_rng(7), False))
    tx = api.load_taxonomy(tax, 1, 0, NG)
    beta = 0.02
    res = {"workload": "4 x configs[2] shape (1e9 symbols, 1e6 x 5000, EBWT=0), seeds " + ",".join(map(str, SEEDS)) + ", beta 0.02, constant norms 85",
           "rank": 1, "higher": 0}
    try:
        lcp = torch.empty(N, dtype=torch.int32, device=dev)
        da = torch.empty_like(lcp)
        norms = torch.full((NR,), NORM, dtype=torch.uint8, device=dev)
        ctx.synth_dev(SEEDS[0], 0, N, NR, NG, ALPHA, 0, lcp, da, None)
        ctx.fused_choose_lists_dev(lcp, da, None, N, NR, NG, ALPHA, NORM, 0.25)[0].close()      # warm: probe, scratch, record pools
        fixed, per, concat = [], [], []
        for seed in SEEDS:
            ctx.synth_dev(seed, 0, N, NR, NG, ALPHA, 0, lcp, da, None)
            fixed.append(ctx.fused_choose_lists_dev(lcp, da, None, N, NR, NG, ALPHA, NORM, beta)[0])
            raw, _ = ctx.fused_choose_lists_dev(lcp, da, None, N, NR, NG, ALPHA, 1, -1.0)
            ctx.set_timing(1)
            best = None
            for _ in range(3):
                li = ctx.lists_concat_norms([raw], [0], [NG], norms, beta)
                info = ctx.concat_info()
                if best is None or info["rows_ms"] + info["scan_ms"] + info["copy_ms"] < best["rows_ms"] + best["scan_ms"] + best["copy_ms"]:
                    best = info
                li.close()
            per.append(ctx.lists_concat_norms([raw], [0], [NG], norms, beta))
            ctx.set_timing(0)
            best["pairs_in"] = raw.info()[1]
            concat.append({k: (round(v, 3) if isinstance(v, float) else v) for k, v in best.items()})
            raw.close()
        res["pairs"] = [li.info()[1] for li in fixed]
        res["same_lists_pairs"] = res["pairs"] == [li.info()[1] for li in per]
        res["concat_norms"] = concat
        ctx.set_timing(1)
        out = {}
        for name, lists in (("k_classify", fixed), ("k_classify_norms", per), ("k_classify_again", fixed)):
            kern = []
            for _ in range(5):
                v, counts = ctx.classify_lists_dev(lists, NG, tx, True)
                kern.append(ctx.host_times()["classify_kernel_ms"])
            out[name] = (v.tobytes(), counts)
            res[name + "_ms"] = round(min(kern), 3)
            res[name + "_ms_all"] = [round(x, 3) for x in kern]
        ctx.set_timing(0)
        res["counts_CUAH"] = out["k_classify"][1]
        res["same_verdicts"] = out["k_classify"][0] == out["k_classify_norms"][0]
        res["norms_over_fixed"] = round(res["k_classify_norms_ms"] / min(res["k_classify_ms"], res["k_classify_again_ms"]), 3)
        nbytes = sum(res["pairs"]) * 8 + 4 * (NR + 1) * 8 + 4 * NR + NR * 12
        res["kernel_bytes"] = nbytes
        for li in fixed + per:
            li.close()
        del lcp, da
        # the extra pass at the example's size: 10^4 reads x 3 genomes
        n2, nr2, ng2 = 4_000_000, 10_000, 3
        lcp = torch.empty(n2, dtype=torch.int32, device=dev)
        da = torch.empty_like(lcp)
        ctx.synth_dev(SEEDS[0], 0, n2, nr2, ng2, ALPHA, 0, lcp, da, None)
        raw, _ = ctx.fused_choose_lists_dev(lcp, da, None, n2, nr2, ng2, ALPHA, 1, -1.0)
        norms2 = torch.full((nr2,), NORM, dtype=torch.uint8, device=dev)
        ctx.set_timing(1)
        small = []
        for _ in range(5):
            t0 = now()
            li = ctx.lists_concat_norms([raw], [0], [ng2], norms2, 0.25)
            call_ms = (now() - t0) * 1e3
            info = ctx.concat_info()
            info["call_ms"] = call_ms
            small.append(info)
            li.close()
        ctx.set_timing(0)
        b = min(small, key=lambda x: x["call_ms"])
        b["pairs_in"] = raw.info()[1]
        res["concat_norms_example_size"] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in b.items()}
    finally:
        shutil.rmtree(work, ignore_errors=True)
        tx.close()
        ctx.close()
    line = json.dumps(res)
    print(line)
    if out_path:
        open(out_path, "w").write(line + "\n")


def main():
    if "--per-read" in sys.argv[1:]:
        rest = [a for a in sys.argv[1:] if a != "--per-read"]
        return per_read(rest[0] if rest else None)
    lib = _lib.load()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    dev = torch.device("cuda:0")
    work = tempfile.mkdtemp(prefix="bench_classify_")
    tax = os.path.join(work, "lineage.csv")
    open(tax, "wb").write(M.taxonomy(NG, np.random.default_rng(7), False))
    tx = api.load_taxonomy(tax, 1, 0, NG)
    lcp = torch.empty(N, dtype=torch.int32, device=dev)
    da = torch.empty_like(lcp)
    res = {"workload": "4 x configs[2] shape (1e9 symbols, 1e6 x 5000, EBWT=0), seeds " + ",".join(map(str, SEEDS)), "rank": 1, "higher": 0}
    try:
        ctx.synth_dev(SEEDS[0], 0, N, NR, NG, ALPHA, 0, lcp, da, None)
        ctx.fused_choose_lists_dev(lcp, da, None, N, NR, NG, ALPHA, NORM, 0.25)[0].close()      # warm: probe, scratch, record pools
        for beta in (0.25, 0.02):
            r = {"lists_ms": [], "pairs": [], "old_choose_ms": [], "old_write_ms": []}
            lists, bases = [], []
            for k, seed in enumerate(SEEDS):
                ctx.synth_dev(seed, 0, N, NR, NG, ALPHA, 0, lcp, da, None)
                t0 = now()
                li, _ = ctx.fused_choose_lists_dev(lcp, da, None, N, NR, NG, ALPHA, NORM, beta)
                r["lists_ms"].append(round((now() - t0) * 1e3, 3))
                lists.append(li)
                r["pairs"].append(li.info()[1])
                # today's chain for the same collection
                t0 = now()
                mx, off, pairs, _ = ctx.fused_choose_dev(lcp, da, None, N, NR, NG, ALPHA, NORM, beta)
                r["old_choose_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
                b = os.path.join(work, f"c{k}.res")
                t0 = time.perf_counter()
                assert lib.lime_write_res_bin_pairs((b + ".bin").encode(), (b + ".pos").encode(), mx.ctypes.data, off.ctypes.data,
                                                    pairs.ctypes.data if len(pairs) else None, NR, NORM, C.c_float(beta)) == 0
                r["old_write_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
                bases.append(b)
                del mx, off, pairs
            ctx.set_timing(1)
            kern, call = [], []
            for _ in range(3):
                t0 = now()
                v, counts = ctx.classify_lists_dev(lists, NG, tx, True)
                call.append((time.perf_counter() - t0) * 1e3)
                kern.append(ctx.host_times()["classify_kernel_ms"])
            ctx.set_timing(0)
            out_new = os.path.join(work, "new.txt")
            t0 = time.perf_counter()
            api.write_classification(out_new, v)
            write_ms = (time.perf_counter() - t0) * 1e3
            nbytes = sum(r["pairs"]) * 8 + 4 * (NR + 1) * 8 + 4 * NR + NR * 12
            r.update(counts_CUAH=counts, rules={str(q): int((v["rule"] == q).sum()) for q in range(4)},
                     kernel_ms=round(min(kern), 3), kernel_bytes=nbytes, kernel_GBps=round(nbytes / min(kern) / 1e6, 1),
                     kernel_roofline_frac=round(nbytes / min(kern) / 1e6 / 8000.0, 4),
                     classify_call_ms=round(min(call), 3), write_classification_ms=round(write_ms, 3))
            arr = (C.c_char_p * 4)(*[b.encode() for b in bases])
            out_old = os.path.join(work, "old.txt")
            t0 = time.perf_counter()
            assert lib.lime_classify(4, arr, 1, NR, NG, out_old.encode(), tax.encode(), 1, 0, None) == 0, lib.lime_classify_error()
            r["old_classify_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            r["same_bytes"] = open(out_new, "rb").read() == open(out_old, "rb").read()
            r["new_end_to_end_ms"] = round(sum(r["lists_ms"]) + r["classify_call_ms"] + write_ms, 3)
            r["old_end_to_end_ms"] = round(sum(r["old_choose_ms"]) + sum(r["old_write_ms"]) + r["old_classify_ms"], 3)
            r["speedup"] = round(r["old_end_to_end_ms"] / r["new_end_to_end_ms"], 2)
            res[f"beta_{beta}"] = r
            for li in lists:
                li.close()
            for b in bases:
                for ext in (".bin", ".pos"):
                    os.remove(b + ext)
    finally:
        shutil.rmtree(work, ignore_errors=True)
        tx.close()
        ctx.close()
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(line + "\n")


if __name__ == "__main__":
    main()
