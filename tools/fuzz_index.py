#!/usr/bin/env python3
"""tools/fuzz_index.py [seconds] [seed] -- random collections through lime_build_index against lime_amd/builder.py (bit-exact), on the GPU
box: the generator of tests/test_index_edges_gpu.py::test_seeded_fuzz (tests/index_cases.py: fuzz_collection) in a time-boxed loop.
Alphabet sizes on both sides of every packing width, document lengths around k_syms * 2^r, planted repeats, identical documents, any
terminator byte, lcp_cap; stops at the first difference with the call that reproduces it.  Not part of the test suite (a soak)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lime_amd
from lime_amd.builder import build_arrays_sa
from tests import index_cases as IC

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
t_end = time.time() + budget
t_print = time.time()
stats = {"cases": 0, "positions": 0, "capped": 0, "rounds": 0}
ctx = lime_amd.Context()
try:
    case = 0
    while time.time() < t_end:
        reads, genomes, term, cap, desc = IC.fuzz_collection(seed, case)
        want = IC.capped(build_arrays_sa(reads, genomes, term), cap)
        diff = IC.first_difference(ctx.build_index(reads, genomes, term, cap), want)
        if diff is not None:
            sys.exit(f"fuzz_index: tests.index_cases.fuzz_collection({seed}, {case}) [{desc}]: {diff}")
        stats["cases"] += 1; stats["positions"] += len(want[0]); stats["capped"] += cap > 0; stats["rounds"] += ctx.index_info()["rounds"]
        case += 1
        if time.time() - t_print > 30:                   # a line now and then: a silent GPU run is taken for hung
            print("fuzz_index ...", stats, flush=True); t_print = time.time()
finally:
    ctx.close()
print("fuzz_index ok:", stats, "in", round(budget), "s, seed", seed)
