"""The collections of tests/classify_cases.py without a GPU: the model of the decision (model_decide: sets, dicts, np.float32) against the
bytes the reference's own Classify builds wrote (every tests/golden/classify_*.npz, every key) and against lime_classify_mem; what the wide
goldens and the hand-built placements must cover, computed from the model's per-read report alone.  Host code."""
import functools
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import classify_cases as CC  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = sorted(glob.glob(os.path.join(GOLDEN, "classify_*.npz")))
KEYS = [f"out_b{b}_h{h}_r{r}" for b in (1, 0) for h in (0, 1) for r in (0, 1, 2, 4) if not (h and r == 0)]


@functools.lru_cache(maxsize=None)
def golden_reports(name):
    """{key: (Reports, wide Reports or None)} of one golden, and its lists: computed once, shared, never changed"""
    g = np.load(os.path.join(GOLDEN, f"classify_{name}.npz"))
    norm, beta = int(g["norm"]), float(g["beta"])
    n_files, _, n_targ = g["sims"].shape
    lists = [CC.lists_of(s, norm, beta) for s in g["sims"]]
    out = {}
    for key in KEYS:
        assert key in g.files, f"classify_{name}.npz lacks {key}: make it again with the reference's builds (tests/golden/make_golden_classify.py)"
        binary, higher, rank = int(key[5]), int(key[8]), int(key[11:])
        tax = CC.Tax(g["tax"].tobytes(), rank, higher, n_targ)
        rep = CC.model_decide(lists, [norm] * n_files, [beta] * n_files, n_targ, tax, binary)
        wide = CC.model_decide(lists, [norm] * n_files, [beta] * n_files, n_targ, tax, binary, wide=True) if name.startswith("tol") else None
        out[key] = (rep, wide)
    return g, lists, out


def _mem(col_lists, norm, beta, n_targ, tax_path, binary, higher, rank, tmp_path):
    from lime_amd import api
    tx = api.load_taxonomy(tax_path, rank, higher, n_targ)
    v, counts = api.classify_mem(col_lists, [norm] * len(col_lists), [beta] * len(col_lists), n_targ, tx, binary)
    outp = str(tmp_path / "mem.txt")
    api.write_classification(outp, v)
    tx.close()
    return v, counts, open(outp, "rb").read()


@pytest.mark.parametrize("case", CASES, ids=[os.path.basename(c)[9:-4] for c in CASES])
def test_model_reference_and_host_agree_on_goldens(case, tmp_path):
    g, lists, reports = golden_reports(os.path.basename(case)[9:-4])
    norm, beta = int(g["norm"]), float(g["beta"])
    n_targ = g["sims"].shape[2]
    tax = str(tmp_path / "lineage.csv")
    open(tax, "wb").write(g["tax"].tobytes())
    for key in KEYS:
        binary, higher, rank = int(key[5]), int(key[8]), int(key[11:])
        rep = reports[key][0]
        assert CC.classification_bytes(rep) == g[key].tobytes(), (key, "model against the reference")
        v, counts, got = _mem(lists, norm, beta, n_targ, tax, binary, higher, rank, tmp_path)
        assert got == g[key].tobytes(), (key, "lime_classify_mem against the reference")
        assert CC.same_verdicts(rep, v) is None, (key, CC.same_verdicts(rep, v))
        assert counts == [sum(1 for x in rep if x.type == t) for t in "CUAH"]


def check_collection(col, combos, tmp_path, tag=""):
    lists = CC.collection_lists(col)
    tax = str(tmp_path / "lineage.csv")
    open(tax, "wb").write(col["tax"])
    n_files = len(col["sims"])
    for binary, higher, rank in combos:
        rep = CC.model_decide(lists, [col["norm"]] * n_files, [col["beta"]] * n_files, col["n_targ"], CC.Tax(col["tax"], rank, higher, col["n_targ"]), binary)
        v, _, got = _mem(lists, col["norm"], col["beta"], col["n_targ"], tax, binary, higher, rank, tmp_path)
        where = (tag or col["name"], binary, higher, rank)
        assert CC.same_verdicts(rep, v) is None, (where, CC.same_verdicts(rep, v))
        assert got == CC.classification_bytes(rep), where
    return lists


def generator_collections():
    yield CC.near_tie_tables(2, 60, 130, seed=31)
    yield CC.near_tie_tables(4, 60, 200, seed=32)
    for norm in (50, 100):
        for n_files in (2, 4):
            yield CC.tolerance_tables(n_files, 90, 70, seed=33 + n_files, norm=norm)
    yield CC.beta0_tables(4, 45, 129, seed=35)
    for n_files in (2, 4):
        yield CC.placement_cases(n_files)


def test_model_and_host_agree_on_generators(tmp_path):
    for col in generator_collections():
        check_collection(col, CC.COMBOS, tmp_path)


@pytest.mark.parametrize("n_targ", CC.EVERY_GENOME_N)
def test_model_and_host_agree_on_every_genome_cases(n_targ, tmp_path):
    for kind in CC.EVERY_GENOME_TAX:
        for n_files in (2, 4):
            col = CC.every_genome_cases(n_targ, kind, n_files)
            check_collection(col, CC.COMBOS, tmp_path)
            lists = CC.collection_lists(col)
            rep = CC.model_decide(lists, [64] * n_files, [0.0] * n_files, n_targ, CC.Tax(col["tax"], 1, 1, n_targ), 1)
            if n_targ > 2 and kind != "one":
                assert sum(x.every_genome for x in rep[1:7]) >= 3, col["name"]           # (a genome in two lists of a strand sums to 2 / 64: not below TOL)
                assert {x.type for x in rep[1:7] if x.every_genome} == {{"two": "A", "higher": "H", "last": "A"}[kind]}, col["name"]
            else:                                            # one taxon (or one or two genomes): rule 1 decides
                assert all(x.rule == 1 for x in rep[:2]), col["name"]


def test_chosen_rank_itself_decides_with_a_shifted_lineage(tmp_path):
    col = CC.shifted_lineage_case()
    lists = check_collection(col, ((1, 1, 1), (0, 1, 1), (1, 0, 1)), tmp_path)
    rep = CC.model_decide(lists, [85, 85], [0.0, 0.0], 6, CC.Tax(col["tax"], 1, 1, 6), 1)
    assert (rep[0].type, rep[0].h_rank, rep[0].taxon) == ("H", 0, 14), dict(rep[0])
    assert (rep[1].type, rep[1].h_rank) == ("H", 2), dict(rep[1])


def test_model_and_host_agree_on_stride_case(tmp_path):
    col = CC.stride_case()
    assert col["sims"][0].shape == (16384 + 5, 3)
    lists = check_collection(col, ((1, 1, 1), (0, 0, 0)), tmp_path)
    rep = CC.model_decide(lists, [85, 85], [0.1, 0.1], 3, CC.Tax(col["tax"], 1, 1, 3), 1)
    edge = [0, 1, 2, 3, 4, 16384, 16385, 16386, 16387, 16388]
    rows = {tuple(s[r].tobytes() for s in col["sims"]) for r in edge}
    assert len(rows) == 10 and all(x.T >= 4 for x in (rep[r] for r in edge))                  # distinct, non-trivial
    assert len({(x.type, x.taxon, float(x.sim), x.rule) for x in (rep[r] for r in edge)}) >= 4


def test_model_and_host_agree_on_200_fuzz_seeds(tmp_path):
    for seed in range(200):
        col, rank, higher, binary = CC.fuzz_collection(seed)
        assert col["sims"][0].shape[0] <= 64 or "tol" in col["name"]
        assert col["n_targ"] <= 300 and len(col["sims"]) in (2, 4)
        check_collection(col, ((binary, higher, rank),), tmp_path, tag=f"fuzz_collection({seed})")


def test_wide_goldens_cover_the_kernels_widths():
    """Conditions on the new goldens, from the model's report alone.  H is decided at the five higher ranks above the species; the species
    itself (index 0) cannot decide: it is reached with rank 1 only, where it is the column at_rank was read from, so genomes that differ
    at the rank differ there too.  The condition states that as well."""
    wide = {}                                                # outcome -> {(case, read)} with T > 64
    h_ranks, every, longest = set(), set(), 0
    for name in CC.NEW_GOLDENS:
        g, _, reports = golden_reports(name)
        n_targ = g["sims"].shape[2]
        depends_on_float32 = set()
        for key, (rep, rep_wide) in reports.items():
            for r, x in enumerate(rep):
                if x.T > 64:
                    wide.setdefault((x.rule, x.type), set()).add((name, r))
                if x.type == "H":
                    h_ranks.add(x.h_rank)
                if x.every_genome and n_targ > 64:
                    every.add((name, r))
                longest = max(longest, x.longest_row)
                if rep_wide is not None and (x.type, x.taxon, x.rule) != (rep_wide[r].type, rep_wide[r].taxon, rep_wide[r].rule):
                    depends_on_float32.add(r)
        if name.startswith("tol"):
            assert len(depends_on_float32) >= 20, (name, len(depends_on_float32))
    for outcome in ((1, "C"), (2, "C"), (3, "C"), (3, "H"), (3, "A")):
        assert len(wide.get(outcome, ())) >= 10, (outcome, len(wide.get(outcome, ())))
    assert h_ranks == {1, 2, 3, 4, 5}, h_ranks
    assert len(every) >= 5 and longest >= 65, (len(every), longest)
    t_seen = {x.T for name in CC.NEW_GOLDENS for x in golden_reports(name)[2][KEYS[0]][0]}
    assert {63, 64, 65, 127, 128, 129} <= t_seen and max(t_seen) > 256


def test_every_placement_is_present_and_decides_as_built():
    labels, verdict = [], {}
    for n_files in (2, 4):
        col = CC.placement_cases(n_files)
        lists = CC.collection_lists(col)
        rep = CC.model_decide(lists, [col["norm"]] * n_files, [0.0] * n_files, col["n_targ"], CC.Tax(col["tax"], 1, 0, col["n_targ"]), 1)
        for r, lab in enumerate(col["labels"]):
            labels.append(lab)
            verdict.setdefault(lab, []).append(rep[r])
            if lab.startswith("last_element"):
                assert rep[r].T == int(lab.split("_T")[1]), (lab, rep[r].T)
        up = CC.model_decide(lists, [col["norm"]] * n_files, [0.0] * n_files, col["n_targ"], CC.Tax(col["tax"], 1, 1, col["n_targ"]), 1)
        hole = up[col["labels"].index(f"shared_hole_of{n_files}")]
        assert (hole.type, hole.h_rank, hole.taxon) == ("H", 3, 4000 + CC.HOLE_PAIR[0] // 16), dict(hole)
    for want in CC.PLACEMENTS:
        assert want in labels, want
    for lab, reps in verdict.items():
        if lab.startswith("last_element_rule1"):
            assert all((x.type, x.rule, x.taxon) == ("C", 1, 1000 + 419 // 2) for x in reps), lab        # the last element's species
        if lab.startswith("last_element_rule3"):
            assert all((x.type, x.rule) == ("A", 3) for x in reps), lab
        if lab.startswith("find_row"):
            found = lab.endswith("first") or lab.endswith("last")
            assert all((x.type, x.rule) == (("C", 2) if found else ("A", 3)) for x in reps), lab
            assert all(x.longest_row == max(2, int(lab[8:].split("_")[0])) for x in reps), lab             # (list 0 holds two pairs)
    assert all(x.rule == 3 for lab in ("later_only_of2", "earlier_too_of2", "later_only_of4", "earlier_too_of4") for x in verdict[lab])
