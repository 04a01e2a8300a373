"""Every read normalised by its own length, without a GPU: the numpy models of tests/readnorm_cases.py against the fixed-norm models they
stand on, and lime_classify_mem_norms (the host reference of the per-read device path) against lime_classify_mem and against model_decide,
read by read through the groups of equal norms, and byte for byte on the goldens where the norms are constant.  Host code."""
import glob
import os

import numpy as np
import pytest

from tests import classify_cases as CC
from tests import readnorm_cases as RN
from tests import shard_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = sorted(glob.glob(os.path.join(GOLDEN, "classify_*.npz")))


# ---- the models themselves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", (1, 16, 255))
def test_model_of_the_norms(alpha):
    lengths = [0, 1, alpha - 1, alpha, alpha + 1, 100, 255, 256, 1000]
    norm, long_ = RN.norms_of(lengths, alpha)
    for n, L in zip(norm, lengths):
        if L > 255:
            continue
        assert n == (L + 1 - alpha if L >= alpha else 1), (alpha, L, n)
        assert 1 <= n <= 255
    assert list(long_) == [i for i, L in enumerate(lengths) if L > 255] and {7, 8} <= set(int(i) for i in long_)
    assert RN.norms_of([100], 16)[0][0] == 85                      # the reference's norm of the example (ClusterBWT_DA.cpp:555)
    assert list(RN.doc_off_of([3, 0, 2])) == [0, 3, 3, 5]


@pytest.mark.parametrize("beta", RN.BETAS)
def test_pass_table_is_the_fixed_norm_test_for_every_norm(beta):
    t = RN.pass_table(beta)
    assert t.shape == (256, 256) and not t[0].any()
    for n in range(1, 256):
        assert np.array_equal(t[n], HC.passes(np.arange(256), n, beta)), (beta, n)
    table, norms, want = RN.threshold_rows(beta)
    assert set(int(x) for x in norms) == set(range(1, 256)) and want.any() and (~want).any()
    got = RN.choose_norms(table, norms, beta)
    assert np.array_equal(np.diff(got[1].astype(np.int64)) > 0, want)          # (every row holds a non-zero cell but maximum 0, which fails)
    assert HC.same_lists(got, RN.choose_by_groups(table, norms, beta))


def test_choose_with_per_read_norms_equals_the_fixed_norm_choose_by_groups():
    for case in range(40):
        rng = np.random.default_rng([RN.SEED, 1, case])
        table = HC.sparse_table(int(rng.integers(1, 120)), int(rng.integers(1, 60)), rng, density=float(rng.choice([0.0, 0.05, 0.4])))
        norms = rng.choice([1, 17, 50, 85, 100, 255], size=len(table)).astype(np.uint8)
        for beta in RN.BETAS + (-1.0,):
            assert HC.same_lists(RN.choose_norms(table, norms, beta), RN.choose_by_groups(table, norms, beta)), (case, beta)
        const = np.full(len(table), HC.NORM, np.uint8)
        assert HC.same_lists(RN.choose_norms(table, const, HC.BETA), HC.choose(table, HC.NORM, HC.BETA)), case


# ---- lime_classify_mem_norms --------------------------------------------------------------------------------------------------------
def _tax_file(col, tmp_path):
    p = str(tmp_path / "lineage.csv")
    open(p, "wb").write(col["tax"])
    return p


def check_by_groups(col, read_norms, combos, tmp_path, tag):
    """lime_classify_mem_norms on the per-read lists against lime_classify_mem and model_decide, each run once per group of equal norms on
    the fixed-norm lists of the whole collection"""
    from lime_amd import api
    n_files, n_targ = len(col["sims"]), col["n_targ"]
    betas = [col["beta"]] * n_files
    lists = RN.lists_norms(col, read_norms)
    tax = _tax_file(col, tmp_path)
    for binary, higher, rank in combos:
        where = (tag, binary, higher, rank)
        tx = api.load_taxonomy(tax, rank, higher, n_targ)
        v, counts = api.classify_mem(lists, [0] * n_files, betas, n_targ, tx, binary, read_norms=read_norms)
        mem = RN.by_groups(col, read_norms, lambda ls, ns: api.classify_mem(ls, ns, betas, n_targ, tx, binary)[0])
        want = np.array([m.tobytes() for m in mem])
        got = np.array([v[r].tobytes() for r in range(len(v))])
        assert np.array_equal(got, want), (where, "against lime_classify_mem", int(np.nonzero(got != want)[0][0]))
        rep = RN.model_by_groups(col, read_norms, rank, higher, binary)
        assert CC.same_verdicts(rep, v) is None, (where, "against model_decide", CC.same_verdicts(rep, v))
        assert counts == [sum(1 for x in rep if x.type == t) for t in "CUAH"], where
        tx.close()


def test_mem_norms_by_groups_on_mixed_tolerance_tables(tmp_path):
    """reads of norm 50 and of norm 100 mixed, counts on the 0.02 tolerance of both: every COMBOS"""
    for n_files in (2, 4):
        col, read_norms = RN.mixed_tolerance(n_files, 60, 70, seed=33 + n_files)
        assert {int(x) for x in read_norms[0]} == {50, 100}
        check_by_groups(col, read_norms, CC.COMBOS, tmp_path, col["name"])


def test_mem_norms_by_groups_on_fuzz_collections(tmp_path):
    """fuzz_collection seeds with a norm per mate and read drawn from {1, 50, 85, 100, 255} (mates of one read differ): every COMBOS on
    a few seeds, the seed's own combination on the rest"""
    mixed, seen = 0, set()
    for seed in range(30):
        col, rank, higher, binary = CC.fuzz_collection(seed)
        n_files, n_reads = len(col["sims"]), col["sims"][0].shape[0]
        rng = np.random.default_rng([RN.SEED, 2, seed])
        some = tuple(int(x) for x in rng.choice(RN.MATE_NORMS, size=3, replace=False))     # (three of the five per seed: at most nine groups)
        seen |= set(some)
        read_norms = RN.draw_norms(n_files, n_reads, rng, some)
        rows = [l.split(";") for l in col["tax"].decode().split("\n")[1:-1]]
        full = all(f[q] != "" for f in rows for q in (1, 2, 4))              # COMBOS' ranks need a taxon per genome
        combos = CC.COMBOS if (seed < 4 and full) else ((binary, higher, rank),)
        check_by_groups(col, read_norms, combos, tmp_path, f"fuzz_collection({seed})")
        if n_files == 4:
            mixed += int((read_norms[0] != read_norms[2]).any())
    assert mixed >= 5 and seen == set(RN.MATE_NORMS)


def test_a_list_without_read_norms_uses_its_one_norm(tmp_path):
    from lime_amd import api
    col = CC.near_tie_tables(4, 40, 130, seed=32)
    n_files, n_targ, n_reads = 4, col["n_targ"], 40
    rng = np.random.default_rng([RN.SEED, 3])
    per = rng.choice(RN.MATE_NORMS, size=n_reads).astype(np.uint8)
    read_norms = [per, per, np.full(n_reads, col["norm"], np.uint8), np.full(n_reads, col["norm"], np.uint8)]
    lists = RN.lists_norms(col, read_norms)
    tx = api.load_taxonomy(_tax_file(col, tmp_path), 1, 1, n_targ)
    betas = [col["beta"]] * 4
    all_given, _ = api.classify_mem(lists, [0] * 4, betas, n_targ, tx, True, read_norms=read_norms)
    some_null, _ = api.classify_mem(lists, [0, 0, col["norm"], col["norm"]], betas, n_targ, tx, True, read_norms=[per, per, None, None])
    assert all_given.tobytes() == some_null.tobytes()
    rep = RN.model_by_groups(col, read_norms, 1, 1, 1)
    assert CC.same_verdicts(rep, some_null) is None
    with pytest.raises(api.LimeError) as e:                                  # a list without read norms needs its one norm
        api.classify_mem(lists, [0] * 4, betas, n_targ, tx, True, read_norms=[per, per, None, None])
    assert e.value.code == -1 and "bad list" in str(e.value)
    with pytest.raises(api.LimeError) as e:                                  # NORM_PER_READ is the sample calls' alone
        api.classify_mem(lists, [api.NORM_PER_READ] * 4, betas, n_targ, tx, True)
    assert e.value.code == -1 and "LIME_NORM_PER_READ" in str(e.value)
    tx.close()


@pytest.mark.parametrize("case", CASES, ids=[os.path.basename(c)[9:-4] for c in CASES])
def test_constant_norms_give_classify_mem_byte_for_byte_on_goldens(case, tmp_path):
    from lime_amd import api
    assert len(CASES) == 9
    g = np.load(case)
    norm, beta = int(g["norm"]), float(g["beta"])
    n_files, n_reads, n_targ = g["sims"].shape
    lists = [CC.lists_of(s, norm, beta) for s in g["sims"]]
    tax = str(tmp_path / "lineage.csv")
    open(tax, "wb").write(g["tax"].tobytes())
    const = [np.full(n_reads, norm, np.uint8)] * n_files
    for binary, higher, rank in ((1, 0, 1), (0, 0, 1), (1, 1, 1), (0, 1, 2), (1, 0, 0)):
        tx = api.load_taxonomy(tax, rank, higher, n_targ)
        want, cw = api.classify_mem(lists, [norm] * n_files, [beta] * n_files, n_targ, tx, binary)
        got, cg = api.classify_mem(lists, [0] * n_files, [beta] * n_files, n_targ, tx, binary, read_norms=const)
        assert got.tobytes() == want.tobytes() and cg == cw, (binary, higher, rank)
        outp = str(tmp_path / "norms.txt")
        api.write_classification(outp, got)
        assert open(outp, "rb").read() == g[f"out_b{binary}_h{higher}_r{rank}"].tobytes(), (binary, higher, rank)
        tx.close()
