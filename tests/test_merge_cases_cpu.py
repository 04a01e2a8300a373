"""The merge of reads into a prebuilt genome index without a GPU: the Python model of tests/merge_cases.py (the two sides sorted alone,
ranks by text comparison, placement by i + j[i] / k + c[k], same-side lcps from the sides) equals lime_amd/builder.py on every
collection tests/test_merge_edges_gpu.py runs on the device and on the 200 seeded collections of index_cases.fuzz_collection; the
collections hold what their tests say they hold; and lime_gindex_probe (pure host code) accepts and refuses the files it should."""
import numpy as np
import pytest

from tests import index_cases as IC
from tests import merge_cases as MC


def _check(reads, genomes, term=0, cap=0, what=""):
    from lime_amd.builder import build_arrays
    got, facts = MC.model_merge(reads, genomes, term, cap)
    want = IC.capped(build_arrays(reads, genomes, term), cap)
    diff = IC.first_difference(got, want)
    assert diff is None, f"{what}: {diff}"
    return facts


def test_model_on_ties_and_one_symbol():
    f = _check(*MC.TIES, what="ties")
    # the terminator-only read suffixes and nothing else are below every genome suffix; every other read suffix is above the genomes' terminators
    n_reads, n_refs = len(MC.TIES[0]), len(MC.TIES[1])
    assert f["j"][:n_reads] == [0] * n_reads and min(f["j"][n_reads:]) >= n_refs
    f = _check(*MC.ONE_SYMBOL, what="one symbol")
    assert f["j"][:18] == [0] * 18 and min(f["j"][18:]) >= 8
    for cap in (1, 8, 9):
        _check(*MC.ONE_SYMBOL, cap=cap, what=f"one symbol cap {cap}")


def test_model_on_word_collections():
    for name, (reads, genomes) in MC.word_collections().items():
        f = _check(reads, genomes, what=name)
        # the compares across the sides end at every byte of a word, by a difference and by one side's end
        assert {v % 8 for v in f["cross"]} == set(range(8)), name


@pytest.mark.parametrize("term", [0x00, 0xFF])
def test_model_on_extreme_bytes(term):
    reads, genomes = MC.extreme_bytes()
    assert {0x00, 0xFF} <= set(b"".join(reads)) and {0x00, 0xFF} <= set(b"".join(genomes))
    _check(reads, genomes, term=term, what=f"term {term}")


def test_model_on_degenerate_sides():
    cases = MC.degenerate()
    for name, (reads, genomes) in cases.items():
        f = _check(reads, genomes, what=name)
        ng = sum(len(g) + 1 for g in genomes)
        n_empty = len(reads)                                                   # one terminator-only suffix per read
        if name == "all_reads_below":
            assert set(f["j"][n_empty:]) == {len(genomes)}                     # above the genomes' terminators, below their first symbol
        if name == "all_reads_above":
            assert set(f["j"][n_empty:]) == {ng}


@pytest.mark.parametrize("first", MC.RUN_FIRSTS)
def test_model_on_runs(first):
    reads, genomes = MC.runs_collection(first)
    f = _check(reads, genomes, what=f"run from {first}")
    j, c = f["j"], f["c"]
    assert len(set(j[first:first + MC.RUN_COPIES])) == 1 and j[first - 1] != j[first] and j[first + MC.RUN_COPIES] != j[first]
    assert 0 < j[first] < len(c) - 1                                           # between two genome suffixes
    # 300 neighbouring genome suffixes with no read between them
    flat = max(len(list(g)) for _, g in __import__("itertools").groupby(c))
    assert flat >= 300


def test_model_on_views_and_caps():
    reads, genomes = MC.views_collection()
    assert len(genomes[-1]) < 8 and any(r != genomes[-1] and r.startswith(genomes[-1]) for r in reads)
    assert len(reads[-1]) < 8 and any(g.startswith(reads[-1]) for g in genomes)
    _check(reads, genomes, what="views")
    reads, genomes = MC.caps_collection()
    f = _check(reads, genomes, what="caps")
    assert {14, 15, 16, 17, 18} <= set(f["cross"]) and max(f["cross"]) == 18
    for cap in (1, 15, 16, 17, 1000):
        _check(reads, genomes, cap=cap, what=f"caps {cap}")


def test_model_on_the_seeded_fuzz():
    from lime_amd.builder import build_arrays_sa
    for case in range(IC.FUZZ_CASES):
        reads, genomes, term, cap, desc = IC.fuzz_collection(MC.SEED, case)
        got, _ = MC.model_merge(reads, genomes, term, cap)
        diff = IC.first_difference(got, IC.capped(build_arrays_sa(reads, genomes, term), cap))
        assert diff is None, f"fuzz_collection({MC.SEED}, {case}) [{desc}]: {diff}"
    assert IC.FUZZ_CASES == 200


# ---- the genome index file's header and size checks (lime_gindex_probe) ----
def _probe(tmp_path, data):
    from lime_amd import api
    p = tmp_path / "g.gidx"
    p.write_bytes(data)
    try:
        return api.gindex_probe(str(p))
    except api.LimeError as e:
        return e.code


def test_gindex_probe(tmp_path):
    from lime_amd import _lib
    good = MC.gindex_file_bytes(3, 41, term=36, lcp_cap=20)
    assert len(good) == 64 + 32 + 3 * 176 + 48 + 48
    assert _probe(tmp_path, good) == {"n_docs": 3, "n_text": 41, "lcp_cap": 20, "term": 36}
    assert _probe(tmp_path, MC.gindex_file_bytes(0, 0)) == {"n_docs": 0, "n_text": 0, "lcp_cap": 0, "term": 0}
    assert _probe(tmp_path, MC.gindex_file_bytes(3, 41, magic=b"LGIY")) == _lib.ERR_ARG
    assert _probe(tmp_path, MC.gindex_file_bytes(3, 41, version=2)) == _lib.ERR_ARG
    for k in range(6):                                                         # every section's size against n_docs and n_text
        sizes = [32, 176, 176, 176, 41, 44]
        sizes[k] += 4
        assert _probe(tmp_path, MC.gindex_file_bytes(3, 41, sizes=sizes)) == _lib.ERR_ARG, k
    assert _probe(tmp_path, good[:-1]) == _lib.ERR_IO                          # one byte short
    assert _probe(tmp_path, good[:63]) == _lib.ERR_IO
    assert _probe(tmp_path, good + b"\0") == _lib.ERR_ARG
    from lime_amd import api
    with pytest.raises(api.LimeError) as e:
        api.gindex_probe(str(tmp_path / "no_such_file"))
    assert e.value.code == _lib.ERR_IO
