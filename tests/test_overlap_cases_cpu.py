"""Without a GPU: the two models of tests/overlap_cases.py against each other; lime_pair_overlap_trim (the loop form in the library's host
code) against them on every hand-made case, on the mismatch thresholds, on the trap and on 400 seeded collections, the inserts compared
exactly (which pins "largest" where nothing is cut); the consequences the rule states; every refusal; LiME_fasta's usage errors that need
no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import overlap_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lime_amd", "bin")


def _host_cut(r1, r2, O, E):
    from lime_amd import api
    return api.overlap_trim(*V.records(r1), *V.records(r2), O, E)


def _same_as_models(r1, r2, O, E, what):
    o1, o2, ins, info = V.cut_model(r1, r2, O, E)
    assert V.cut_model(r1, r2, O, E, insert=V.insert_masks) == (o1, o2, ins, info), what
    t1, f1, t2, f2, got_ins, got = _host_cut(r1, r2, O, E)
    for (w_text, w_off), text, off in ((V.records(o1), t1, f1), (V.records(o2), t2, f2)):
        assert np.array_equal(off, w_off) and np.array_equal(text, w_text), (what, O, E)
    assert got_ins.tolist() == ins, (what, got_ins.tolist(), ins)
    assert got == info, (what, got, info)
    return ins, info


@pytest.mark.parametrize("name", sorted(V.hand_cases()))
def test_lime_pair_overlap_trim_on_the_hand_made_cases(name):
    r1, r2, O, E = V.hand_cases()[name]
    _same_as_models(r1, r2, O, E, name)


def test_what_the_hand_made_cases_are_for():
    h = V.hand_cases()
    ins = lambda name: V.cut_model(*h[name])[2]                                 # noqa: E731
    assert ins("every insert of 130 / 100") == [0] + list(range(30, 201)) + [0]  # every candidate is found, the two outside are not
    r1, r2, O, E = h["every insert of 130 / 100"]
    o1, o2, got, info = V.cut_model(r1, r2, O, E)
    assert [len(x) for x in o1] == [130] + [min(130, I) for I in range(30, 201)] + [130]
    assert [len(x) for x in o2] == [100] + [min(100, I) for I in range(30, 201)] + [100]
    assert info["n_overlap"] == 171 and info["n_cut"] == 100                    # an I of 130 and above cuts nothing
    assert ins("first, last and 64th candidate of the steps") == [170, 165, 164, 107, 106, 101, 100, 43, 42, 37, 36, 30]
    assert ins("N opposite N") == [0, 80, 0]       # N opposite N is a mismatch: one of 80 places, at E = 0
    assert ins("lower case") == [80, 80, 80]
    assert ins("other bytes") == [80]              # five of 80 places hold no base: 5 <= 8
    assert ins("an empty mate") == [0, 0, 0, 1]
    assert ins("every pair empty") == [0] * 5
    assert ins("mates shorter than O") == [0, 0, 30, 0]
    assert ins("an ordinary overlap cuts nothing") == [100, 101, 150, 170, 0]
    assert V.cut_model(*h["an ordinary overlap cuts nothing"])[3]["n_cut"] == 0
    assert ins("O of 1") == [1, 0, 0]
    # (AC)* against (GT)*: every even I agrees everywhere, the largest candidate wins; A* against T*: every I
    assert ins("periodic reads") == [170, 170, 150, 140]


def test_the_consequences_of_the_rule():
    """nothing is cut below O symbols, no read is emptied, an empty mate gives no overlap, read indices never change"""
    for case in range(0, V.FUZZ_CASES, 8):
        r1, r2, O, E = V.fuzz_collection(V.SEED, case)
        o1, o2, ins, info = V.cut_model(r1, r2, O, E, insert=V.insert_masks)
        assert len(o1) == len(r1) and len(o2) == len(r2)
        for a, b, x, y, I in zip(r1, r2, o1, o2, ins):
            assert a.startswith(x) and b.startswith(y)
            assert len(x) >= min(len(a), O) and len(y) >= min(len(b), O)
            assert (len(x) > 0) == (len(a) > 0) and (len(y) > 0) == (len(b) > 0)
            if not a or not b:
                assert I == 0
            if I:
                n, mis = V.mis_at(a, b, I)
                assert O <= I <= len(a) + len(b) - O and n >= O and mis <= (n * E) // 100
                for J in range(I + 1, len(a) + len(b) - O + 1):                  # none above it is admissible
                    n, mis = V.mis_at(a, b, J)
                    assert n < O or mis > (n * E) // 100


def test_the_mismatch_thresholds():
    cases = V.threshold_cases()
    assert len(cases) == 3 * len(V.THRESHOLD_N) * 2
    for name, (a, b, O, E, n, n_err) in cases.items():
        assert V.mis_at(a, b, n) == (n, n_err), name
        ins, _ = _same_as_models([a], [b], O, E, name)
        assert (ins[0] == n) == (n_err <= (n * E) // 100), (name, ins)


def test_the_trap_the_larger_insert_wins_until_it_has_one_mismatch_too_many():
    a, b, O, E, small, large = V.trap(5)
    assert V.mis_at(a, b, small) == (60, 0) and V.mis_at(a, b, large) == (50, 5) and (50 * E) // 100 == 5
    ins, info = _same_as_models([a], [b], O, E, "the trap at the threshold")
    assert ins == [large] and info["n_cut"] == 0       # largest, not best-scoring: nothing is cut
    a, b, O, E, small, large = V.trap(6)
    assert V.mis_at(a, b, small) == (60, 0) and V.mis_at(a, b, large) == (50, 6)
    ins, info = _same_as_models([a], [b], O, E, "the trap one over")
    assert ins == [small] and info["n_cut"] == 1


def test_the_generators_yield():
    pairs, cut, whole, none = V.fuzz_yield()
    print("pairs", pairs, "cut", cut, "overlap without a cut", whole, "none", none)
    assert V.fuzz_yield(insert=V.insert_loop, cases=40)[0] > 0


@pytest.mark.parametrize("part", range(8))
def test_lime_pair_overlap_trim_on_seeded_collections(part):
    for case in range(part, V.FUZZ_CASES, 8):
        r1, r2, O, E = V.fuzz_collection(V.SEED, case)
        _same_as_models(r1, r2, O, E, f"fuzz_collection({V.SEED}, {case})")


def test_unequal_long_mates_past_the_kept_words():
    rng = np.random.default_rng([V.SEED, 5])
    for La, Lb, I in ((1000, 700, 650), (700, 1000, 1200), (513, 511, 512), (2000, 40, 35)):
        a, b = V.plant(rng, V.bases(rng, I), I, n_err=3, La=La, Lb=Lb)
        ins, _ = _same_as_models([a], [b], 30, 10, (La, Lb, I))
        assert ins == [I]


def test_refusals():
    from lime_amd import _lib, api
    lib = _lib.load()
    r = [b"ACGT" * 10]
    for O, E, word in ((0, 10, "overlap"), (30, 51, "0 .. 50")):
        with pytest.raises(api.LimeError) as e:
            _host_cut(r, r, O, E)
        assert e.value.code == _lib.ERR_ARG and word in str(e.value) and str(e.value).count("lime_pair_overlap_trim:") == 1
    assert _host_cut(r, r, 1, 50)[5]["n_pairs"] == 1
    with pytest.raises(api.LimeError) as e:
        api.overlap_trim(np.zeros(4, np.uint8), np.array([0, 3, 2], np.uint64), np.zeros(4, np.uint8), np.array([0, 2, 4], np.uint64), 3, 10)
    assert e.value.code == _lib.ERR_ARG and "decreases" in str(e.value)
    with pytest.raises(api.LimeError) as e:
        api.overlap_trim(np.zeros(4, np.uint8), np.array([0, 2, 4], np.uint64), np.zeros(4, np.uint8), np.array([1, 2, 4], np.uint64), 3, 10)
    assert e.value.code == _lib.ERR_ARG and "start at 0" in str(e.value)
    with pytest.raises(ValueError):
        api.overlap_trim(np.zeros(4, np.uint8), np.array([0, 4], np.uint64), np.zeros(4, np.uint8), np.array([0, 2, 4], np.uint64), 3, 10)
    assert lib.lime_pair_overlap_trim(None, None, None, None, 0, 30, 10, None, None, None, None, None, None) == _lib.ERR_ARG
    p = [C.c_void_p(1) for _ in range(5)]
    oi = _lib.OverlapInfo(7, 7, 7, 7, 7)
    off = np.zeros(1, np.uint64)
    assert lib.lime_pair_overlap_trim(None, off.ctypes.data, None, off.ctypes.data, 0, 0, 10, *[C.byref(x) for x in p], C.byref(oi)) == _lib.ERR_ARG
    assert all(x.value is None for x in p) and oi.n_pairs == 0                 # a refusal leaves every output cleared
    assert lib.lime_seq_reader_set_overlap(None, None, 30, 10) == _lib.ERR_ARG and lib.lime_seq_reader_overlap_info(None, None) == _lib.ERR_ARG
    assert lib.lime_seq_reader_next_pair(None, None, 1, None, None, None) == _lib.ERR_ARG
    assert lib.lime_docs_trim_overlap_dev(None, None, None, 30, 10, None, None, None, None, None) == _lib.ERR_ARG


def test_no_pairs_the_insert_array_is_optional_and_an_unchanged_collection():
    from lime_amd import _lib
    t1, f1, t2, f2, ins, info = _host_cut([], [], 30, 10)
    assert len(t1) == 0 and len(t2) == 0 and list(f1) == [0] and list(f2) == [0] and len(ins) == 0 and info == {k: 0 for k in V.INFO_KEYS}
    r1, r2 = [b"TTTTTTTT", b"", b"GGGG"], [b"TTTTTTTT", b"ACGT", b""]
    t1, f1, t2, f2, ins, info = _host_cut(r1, r2, 3, 0)
    assert np.array_equal(t1, V.records(r1)[0]) and np.array_equal(t2, V.records(r2)[0]) and ins.tolist() == [0, 0, 0]
    assert info == {"n_pairs": 3, "n_overlap": 0, "n_cut": 0, "symbols_in": 24, "symbols_out": 24}
    lib = _lib.load()
    (x1, o1), (x2, o2) = V.records(r1), V.records(r2)
    p = [C.c_void_p() for _ in range(4)]
    assert lib.lime_pair_overlap_trim(x1.ctypes.data, o1.ctypes.data, x2.ctypes.data, o2.ctypes.data, 3, 3, 0, *[C.byref(x) for x in p], None, None) == 0
    for x in p:
        lib.lime_free(x)


def test_the_new_symbols_are_declared_and_exported():
    from lime_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    for n in ("lime_pair_overlap_trim", "lime_docs_trim_overlap_dev", "lime_seq_reader_set_overlap", "lime_seq_reader_next_pair", "lime_seq_reader_overlap_info"):
        assert n in _lib.SYMBOLS and hasattr(lib, n) and re.search(r"\b%s\(" % n, header), n
    assert C.sizeof(_lib.OverlapInfo) == 40


# ---- the program's usage errors: checked before a device is opened ----
def _lime_fasta(args):
    assert os.path.exists(os.path.join(BIN, "LiME_fasta"))
    return subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=120)


BASE = ["--gidx", "g.gidx", "--lineage", "l.csv"]


def test_trim_overlap_with_one_reads_file_is_the_usage_error(tmp_path):
    out = str(tmp_path / "no.txt")
    p = _lime_fasta(["r.fastq"] + BASE + ["--readlen", "auto", "--out", out, "--trim-overlap", "30"])
    assert p.returncode == 1 and b"Error usage" in p.stderr and b"--trim-overlap" in p.stderr and not os.path.exists(out)


def test_trim_overlap_with_a_numeric_readlen_is_the_usage_error(tmp_path):
    out = str(tmp_path / "no.txt")
    p = _lime_fasta(["r_1.fastq", "r_2.fastq"] + BASE + ["--readlen", "100", "--out", out, "--trim-overlap", "30"])
    assert p.returncode == 1 and b"Error usage" in p.stderr and not os.path.exists(out)


@pytest.mark.parametrize("extra", [["--trim-overlap", "0"], ["--trim-overlap", "30,51"], ["--trim-overlap"], ["--trim-overlap", ""], ["--trim-overlap", "x"],
                                   ["--trim-overlap", "30,"], ["--trim-overlap", ",10"], ["--trim-overlap", "30,10,1"], ["--trim-overlap", "-3"]])
def test_a_bad_overlap_option_is_the_usage_error(tmp_path, extra):
    out = str(tmp_path / "no.txt")
    p = _lime_fasta(["r_1.fastq", "r_2.fastq"] + BASE + ["--readlen", "auto", "--out", out] + extra)
    assert p.returncode == 1 and b"Error usage" in p.stderr and not os.path.exists(out)


def test_good_overlap_options_get_past_the_usage_check(tmp_path):
    """the same line with legal values ends later, at the reads file that is not there or at the missing device: not at the usage text"""
    out = str(tmp_path / "no.txt")
    for extra in (["--trim-overlap", "30"], ["--trim-overlap", "1,50"], ["--trim-overlap", "30,0", "--trim-adapter", "ACGT", "--min-len", "20"]):
        p = _lime_fasta([str(tmp_path / "r_1.fastq"), str(tmp_path / "r_2.fastq")] + BASE + ["--readlen", "auto", "--out", out] + extra)
        assert p.returncode != 0 and b"Error usage" not in p.stderr and not os.path.exists(out)
