"""Without a GPU: the two models of tests/filter_cases.py against each other; lime_read_filter (the loop form in the library's host code)
against them on every hand-made case, on the 564-symbol trap, on the mismatch thresholds and on 400 seeded collections; the info counts,
first reason only; every refusal by its text; LiME_fasta's usage errors that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import filter_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lime_amd", "bin")


def _host_filter(reads, p):
    from lime_amd import api
    text, off = F.records(reads)
    return api.read_filter(text, off, **p)


def _same_as_models(reads, p, what):
    want, info = F.filter_model(reads, p)
    assert F.filter_model(reads, p, keep=F.keep_words) == (want, info), what
    w_text, w_off = F.records(want)
    text, off, got = _host_filter(reads, p)
    assert np.array_equal(off, w_off) and np.array_equal(text, w_text), (what, p)
    assert got == info, (what, got, info)
    return info


@pytest.mark.parametrize("name", sorted(F.hand_cases()))
def test_lime_read_filter_on_the_hand_made_cases(name):
    reads, p = F.hand_cases()[name]
    _same_as_models(reads, p, name)


def test_what_the_hand_made_cases_are_for():
    """the expectations written out, so that a mistake shared by both models would show"""
    c = F.hand_cases()
    K = lambda name: [F.keep_loop(r, c[name][1])[0] for r in c[name][0]]
    R = lambda name: [sorted(F.keep_loop(r, c[name][1])[1]) for r in c[name][0]]
    assert K("the trap") == [0]                                             # 9 misses in 564 symbols: 72 <= 564, and the read begins with G
    assert K("a clean tail") == [100, 109, 100]                             # 30 cut, 9 left (T = 10), 10 cut
    assert K("a tail of another base is left") == [130]
    # A then G: the G tail is 20 (the 20 A in front would be 20 misses); alternating AG: half of every tail misses; G then AAA: the G tail
    # of 23 holds 3 misses (24 > 23) and the A tail is shorter than T
    assert K("every base of the mask on its own") == [110, 130, 113]
    assert K("the longest, not the first run") == [60, 60]                  # 2 misses in 42 and 3 in 25 (24 <= 25): across the interruption
    assert K("lower case") == [50, 50]
    assert K("N in the tail is a miss") == [50, 62]                         # 1 in 16 is allowed, 2 in 12 are not
    assert K("the whole read is the tail") == [0, 0, 0, 9]
    assert K("the cap") == [100, 100, 99, 90] and R("the cap") == [[], ["n_capped"], [], ["n_polyx"]]       # (the tail leaves 90: nothing to cap)
    assert K("short") == [30, 0, 0, 0] and R("short") == [[], ["n_short"], ["n_polyx", "n_short"], []]       # (an empty read: counted nowhere)
    # 2 N pass, 3 do not; "ACNNGT" G*20 "NN": the tail of 24 begins at the G of "GT" with T, N, N wrong (24 <= 24), leaving ACNN: 2 N
    assert K("many N") == [10, 0, 4, 0, 0] and R("many N")[2] == ["n_polyx"]
    # AAAC: 49 or 50 of 99 pairs differ; (ACGTTGCA)5 A60: 30 of 99 differ and 3000 >= 2970; N N counts as equal; n < 2 passes; AA fails
    assert K("low complexity") == [0, 50, 100, 0, 100, 1, 2, 0]
    assert R("the first reason alone") == [["n_short"], ["n_short"], ["n_many_n"], ["n_low_complexity"]]
    assert K("every read empty") == [0] * 5 and R("every read empty") == [[]] * 5
    assert K("other bytes") == [0] and R("other bytes") == [["n_many_n", "n_polyx"]]      # 0xC7 is not 'G': only bit 5 is folded away


def test_the_trap():
    """500 G, ACTACTACT, 55 G: a first-run scan stops at t = 55; the rule takes the largest admissible t, 564"""
    assert len(F.TRAP) == 564
    p = F.params(F.G_)
    assert F.keep_loop(F.TRAP, p) == (0, {"n_polyx"}) and F.keep_words(F.TRAP, p) == (0, {"n_polyx"})
    c = F.classes(F.TRAP)
    assert F.tail_loop(c, F.G_, 10) == 564 and F.tail_words(F._words(c), 564, F.G_, 10) == 564
    text, off, info = _host_filter([F.TRAP, b"ACTA" + F.TRAP], p)
    assert list(off) == [0, 0, 4] and text.tobytes() == b"ACTA"
    assert info == {"n_reads": 2, "n_polyx": 2, "n_capped": 0, "n_short": 0, "n_many_n": 0, "n_low_complexity": 0, "symbols_in": 1132, "symbols_out": 4}
    # G, 70 or 71 other bases, then the trap: 79 misses in 635 symbols are allowed (632 <= 635), 80 in 636 are not (640 > 636), and the
    # tail of 564 behind them still is
    front = b"ACT" * 23 + b"AC"
    assert F.keep_loop(b"G" + front[:70] + F.TRAP, p)[0] == 0 and F.keep_loop(b"G" + front + F.TRAP, p)[0] == 72
    _same_as_models([b"G" + front[:70] + F.TRAP, b"G" + front + F.TRAP], p, "the trap behind misses")


def test_the_mismatch_thresholds():
    cases = F.threshold_cases()
    assert len(cases) >= 100
    p = F.params(F.G_, polyx_min=5)
    whole = shorter = 0
    for read, t, m, first_is_x in cases:
        assert len(read) == 200 and sum(x != ord("G") for x in read[200 - t:]) == m and (read[200 - t] == ord("G")) == first_is_x
        n = F.keep_loop(read, p)[0]
        if first_is_x and 8 * m <= t:
            assert n == 200 - t, (t, m)
            whole += 1
        else:
            assert 200 - t < n <= 200, (t, m, first_is_x)                   # the next shorter tail, or none
            shorter += 1
    print("whole tails", whole, "shorter or none", shorter)
    assert whole >= 40 and shorter >= 40
    _same_as_models([c[0] for c in cases], p, "thresholds")


def test_lime_read_filter_on_seeded_collections():
    tot = {k: 0 for k in F.INFO_KEYS}
    for case in range(F.FUZZ_CASES):
        reads, p = F.fuzz_collection(F.SEED, case)
        info = _same_as_models(reads, p, f"fuzz_collection({F.SEED}, {case})")
        for k in tot:
            tot[k] += info[k]
    print(tot)
    assert F.FUZZ_CASES == 400 and min(tot[k] for k in ("n_polyx", "n_capped", "n_short", "n_many_n", "n_low_complexity")) > 300
    assert 0 < tot["symbols_out"] < tot["symbols_in"]


def test_the_generator_mixes_what_it_says():
    rng = np.random.default_rng([F.SEED, 5])
    reads = [F.fuzz_read(rng, 200) for _ in range(600)]
    assert any(r == r[:1] * 200 for r in reads) and any(r == r[:2] * 100 and r[0] != r[1] for r in reads)
    assert any(b"N" in r for r in reads) and any(r.islower() for r in reads)
    tails = [F.tail_loop(F.classes(r), F.G_, 10) for r in reads]
    assert sum(t > 0 for t in tails) > 100 and F.MISS_RATES == (0.0, 0.05, 0.12, 0.125, 0.20)


def test_the_info_counts_and_first_reason_only():
    reads = [b"A" * 20, b"N" * 20, b"N" * 40, b"A" * 40, b"ACGT" * 10, b"", b"ACTA" * 10 + b"G" * 12, b"ACGT" * 20]
    p = F.params(F.G_, max_len=60, min_len=30, max_n=5, min_complexity=30)
    text, off, info = _host_filter(reads, p)
    assert info == {"n_reads": 8, "n_polyx": 1, "n_capped": 1, "n_short": 2, "n_many_n": 1, "n_low_complexity": 1, "symbols_in": 292, "symbols_out": 140}
    assert list(np.diff(off.astype(np.int64))) == [0, 0, 0, 0, 40, 0, 40, 60]
    assert info == F.filter_model(reads, p)[1] == F.filter_model(reads, p, keep=F.keep_words)[1]
    # a read the tail empties with no filter set: n_polyx alone, and n_short too once min_len is set
    assert _host_filter([b"G" * 30], F.params(F.G_))[2]["n_polyx"] == 1
    i = _host_filter([b"G" * 30], F.params(F.G_, min_len=1))[2]
    assert (i["n_polyx"], i["n_short"]) == (1, 1)


def test_max_n_of_0_and_its_off_value_differ():
    reads = [b"ACGTNACGT"]
    assert _host_filter(reads, F.params(max_n=0))[2]["n_many_n"] == 1
    assert _host_filter(reads, F.params(max_n=F.OFF, min_len=1))[2]["n_many_n"] == 0
    assert _host_filter(reads, F.params(max_n=1))[2]["symbols_out"] == 9


BAD = [(dict(polyx=16), "poly-X mask"), (dict(polyx=F.G_, polyx_min=0), "1 .. 255"), (dict(polyx=F.G_, polyx_min=256), "1 .. 255"),
       (dict(min_len=1, min_complexity=101), "0 .. 100"), (dict(), "nothing asked"), (dict(polyx=0, polyx_min=0), "nothing asked")]


def test_refusals():
    from lime_amd import _lib, api
    reads = [b"ACGTACGT"]
    for kw, word in BAD:
        with pytest.raises(api.LimeError) as e:
            _host_filter(reads, F.params(**kw))
        assert e.value.code == _lib.ERR_ARG and word in str(e.value) and str(e.value).count("lime_read_filter:") == 1, (kw, str(e.value))
    for kw in (dict(polyx=15, polyx_min=255), dict(polyx=0, polyx_min=0, max_len=1), dict(min_complexity=100), dict(max_n=0), dict(min_len=1)):
        assert _host_filter(reads, F.params(**kw))[2]["n_reads"] == 1
    with pytest.raises(api.LimeError) as e:
        api.read_filter(np.zeros(4, np.uint8), np.array([0, 3, 2], np.uint64), polyx="G")
    assert e.value.code == _lib.ERR_ARG and "decreases" in str(e.value)
    with pytest.raises(api.LimeError) as e:
        api.read_filter(np.zeros(4, np.uint8), np.array([1, 3, 4], np.uint64), polyx="G")
    assert e.value.code == _lib.ERR_ARG and "start at 0" in str(e.value)
    with pytest.raises(ValueError):
        api.read_filter(np.zeros(4, np.uint8), np.array([0, 4], np.uint64), polyx="GN")
    lib = _lib.load()
    f = _lib.Filter(4, 10, 0, 0, _lib.FILTER_OFF, 0)
    assert lib.lime_read_filter(None, None, 0, C.byref(f), None, None, None) == _lib.ERR_ARG
    pt, po, fi = C.c_void_p(1), C.c_void_p(1), _lib.FilterInfo(7, 7, 7, 7, 7, 7, 7, 7)
    off = np.zeros(1, np.uint64)
    assert lib.lime_read_filter(None, off.ctypes.data, 0, None, C.byref(pt), C.byref(po), C.byref(fi)) == _lib.ERR_ARG
    assert pt.value is None and po.value is None and fi.n_reads == 0 and "NULL" in lib.lime_last_error().decode()
    off2 = np.array([0, 4], np.uint64)
    assert lib.lime_read_filter(None, off2.ctypes.data, 1, C.byref(f), C.byref(pt), C.byref(po), C.byref(fi)) == _lib.ERR_ARG       # symbols without a text
    assert "NULL array" in lib.lime_last_error().decode()
    assert lib.lime_seq_reader_set_filter(None, C.byref(f)) == _lib.ERR_ARG and lib.lime_seq_reader_filter_info(None, None) == _lib.ERR_ARG
    assert lib.lime_docs_filter_dev(None, None, C.byref(f), None, None, None) == _lib.ERR_ARG


def test_no_reads_and_the_counts_of_an_unchanged_collection():
    text, off, info = _host_filter([], F.params(F.G_))
    assert len(text) == 0 and list(off) == [0] and info == {k: 0 for k in F.INFO_KEYS}
    reads = [b"ACGTTGCA", b"", b"TTGACCA"]
    text, off, info = _host_filter(reads, F.params(15, min_len=5, max_n=0, min_complexity=20, max_len=8))
    want = {k: 0 for k in F.INFO_KEYS}
    want.update(n_reads=3, symbols_in=15, symbols_out=15)
    assert np.array_equal(text, F.records(reads)[0]) and info == want


def test_the_polyx_mask_of_a_string():
    from lime_amd import api
    assert [api.polyx_mask(x) for x in (None, "", "A", "c", b"G", "T", "GA", "acgt", 5)] == [0, 0, 1, 2, 4, 8, 5, 15, 5]
    assert api._polyx_arg("G") == (4, 10) and api._polyx_arg("GA,12") == (5, 12) and api._polyx_arg(("T", 3)) == (8, 3)
    for bad in ("", "N", "G,0", "G,256", "G,1,2", ",5"):
        with pytest.raises(ValueError):
            api._polyx_arg(bad)


def test_the_new_symbols_are_declared_and_exported():
    from lime_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    for n in ("lime_read_filter", "lime_docs_filter_dev", "lime_seq_reader_set_filter", "lime_seq_reader_filter_info"):
        assert n in _lib.SYMBOLS and hasattr(lib, n) and re.search(r"\b%s\(" % n, header), n
    assert C.sizeof(_lib.Filter) == 24 and C.sizeof(_lib.FilterInfo) == 64 and "LIME_FILTER_OFF 0xFFFFFFFFu" in header


# ---- the program's usage errors: checked before a device is opened ----
def _lime_fasta(args):
    assert os.path.exists(os.path.join(BIN, "LiME_fasta"))
    return subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=120)


BASE = ["--gidx", "g.gidx", "--lineage", "l.csv"]


@pytest.mark.parametrize("extra", [["--trim-polyx", "G"], ["--max-len", "255"], ["--trim-polyx", "GA,12", "--min-len", "30"]])
def test_a_flag_that_changes_lengths_with_a_numeric_readlen_is_the_usage_error(tmp_path, extra):
    out = str(tmp_path / "no.txt")
    p = _lime_fasta(["r.fastq"] + BASE + ["--readlen", "100", "--out", out] + extra)
    assert p.returncode == 1 and b"Error usage" in p.stderr and b"--trim-polyx" in p.stderr and not os.path.exists(out)


@pytest.mark.parametrize("extra", [["--trim-polyx", ""], ["--trim-polyx", "N"], ["--trim-polyx", "G,"], ["--trim-polyx", "G,0"], ["--trim-polyx", "G,256"],
                                   ["--trim-polyx", ",5"], ["--trim-polyx", "G,5,5"], ["--trim-polyx", "G A"], ["--trim-polyx"], ["--max-len", "0"],
                                   ["--max-len", "x"], ["--min-len", "0"], ["--min-len", "-3"], ["--max-n", "x"], ["--max-n", "-1"], ["--max-n"],
                                   ["--min-complexity", "101"], ["--min-complexity", "0"], ["--min-complexity", "3x"]])
def test_a_bad_filter_option_is_the_usage_error(tmp_path, extra):
    out = str(tmp_path / "no.txt")
    p = _lime_fasta(["r_1.fastq", "r_2.fastq"] + BASE + ["--readlen", "auto", "--out", out] + extra)
    assert p.returncode == 1 and b"Error usage" in p.stderr and not os.path.exists(out)


def test_good_filter_options_get_past_the_usage_check(tmp_path):
    """the same line with legal values ends later, at the reads file that is not there or at the missing device: not at the usage text"""
    out = str(tmp_path / "no.txt")
    for readlen, extra in (("auto", ["--trim-polyx", "ga,12", "--max-len", "255", "--min-len", "30", "--max-n", "0", "--min-complexity", "100"]),
                           ("auto", ["--trim-polyx", "ACGT"]), ("100", ["--min-len", "30", "--max-n", "5", "--min-complexity", "30"]),
                           ("auto", ["--max-n", "4", "--trim-qual", "20", "--trim-adapter", "ACGT"])):
        p = _lime_fasta([str(tmp_path / "r_1.fastq"), str(tmp_path / "r_2.fastq")] + BASE + ["--readlen", readlen, "--out", out] + extra)
        assert p.returncode != 0 and b"Error usage" not in p.stderr and not os.path.exists(out)
