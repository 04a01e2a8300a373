"""Without a GPU: the two models of tests/adapter_cases.py against each other; lime_adapter_trim (the loop form in the library's host code)
against them on every hand-made case, on the mismatch thresholds and on 400 seeded collections; every refusal; LiME_fasta's usage errors
that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import adapter_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lime_amd", "bin")


def _host_trim(reads, adapter, O, E):
    from lime_amd import api
    text, off = A.records(reads)
    return api.adapter_trim(text, off, adapter, O, E)


def _same_as_models(reads, adapter, O, E, what):
    want, info = A.trim_model(reads, adapter, O, E)
    assert A.trim_model(reads, adapter, O, E, keep=A.keep_masks) == (want, info), what
    w_text, w_off = A.records(want)
    text, off, got = _host_trim(reads, adapter, O, E)
    assert np.array_equal(off, w_off) and np.array_equal(text, w_text), (what, O, E)
    assert got == info, (what, got, info)
    return info


@pytest.mark.parametrize("name", sorted(A.hand_cases()))
def test_lime_adapter_trim_on_the_hand_made_cases(name):
    reads, adapter, O, E = A.hand_cases()[name]
    _same_as_models(reads, adapter, O, E, name)


def test_what_the_hand_made_cases_are_for():
    """the expectations written out, so that a mistake shared by both models would show"""
    c = A.hand_cases()
    K = lambda name: [A.keep_loop(r, *c[name][1:]) for r in c[name][0]]
    assert K("every start of 130") == list(range(128)) + [130, 130]         # full and, from 111 on, partial overlaps down to O = 3 symbols;
                                                                            # the last two starts overlap in fewer: no hit
    assert K("a full hit in the last word") == [110]
    assert K("a partial hit of exactly O") == [97] and K("a partial hit of O - 1") == [99]
    assert K("two hits in one word") == [10] and K("two hits in different words") == [40]
    assert K("a later full hit behind an earlier partial non-hit") == [70]
    assert K("a hit at 0") == [0, 0, 0] and K("every read empty") == [0] * 5
    assert K("lower case") == [33, 70]
    assert K("N inside the occurrence") == [50, 70]                         # one N of 20 is within 5 %, two are not
    assert K("a read of only N") == [100, 64, 1]                            # 50 %: an N is a mismatch, not a wildcard
    assert K("other bytes") == [25]                                         # 0xC1 is not 'A': only bit 5 is folded away
    reads, a, O, E = c["every start of 130"]
    assert not A.hits_at(reads[128], a, O, E, 128) and not A.hits_at(reads[129], a, O, E, 129)


def test_the_mismatch_thresholds():
    cases = A.threshold_cases()
    assert len(cases) >= 60
    hit = 0
    for name, (read, a, O, E, k, n_err) in cases.items():
        assert A.hits_at(read, a, O, E, 70) == (n_err <= (k * E) // 100), name
        assert A.keep_loop(read[:70], a, O, E) == 70, name                   # nothing in front of the occurrence
        info = _same_as_models([read], a, O, E, name)
        if n_err <= (k * E) // 100:
            assert A.keep_loop(read, a, O, E) <= 70 and info["n_changed"] == 1, name
            hit += 1
        else:
            assert A.keep_loop(read, a, O, E) != 70, name
    assert hit == len(cases) // 2


def test_lime_adapter_trim_on_seeded_collections():
    emptied = cut = reads_seen = 0
    for case in range(A.FUZZ_CASES):
        reads, adapter, O, E = A.fuzz_collection(A.SEED, case)
        info = _same_as_models(reads, adapter, O, E, f"fuzz_collection({A.SEED}, {case})")
        emptied += info["n_empty"]; cut += info["n_changed"]; reads_seen += info["n_reads"]
    print("reads", reads_seen, "cut", cut, "emptied", emptied)
    assert A.FUZZ_CASES == 400 and cut > 2000 and emptied > 20 and cut < reads_seen


def test_every_adapter_length_and_every_overlap_at_the_reads_end():
    rng = np.random.default_rng([A.SEED, 4])
    for M in A.ADAPTER_LENGTHS:
        a = A.bases(rng, M)
        for O in sorted({1, min(2, M), max(1, M - 1), M}):
            reads = [A.bases(rng, 90) + a[:k] for k in sorted({1, O - 1, O, M - 1, M} - {0})] + [a, a[:max(1, O - 1)], b""]
            _same_as_models(reads, a, O, 0, (M, O))
            _same_as_models(reads, a, O, 10, (M, O))


def test_refusals():
    from lime_amd import _lib, api
    reads = [b"ACGTACGT"]
    bad = [(b"", 1, 10, "1 .. 64"), (b"A" * 65, 3, 10, "1 .. 64"), (b"ACGN", 3, 10, "A, C, G and T"), (b"AC-T", 3, 10, "A, C, G and T"),
           (b"AC\xc1T", 3, 10, "A, C, G and T"), (b"ACGT", 0, 10, "overlap"), (b"ACGT", 5, 10, "overlap"), (b"ACGT", 3, 51, "0 .. 50")]
    for adapter, O, E, word in bad:
        with pytest.raises(api.LimeError) as e:
            _host_trim(reads, adapter, O, E)
        assert e.value.code == _lib.ERR_ARG and word in str(e.value) and str(e.value).count("lime_adapter_trim:") == 1, (adapter, O, E, str(e.value))
    for adapter, O, E in ((b"A", 1, 0), (b"acgt", 4, 50), (b"A" * 64, 64, 50)):
        assert _host_trim(reads, adapter, O, E)[2]["n_reads"] == 1
    with pytest.raises(api.LimeError) as e:
        api.adapter_trim(np.zeros(4, np.uint8), np.array([0, 3, 2], np.uint64), b"ACGT", 3, 10)
    assert e.value.code == _lib.ERR_ARG and "decreases" in str(e.value)
    with pytest.raises(api.LimeError) as e:
        api.adapter_trim(np.zeros(4, np.uint8), np.array([1, 3, 4], np.uint64), b"ACGT", 3, 10)
    assert e.value.code == _lib.ERR_ARG and "start at 0" in str(e.value)
    lib = _lib.load()
    assert lib.lime_adapter_trim(None, None, 0, None, 4, 3, 10, None, None, None) == _lib.ERR_ARG
    pt, po, ti = C.c_void_p(1), C.c_void_p(1), _lib.TrimInfo(7, 7, 7, 7, 7)
    off = np.zeros(1, np.uint64)
    assert lib.lime_adapter_trim(None, off.ctypes.data, 0, None, 4, 3, 10, C.byref(pt), C.byref(po), C.byref(ti)) == _lib.ERR_ARG
    assert pt.value is None and po.value is None and ti.n_reads == 0         # a refusal leaves every output cleared
    assert lib.lime_seq_reader_set_adapter(None, b"ACGT", 4, 3, 10) == _lib.ERR_ARG and lib.lime_seq_reader_adapter_info(None, None) == _lib.ERR_ARG
    assert lib.lime_docs_trim_adapter_dev(None, None, b"ACGT", 4, 3, 10, None, None, None) == _lib.ERR_ARG


def test_no_reads_and_the_counts_of_an_unchanged_collection():
    text, off, info = _host_trim([], b"ACGT", 3, 10)
    assert len(text) == 0 and list(off) == [0] and info == {"n_reads": 0, "n_changed": 0, "n_empty": 0, "symbols_in": 0, "symbols_out": 0}
    reads = [b"TTTTTTTT", b"", b"GGGG"]
    text, off, info = _host_trim(reads, b"ACAC", 3, 0)
    assert np.array_equal(text, A.records(reads)[0]) and info == {"n_reads": 3, "n_changed": 0, "n_empty": 0, "symbols_in": 12, "symbols_out": 12}


def test_the_new_symbols_are_declared_and_exported():
    from lime_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    for n in ("lime_adapter_trim", "lime_docs_trim_adapter_dev", "lime_seq_reader_set_adapter", "lime_seq_reader_adapter_info"):
        assert n in _lib.SYMBOLS and hasattr(lib, n) and re.search(r"\b%s\(" % n, header), n


# ---- the program's usage errors: checked before a device is opened ----
def _lime_fasta(args):
    assert os.path.exists(os.path.join(BIN, "LiME_fasta"))
    return subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=120)


BASE = ["--gidx", "g.gidx", "--lineage", "l.csv"]


def test_trim_adapter_with_a_numeric_readlen_is_the_usage_error(tmp_path):
    out = str(tmp_path / "no.txt")
    p = _lime_fasta(["r.fastq"] + BASE + ["--readlen", "100", "--out", out, "--trim-adapter", A.TRUSEQ_R1.decode()])
    assert p.returncode == 1 and b"Error usage" in p.stderr and b"--trim-adapter" in p.stderr and not os.path.exists(out)


def test_a_second_adapter_with_one_reads_file_is_the_usage_error(tmp_path):
    out = str(tmp_path / "no.txt")
    p = _lime_fasta(["r.fastq"] + BASE + ["--readlen", "auto", "--out", out, "--trim-adapter", "ACGTACGT,TTGCA"])
    assert p.returncode == 1 and b"Error usage" in p.stderr and not os.path.exists(out)


@pytest.mark.parametrize("extra", [["--trim-adapter", ""], ["--trim-adapter", "A" * 65], ["--trim-adapter", "ACGN"], ["--trim-adapter", "ACGT,"],
                                   ["--trim-adapter", ",ACGT"], ["--trim-adapter", "ACGT,ACGT,ACGT"], ["--trim-adapter", "AC GT"], ["--trim-adapter"],
                                   ["--trim-adapter", "ACGT", "--adapter-overlap", "5"], ["--trim-adapter", "ACGTAC,ACGT", "--adapter-overlap", "5"],
                                   ["--trim-adapter", "ACGT", "--adapter-overlap", "0"], ["--trim-adapter", "ACGT", "--adapter-overlap", "x"],
                                   ["--trim-adapter", "ACGT", "--adapter-error", "51"], ["--trim-adapter", "ACGT", "--adapter-error", "-1"],
                                   ["--adapter-overlap", "3"], ["--adapter-error", "10"]])
def test_a_bad_adapter_option_is_the_usage_error(tmp_path, extra):
    out = str(tmp_path / "no.txt")
    p = _lime_fasta(["r_1.fastq", "r_2.fastq"] + BASE + ["--readlen", "auto", "--out", out] + extra)
    assert p.returncode == 1 and b"Error usage" in p.stderr and not os.path.exists(out)


def test_good_adapter_options_get_past_the_usage_check(tmp_path):
    """the same line with legal values ends later, at the reads file that is not there or at the missing device: not at the usage text"""
    out = str(tmp_path / "no.txt")
    for extra in (["--trim-adapter", "acgtACGT,ACGTA", "--adapter-overlap", "5", "--adapter-error", "50"], ["--trim-adapter", "A" * 64, "--adapter-error", "0"],
                  ["--trim-adapter", "ACGT", "--trim-qual", "20"]):
        p = _lime_fasta([str(tmp_path / "r_1.fastq"), str(tmp_path / "r_2.fastq")] + BASE + ["--readlen", "auto", "--out", out] + extra)
        assert p.returncode != 0 and b"Error usage" not in p.stderr and not os.path.exists(out)
