"""Without a GPU: the two models of tests/trim_cases.py against each other; lime_quality_trim (the loop form in the library's host code)
against them on every hand-made pattern and on 400 seeded collections; lime_fastq_read_qual against lime_fastq_read and a line-splitting model
of the qualities on every input of tests/fastq_cases.py; the cutoffs' limits; LiME_fasta's usage errors that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fastq_cases as QC
from tests import trim_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lime_amd", "bin")


def _host_trim(reads, quals, q5, q3):
    from lime_amd import api
    text, off = T.records(reads)
    qual, _ = T.records(quals)
    return api.quality_trim(text, qual, off, q5, q3)


def _same_as_model(reads, quals, q5, q3, what):
    want, info = T.trim_model(reads, quals, q5, q3)
    w_text, w_off = T.records(want)
    text, off, got = _host_trim(reads, quals, q5, q3)
    assert np.array_equal(off, w_off) and np.array_equal(text, w_text), (what, q5, q3)
    assert got == info, (what, got, info)


def test_the_two_forms_of_the_rule_agree_on_seeded_reads():
    n = 0
    for case in range(T.FUZZ_CASES):
        _, quals, q5, q3 = T.fuzz_collection(T.SEED, case)
        for b in quals:
            assert T.bounds_loop(b, q5, q3) == T.bounds_closed(b, q5, q3), (case, b, q5, q3)
            n += 1
    rng = np.random.default_rng([T.SEED, 5])
    for _ in range(3000):                                                   # short reads over tie-heavy alphabets, every cutoff pair of three
        b = np.array([T.Q(19), T.Q(20), T.Q(21)], np.uint8)[rng.integers(0, 3, size=int(rng.integers(0, 12)))].tobytes()
        for q5 in (0, 20, 21):
            for q3 in (0, 19, 20):
                assert T.bounds_loop(b, q5, q3) == T.bounds_closed(b, q5, q3), (b, q5, q3)
    assert n > 5000 and T.FUZZ_CASES == 400


@pytest.mark.parametrize("L", T.LENGTHS)
def test_lime_quality_trim_on_the_hand_made_patterns(L):
    rng = np.random.default_rng([T.SEED, 6, L])
    for cut in (1, 20):
        pats = T.patterns(L, cut)
        names = sorted(pats)
        quals = [pats[k] for k in names]
        reads = [T.bases(rng, L) for _ in names]
        for q5, q3 in ((cut, cut), (0, cut), (cut, 0), (0, 0), (93, 93), (1, 93), (93, 20)):
            for k, b in zip(names, quals):
                assert T.bounds_loop(b, q5, q3) == T.bounds_closed(b, q5, q3), (L, k, q5, q3)
            _same_as_model(reads, quals, q5, q3, f"patterns of {L}")


def test_lime_quality_trim_what_the_patterns_are_for():
    """the expectations written out, so that a mistake shared by both models would show"""
    p = T.patterns(600, 20)
    B = T.bounds_loop
    assert B(p["all above"], 20, 20) == (0, 600) and B(p["all equal: sums of 0 cut nothing"], 20, 20) == (0, 600)
    assert B(p["all below: both cuts take everything and cross"], 20, 20) == (600, 0)
    assert B(p["low tail of 17"], 20, 20) == (0, 583) and B(p["low head of 65 (5')"], 20, 20) == (65, 600)
    assert B(p["two equal minima"], 0, 20) == (0, 599) and B(p["two equal minima (5')"], 20, 0) == (1, 600)      # the larger index at 3', the smaller at 5'
    assert B(p["early stop on value 1"], 0, 20) == (0, 600)
    for d in (2, 16, 17, 256, 257, 513):
        assert B(p[f"early stop on value {d}"], 0, 20) == (0, 599) and B(p[f"early stop on value {d} (5')"], 20, 0) == (1, 600)
    assert B(p["a cut of 257"], 0, 20) == (0, 343) and B(p["a cut of 257 (5')"], 20, 0) == (257, 600)
    assert B(p["bytes 33"], 93, 93) == (600, 0) and B(p["bytes 126"], 93, 93) == (0, 600)
    low = bytes([20]) * 50                                                  # bytes below 33: negative qualities; a cutoff of 0 still leaves the end alone
    assert B(low, 0, 0) == (0, 50) and B(low, 0, 1) == (0, 0) and B(low, 1, 0) == (50, 50)


def test_lime_quality_trim_on_seeded_collections():
    emptied = cut = 0
    for case in range(T.FUZZ_CASES):
        reads, quals, q5, q3 = T.fuzz_collection(T.SEED, case)
        _same_as_model(reads, quals, q5, q3, f"fuzz_collection({T.SEED}, {case})")
        info = T.trim_model(reads, quals, q5, q3)[1]
        emptied += info["n_empty"]; cut += info["n_changed"]
    assert T.FUZZ_CASES == 400 and emptied > 100 and cut > 1000


def test_a_cutoff_of_0_leaves_an_end_alone_also_with_bytes_below_33():
    reads, quals = [b"ACGTACGTAC", b"", b"TTT"], [bytes([0, 5, 10, 32, 33, 1, 2, 3, 4, 0]), b"", bytes([0, 0, 0])]
    text, off, info = _host_trim(reads, quals, 0, 0)
    assert np.array_equal(text, T.records(reads)[0]) and np.array_equal(off, T.records(reads)[1])
    assert info == {"n_reads": 3, "n_changed": 0, "n_empty": 0, "symbols_in": 13, "symbols_out": 13}
    _same_as_model(reads, quals, 0, 1, "3' only")
    _same_as_model(reads, quals, 1, 0, "5' only")
    assert _host_trim(reads, quals, 0, 1)[2]["n_empty"] == 2                 # (the empty read was empty before: not emptied)


def test_cutoffs_above_93_and_bad_arrays_are_refused():
    from lime_amd import _lib, api
    reads, quals = [b"ACGT"], [b"IIII"]
    for q5, q3 in ((94, 0), (0, 94), (1000, 1000)):
        with pytest.raises(api.LimeError) as e:
            _host_trim(reads, quals, q5, q3)
        assert e.value.code == _lib.ERR_ARG and "0 .. 93" in str(e.value)
    assert _host_trim(reads, quals, 93, 93)[2]["n_reads"] == 1
    with pytest.raises(api.LimeError) as e:
        api.quality_trim(np.zeros(4, np.uint8), np.zeros(4, np.uint8), np.array([0, 3, 2], np.uint64), 1, 1)
    assert e.value.code == _lib.ERR_ARG and "decreases" in str(e.value)
    lib = _lib.load()
    assert lib.lime_quality_trim(None, None, None, 0, 1, 1, None, None, None) == _lib.ERR_ARG


# ---- lime_fastq_read_qual ----
def _split_quals(data):
    """the quality lines of a valid file, CR dropped, back to back"""
    lines = bytes(data).split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return np.frombuffer(b"".join(l.replace(b"\r", b"") for l in lines[3::4]), dtype=np.uint8)


def _read_qual(tmp_path, data):
    """lime_fastq_read_qual on a file of `data` -> (text, qual, doc_off), or (line, reason) of a LIME_ERR_ARG refusal that left every output NULL"""
    from lime_amd import _lib
    lib = _lib.load()
    p = str(tmp_path / "in.fastq")
    open(p, "wb").write(data)
    pt, pq, po, nd = C.c_void_p(1), C.c_void_p(1), C.c_void_p(1), C.c_uint32(7)
    code = lib.lime_fastq_read_qual(os.fsencode(p), C.byref(pt), C.byref(pq), C.byref(po), C.byref(nd))
    if code != 0:
        msg = lib.lime_last_error().decode()
        assert code == _lib.ERR_ARG and pt.value is None and pq.value is None and po.value is None and nd.value == 0
        assert msg.startswith("lime_fastq_read_qual: line "), msg
        return QC.refusal_of(msg)
    lib.lime_free(pt); lib.lime_free(pq); lib.lime_free(po)
    from lime_amd import api
    return api.fastq_read_qual(p)


def _check_read_qual(tmp_path, data, what):
    want = QC.host_read(tmp_path, data)
    got = _read_qual(tmp_path, data)
    assert QC.is_refusal(got) == QC.is_refusal(want), (what, got, want)
    if QC.is_refusal(want):
        assert tuple(got) == tuple(want), (what, got, want)                 # today's line and reason
        return 0
    text, qual, off = got
    assert np.array_equal(text, want[0]) and np.array_equal(off, want[1]), what
    assert np.array_equal(qual, _split_quals(data)) and len(qual) == len(text), what
    return 1


def test_lime_fastq_read_qual_on_every_case(tmp_path):
    cases = QC.cases(4096)
    valid = sum(_check_read_qual(tmp_path, data, name) for name, data in cases.items())
    assert 20 <= valid < len(cases)


def test_lime_fastq_read_qual_on_seeded_inputs(tmp_path):
    valid = 0
    for case in range(QC.FUZZ_CASES):
        valid += _check_read_qual(tmp_path, QC.fuzz_mutated(QC.SEED, case, 4096), f"fuzz_mutated({QC.SEED}, {case})")
        _check_read_qual(tmp_path, QC.fuzz_bytes(QC.SEED, case, 4096), f"fuzz_bytes({QC.SEED}, {case})")
    assert 100 <= valid <= 300


def test_the_new_symbols_are_declared_and_exported():
    from lime_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    for n in ("lime_fastq_read_qual", "lime_quality_trim", "lime_docs_from_fastq_qual", "lime_docs_from_fastq_qual_bytes", "lime_docs_from_fastq_qual_bytes_dev",
              "lime_docs_qual_device", "lime_docs_get_qual", "lime_docs_trim_dev", "lime_seq_reader_set_trim", "lime_seq_reader_trim_info"):
        assert n in _lib.SYMBOLS and hasattr(lib, n) and re.search(r"\b%s\(" % n, header), n
    assert C.sizeof(_lib.TrimInfo) == 40


# ---- the program's usage errors: checked before a device is opened ----
def _lime_fasta(args):
    assert os.path.exists(os.path.join(BIN, "LiME_fasta"))
    return subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=120)


def test_trim_qual_with_a_numeric_readlen_is_the_usage_error(tmp_path):
    out = str(tmp_path / "no.txt")
    p = _lime_fasta(["r.fastq", "--gidx", "g.gidx", "--lineage", "l.csv", "--readlen", "100", "--out", out, "--trim-qual", "20"])
    assert p.returncode == 1 and b"Error usage" in p.stderr and b"--trim-qual" in p.stderr and not os.path.exists(out)


@pytest.mark.parametrize("word", ["", "x", "20,", ",20", "20,20,20", "94", "20,94", "-1", "2 0", "20;20", "1e1", "020,1"])
def test_a_malformed_cutoff_is_the_usage_error(tmp_path, word):
    out = str(tmp_path / "no.txt")
    p = _lime_fasta(["r.fastq", "--gidx", "g.gidx", "--lineage", "l.csv", "--readlen", "auto", "--out", out, "--trim-qual", word])
    assert p.returncode == 1 and b"Error usage" in p.stderr and not os.path.exists(out)


def test_a_fasta_reads_file_with_trim_qual_is_named_before_a_device_is_opened(tmp_path):
    fa, out = str(tmp_path / "reads.fasta"), str(tmp_path / "no.txt")
    open(fa, "wb").write(b">r\nACGT\n")
    p = _lime_fasta([fa, "--gidx", "g.gidx", "--lineage", "l.csv", "--readlen", "auto", "--out", out, "--trim-qual", "5,20"])
    assert p.returncode == 1 and fa.encode() in p.stderr and b"FASTQ" in p.stderr and not os.path.exists(out)
    assert os.listdir(str(tmp_path)) == ["reads.fasta"]
