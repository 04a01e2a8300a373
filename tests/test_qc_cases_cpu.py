"""lime_read_qc (the host oracle of the per-position read statistics), lime_qc_report_write and LiME_fasta's usage errors for --qc-report,
against the two numpy models of tests/qc_cases.py.  No device is needed."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import qc_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lime_amd", "bin")


def _host(reads, quals, n_pos, tables=None):
    from lime_amd import api
    text, q, off = Q.flat(reads, quals)
    return api.read_qc(text, off, n_pos, qual=q, tables=tables)


def _same(got, want, n_pos, what):
    w = Q.split(want, n_pos)
    for k in Q.KEYS:
        assert got[k].shape == w[k].shape and np.array_equal(got[k], w[k]), (what, k, got[k], w[k])
    assert np.array_equal(got["tables"], want), what


HAND = Q.hand_cases()


@pytest.mark.parametrize("name", [c[0] for c in HAND])
def test_lime_read_qc_on_the_hand_made_cases(name):
    _, reads, quals, n_pos, want = next(c for c in HAND if c[0] == name)
    assert np.array_equal(Q.qc_loop(reads, quals, n_pos), want), name            # the written-out tables are the models' ...
    assert np.array_equal(Q.qc_vector(reads, quals, n_pos), want), name
    _same(_host(reads, quals, n_pos), want, n_pos, name)                         # ... and the library's
    Q.invariants(want, n_pos, reads, quals is not None)


def test_the_hand_made_cases_at_every_n_pos():
    for name, reads, quals, _, _ in HAND:
        for n_pos in Q.N_POS:
            want = Q.model(reads, quals, n_pos)
            _same(_host(reads, quals, n_pos), want, n_pos, (name, n_pos))
            Q.invariants(want, n_pos, reads, quals is not None)


def test_the_thresholds():
    for name, reads, quals in Q.threshold_cases():
        for n_pos in Q.N_POS:
            want = Q.model(reads, quals, n_pos)
            _same(_host(reads, quals, n_pos), want, n_pos, (name, n_pos))
            Q.invariants(want, n_pos, reads, quals is not None)
    # what the cases are for, on the model: 52 / 53 and 62 / 63 fall on different sides, bytes below 33 are taken raw
    for q, (ge20, ge30) in ((52, (0, 0)), (53, (1, 0)), (62, (1, 0)), (63, (1, 1)), (0, (0, 0)), (32, (0, 0)), (255, (1, 1))):
        s = Q.split(Q.model([b"A"], [bytes([q])], 4), 4)
        assert (int(s["rows"][0, 5]), int(s["rows"][0, 6]), int(s["rows"][0, 7])) == (q, ge20, ge30) and int(s["mq_hist"][q]) == 1
    for gc, n, at in ((1, 3, 33), (2, 3, 66), (50, 100, 50), (99, 100, 99), (199, 200, 99), (1, 101, 0)):
        assert int(Q.split(Q.model([b"C" * gc + b"T" * (n - gc)], None, 8), 8)["gc_hist"][at]) == 1
    for n_pos in Q.N_POS:
        for L, at in ((n_pos - 1, n_pos - 1), (n_pos, n_pos), (n_pos + 1, n_pos)):
            s = Q.split(Q.model([b"A" * L], None, n_pos), n_pos)
            assert int(s["len_hist"][at]) == 1 and int(s["rows"][n_pos, 0]) == max(L - n_pos, 0)


def test_lime_read_qc_on_seeded_collections():
    """400 collections at each of the ten n_pos and at the generator's own, against both models (which are compared with each other)"""
    for case in range(Q.FUZZ_CASES):
        reads, quals, own = Q.fuzz_collection(Q.SEED, case)
        for n_pos in sorted(set(Q.N_POS) | {own}):
            want = Q.model(reads, quals, n_pos)
            _same(_host(reads, quals, n_pos), want, n_pos, (case, n_pos))
            Q.invariants(want, n_pos, reads, quals is not None)


def test_the_generator_mixes_what_it_says():
    y = Q.fuzz_yield()
    print(y)
    assert y["long"] >= 200 and y["no_base"] >= 50 and y["empty"] >= 50 and y["no_qual"] >= 50 and y["pool_in_word"] >= 100


def test_two_calls_equal_one_call_on_the_concatenation():
    for case in range(0, 40, 2):
        a, qa, n_pos = Q.fuzz_collection(Q.SEED, case)
        b, qb, _ = Q.fuzz_collection(Q.SEED, case + 1)
        if (qa is None) != (qb is None):
            qa = qb = None
        whole = _host(a + b, None if qa is None else qa + qb, n_pos)
        t = np.zeros(Q.words(n_pos), dtype=np.uint64)
        first = _host(a, qa, n_pos, tables=t)
        assert first["tables"] is t
        _host(b, qb, n_pos, tables=t)
        assert np.array_equal(t, whole["tables"]), case
    # a collection with qualities and one without sum too: the quality counters hold the first alone
    t = np.zeros(Q.words(3), dtype=np.uint64)
    _host([b"ACGTA"], [bytes([40] * 5)], 3, tables=t)
    _host([b"ACGTA"], None, 3, tables=t)
    assert np.array_equal(t, Q.model([b"ACGTA"], [bytes([40] * 5)], 3) + Q.model([b"ACGTA"], None, 3))


def test_refusals():
    from lime_amd import _lib, api
    text, off = np.frombuffer(b"ACGT", dtype=np.uint8), np.array([0, 4], np.uint64)
    for n_pos in (0, 513, 100000):
        t = np.zeros(Q.words(4), dtype=np.uint64)
        lib = _lib.load()
        assert lib.lime_read_qc(text.ctypes.data, None, off.ctypes.data, 1, n_pos, t.ctypes.data) == _lib.ERR_ARG
        msg = lib.lime_last_error().decode()
        assert "positions" in msg and "1 .. 512" in msg and msg.count("lime_read_qc:") == 1 and not t.any()
        with pytest.raises(ValueError):
            api.read_qc(text, off, n_pos)
    with pytest.raises(api.LimeError) as e:
        api.read_qc(np.zeros(4, np.uint8), np.array([0, 3, 2], np.uint64), 4)
    assert e.value.code == _lib.ERR_ARG and "decreases" in str(e.value)
    with pytest.raises(api.LimeError) as e:
        api.read_qc(np.zeros(4, np.uint8), np.array([1, 3, 4], np.uint64), 4)
    assert e.value.code == _lib.ERR_ARG and "start at 0" in str(e.value)
    lib = _lib.load()
    t = np.zeros(Q.words(4), dtype=np.uint64)
    assert lib.lime_read_qc(text.ctypes.data, None, None, 1, 4, t.ctypes.data) == _lib.ERR_ARG and "NULL array" in lib.lime_last_error().decode()
    assert lib.lime_read_qc(text.ctypes.data, None, off.ctypes.data, 1, 4, None) == _lib.ERR_ARG and "NULL array" in lib.lime_last_error().decode()
    assert lib.lime_read_qc(None, None, off.ctypes.data, 1, 4, t.ctypes.data) == _lib.ERR_ARG and "NULL array" in lib.lime_last_error().decode()
    assert not t.any()
    zero = np.zeros(1, np.uint64)
    assert lib.lime_read_qc(None, None, zero.ctypes.data, 0, 4, t.ctypes.data) == 0 and not t.any()          # no read: legal, nothing added
    assert lib.lime_docs_qc_dev(None, None, 4, None, None) == _lib.ERR_ARG
    assert lib.lime_seq_reader_set_qc(None, 4) == _lib.ERR_ARG and lib.lime_seq_reader_qc(None, 0, None) == _lib.ERR_ARG


def test_the_new_symbols_are_declared_and_exported():
    from lime_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    for n in ("lime_read_qc", "lime_docs_qc_dev", "lime_seq_reader_set_qc", "lime_seq_reader_qc", "lime_qc_report_write"):
        assert n in _lib.SYMBOLS and hasattr(lib, n) and re.search(r"\b%s\(" % n, header), n
    assert "LIME_QC_MAX_POS 512u" in header and _lib.QC_MAX_POS == 512
    from lime_amd import api
    assert [api.qc_words(p) for p in (1, 256, 512)] == [Q.words(p) for p in (1, 256, 512)] == [375, 2670, 4974]


# ---- the report ----
def _report_case():
    a, qa, _ = Q.fuzz_collection(Q.SEED, 1)
    b, _, _ = Q.fuzz_collection(Q.SEED, 2)
    n_pos = 65
    before = [Q.model(a, qa, n_pos), Q.model(b, None, n_pos)]
    after = [Q.model([r[:40] for r in a], None, n_pos), Q.model(b, None, n_pos)]
    return ["reads \"one\"\\.fastq", "two.fasta"], ["fastq", "fasta"], n_pos, before, after


def test_the_report_is_the_models_dictionary(tmp_path):
    from lime_amd import api
    names, formats, n_pos, before, after = _report_case()
    assert before[0][:8 * (n_pos + 1)].reshape(-1, 8)[:, 5].any()
    path = str(tmp_path / "qc.json")
    api.qc_report_write(path, names, formats, n_pos, before, after)
    got = json.load(open(path), object_pairs_hook=Q.key_order)
    want = Q.report(names, formats, n_pos, before, after)
    assert got == want
    assert os.listdir(str(tmp_path)) == ["qc.json"]
    # keys in the stated order, FASTA sections and every `after` without quality keys
    base = ["reads", "empty", "symbols", "gc", "bases", "length_hist", "gc_hist"]
    qual = ["q20", "q30", "qual_sum", "qual_ge20", "qual_ge30", "mean_qual_hist"]
    assert list(got) == ["lime_qc_report", "positions", "files"] and got["lime_qc_report"] == 1 and got["positions"] == n_pos
    for f, fmt in zip(got["files"], formats):
        assert list(f) == ["file", "format", "before", "after"]
        assert list(f["before"]) == base + (qual if fmt == "fastq" else []) and list(f["after"]) == base
        assert list(f["before"]["bases"]) == ["A", "C", "G", "T", "other"]
        for sec in (f["before"], f["after"]):
            assert all(len(v) == n_pos + 1 for v in sec["bases"].values()) and len(sec["length_hist"]) == n_pos + 1 and len(sec["gc_hist"]) == 101
    assert len(got["files"][0]["before"]["mean_qual_hist"]) == 256
    # integers only
    def no_float(x):
        raise AssertionError("a number that is no integer: " + x)
    json.load(open(path), parse_float=no_float, parse_constant=no_float)
    # the dictionaries that read_qc gives are taken as well, and the tables of a stage that changes nothing give after = before's base part
    api.qc_report_write(path, names[1:], formats[1:], n_pos, [Q.split(before[1], n_pos) | {"tables": before[1]}], [after[1]])
    one = json.load(open(path))
    assert one["files"][0]["after"] == one["files"][0]["before"] == want["files"][1]["before"]


def test_a_failing_write_leaves_no_file(tmp_path):
    from lime_amd import _lib, api
    names, formats, n_pos, before, after = _report_case()
    gone = tmp_path / "not_there"
    with pytest.raises(api.LimeError) as e:
        api.qc_report_write(str(gone / "qc.json"), names, formats, n_pos, before, after)
    assert e.value.code == _lib.ERR_IO and "cannot write" in str(e.value) and not gone.exists() and os.listdir(str(tmp_path)) == []
    # the rename fails where the name is a directory: the temporary file goes too
    (tmp_path / "qc.json").mkdir()
    with pytest.raises(api.LimeError) as e:
        api.qc_report_write(str(tmp_path / "qc.json"), names, formats, n_pos, before, after)
    assert e.value.code == _lib.ERR_IO and os.listdir(str(tmp_path)) == ["qc.json"] and os.listdir(str(tmp_path / "qc.json")) == []
    lib = _lib.load()
    for n_pos_bad in (0, 513):
        with pytest.raises(api.LimeError) as e:
            api.qc_report_write(str(tmp_path / "x.json"), names, formats, n_pos_bad, [np.zeros(Q.words(n_pos_bad), np.uint64)] * 2, [np.zeros(Q.words(n_pos_bad), np.uint64)] * 2)
        assert e.value.code == _lib.ERR_ARG and "positions" in str(e.value)
    with pytest.raises(api.LimeError) as e:
        api.qc_report_write(str(tmp_path / "x.json"), names, [0, 2], n_pos, before, after)
    assert e.value.code == _lib.ERR_ARG and "format" in str(e.value)
    assert lib.lime_qc_report_write(None, 1, None, None, 4, None, None) == _lib.ERR_ARG and "NULL" in lib.lime_last_error().decode()
    with pytest.raises(api.LimeError) as e:
        api.qc_report_write(str(tmp_path / "x.json"), [], [], n_pos, [], [])
    assert e.value.code == _lib.ERR_ARG and "no file" in str(e.value)
    assert not os.path.exists(str(tmp_path / "x.json"))


# ---- the program's usage errors: checked before a device is opened ----
def _lime_fasta(args):
    assert os.path.exists(os.path.join(BIN, "LiME_fasta"))
    return subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=120)


BASE = ["--gidx", "g.gidx", "--lineage", "l.csv", "--readlen", "100"]


@pytest.mark.parametrize("extra", [["--qc-positions", "64"], ["--qc-report", "q.json", "--qc-positions", "0"], ["--qc-report", "q.json", "--qc-positions", "513"],
                                   ["--qc-report", "q.json", "--qc-positions", "x"], ["--qc-report", "q.json", "--qc-positions", "-1"],
                                   ["--qc-report", "q.json", "--qc-positions"], ["--qc-report"]])
def test_a_bad_qc_option_is_the_usage_error(tmp_path, extra):
    out = str(tmp_path / "no.txt")
    extra = [str(tmp_path / x) if x == "q.json" else x for x in extra]
    p = _lime_fasta(["r_1.fastq", "r_2.fastq"] + BASE + ["--out", out] + extra)
    assert p.returncode == 1 and b"Error usage" in p.stderr and b"--qc-report" in p.stderr and os.listdir(str(tmp_path)) == []


def test_good_qc_options_get_past_the_usage_check(tmp_path):
    """the same line with legal values ends later, at the reads file that is not there: not at the usage text"""
    out = str(tmp_path / "no.txt")
    for extra in (["--qc-report", str(tmp_path / "q.json")], ["--qc-report", str(tmp_path / "q.json"), "--qc-positions", "1"],
                  ["--qc-positions", "512", "--qc-report", str(tmp_path / "q.json"), "--batch-reads", "5"]):
        p = _lime_fasta([str(tmp_path / "r_1.fastq"), str(tmp_path / "r_2.fastq")] + BASE + ["--out", out] + extra)
        assert p.returncode != 0 and b"Error usage" not in p.stderr and os.listdir(str(tmp_path)) == []


def test_the_python_mirror_refuses_the_same():
    from lime_amd import api
    for kw in (dict(qc_positions=64), dict(qc_report="q.json", qc_positions=0), dict(qc_report="q.json", qc_positions=513)):
        with pytest.raises(ValueError):
            api.lime_fasta(["r.fastq"], "l.csv", 100, "o.txt", gidx="g.gidx", **kw)
