"""Without a GPU: the two models of tests/fastq_cases.py (the rule per byte, and a plain reader over split(b"\\n")) against lime_fastq_read,
rc 0 and 1, on every case and on the seeded inputs: valid inputs by text and doc_off, refused ones by code, line and reason.  The FASTQ
path's symbols exist; lime_seq_format; BuildIndex's reading of a FASTQ reads file; api.fastq_read."""
import ctypes as C
import collections
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fasta_cases as FC
from tests import fastq_cases as QC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lime_amd", "bin")


_host = QC.host_read


def _same(a, b, what):
    assert QC.is_refusal(a) == QC.is_refusal(b), (what, a, b)
    if QC.is_refusal(a):
        assert tuple(a) == tuple(b), (what, a, b)
    else:
        assert np.array_equal(a[1], b[1]), (what, a[1][:8], b[1][:8])
        assert np.array_equal(a[0], b[0]), what


def _check(tmp_path, name, data):
    want = QC.model_parse(data)
    _same(QC.split_parse(data), want, name + " (the two models)")
    _same(_host(tmp_path, data, 0), want, name)
    r = _host(tmp_path, data, 1)
    _same(r, want if QC.is_refusal(want) else (FC.model_revcomp(*want), want[1]), name + " (rc)")
    return want


def test_models_match_lime_fastq_read_on_every_case(tmp_path):
    from lime_amd import api
    seen = collections.Counter()
    for name, data in QC.cases(api.FASTA_BLOCK).items():
        want = _check(tmp_path, name, data)
        seen["valid" if not QC.is_refusal(want) else want[1]] += 1
        if name.startswith("reason "):
            assert QC.is_refusal(want) and want[1] == int(name.split()[1]), (name, want)
    assert all(seen[k] >= 10 for k in ("valid", 0, 1, 2, 3)), seen


def test_models_match_lime_fastq_read_on_random_strings(tmp_path):
    from lime_amd import api
    for case in range(QC.FUZZ_CASES):
        _check(tmp_path, f"fuzz_bytes({QC.SEED}, {case})", QC.fuzz_bytes(QC.SEED, case, api.FASTA_BLOCK))
    assert QC.FUZZ_CASES == 400


def test_models_match_lime_fastq_read_on_mutated_records(tmp_path):
    from lime_amd import api
    seen = collections.Counter()
    for case in range(QC.FUZZ_CASES):
        want = _check(tmp_path, f"fuzz_mutated({QC.SEED}, {case})", QC.fuzz_mutated(QC.SEED, case, api.FASTA_BLOCK))
        seen["valid" if not QC.is_refusal(want) else want[1]] += 1
    assert QC.FUZZ_CASES == 400 and seen["valid"] >= 100 and all(seen[k] >= 5 for k in range(4)), seen


def test_the_reason_texts_are_the_headers():
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    for r in QC.REASONS:
        assert '"%s"' % r in header, r


def test_symbols_exist():
    from lime_amd import _lib, api
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    for n in ("lime_fastq_read", "lime_seq_format", "lime_docs_from_fastq", "lime_docs_from_fastq_bytes", "lime_docs_from_fastq_bytes_dev", "lime_docs_from_file"):
        assert n in _lib.SYMBOLS and hasattr(lib, n) and re.search(r"\b%s\(" % n, header), n
    for n in ("fastq_read", "seq_format"):
        assert hasattr(api, n), n
    for n in ("docs_from_fastq", "docs_from_fastq_bytes", "docs_from_fastq_bytes_dev", "docs_from_file"):
        assert hasattr(api.Context, n), n
    csrc = os.path.join(ROOT, "lime_amd", "csrc")
    shared, kernel = open(os.path.join(csrc, "lime_bytes.h")).read(), open(os.path.join(csrc, "lime_fastq_kernel.hip")).read()
    assert shared.count("static_assert(LIME_FASTA_BLOCK == BY_WG * BY_LANE") == 1 and len(re.findall(r"static_assert\(\s*LIME_FASTA_BLOCK", shared)) == 1
    assert '#include "lime_bytes.h"' in kernel and "LIME_FASTA_BLOCK ==" not in kernel
    assert not re.search(r"\b\w*(WG|LANE)\s*=[^=]", kernel)           # no workgroup size or bytes per lane of its own: lime_bytes.h's


def test_seq_format(tmp_path):
    from lime_amd import _lib, api
    for name, data, want in (("q", b"@r\nAC\n+\nII\n", "fastq"), ("a", b">r\nAC\n", "fasta"), ("empty", b"", "fasta"), ("other", b"AC\n>r\nAC\n", "fasta"),
                             ("at", b"@", "fastq"), ("lf", b"\n@r\n", "fasta")):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        assert api.seq_format(p) == want, name
    with pytest.raises(api.LimeError) as e:
        api.seq_format(str(tmp_path / "no_such_file"))
    assert e.value.code == _lib.ERR_IO
    f = C.c_int(5)
    assert _lib.load().lime_seq_format(os.fsencode(str(tmp_path / "no_such_file")), C.byref(f)) == _lib.ERR_IO


def test_api_fastq_read(tmp_path):
    from lime_amd import _lib, api
    data = QC.cases(api.FASTA_BLOCK)["CRLF throughout"] + QC.cases(api.FASTA_BLOCK)["empty reads"]
    p = str(tmp_path / "r.fastq")
    open(p, "wb").write(data)
    text, off = QC.split_parse(data)
    assert QC.records(api.fastq_read(p))[0].tobytes() == text.tobytes() and np.array_equal(QC.records(api.fastq_read(p))[1], off)
    assert np.array_equal(QC.records(api.fastq_read(p, rc=True))[0], FC.model_revcomp(text, off))
    open(p, "wb").write(data + b"@r\nACGT\n+\nIII\n" + data)
    with pytest.raises(api.LimeError) as e:
        api.fastq_read(p)
    assert e.value.code == _lib.ERR_ARG and QC.refusal_of(str(e.value)) == QC.split_parse(data + b"@r\nACGT\n+\nIII\n")
    with pytest.raises(api.LimeError) as e:
        api.fastq_read(str(tmp_path / "no_such_file"))
    assert e.value.code == _lib.ERR_IO


def test_buildindex_reads_fastq_on_the_host(tmp_path):
    """BuildIndex decides the reads file's format by lime_seq_format and reads FASTQ with lime_fastq_read, before any device work: a malformed
    file ends it with the file's name, the line and the reason; a well-formed one gets past the reading (what follows needs a device)"""
    exe = os.path.join(BIN, "BuildIndex")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    refs, good, bad = str(tmp_path / "refs.fasta"), str(tmp_path / "good.fastq"), str(tmp_path / "bad.fastq")
    open(refs, "wb").write(b">g\nACGTACGTTTGACCA\n")
    open(good, "wb").write(QC.rec(seq=b"ACGTAC") + QC.rec(seq=b"TTGACC", qual=b"@+I!II"))
    data = QC.rec() + b"@r\nACGT\n-\nIIII\n"
    open(bad, "wb").write(data)
    line, reason = QC.split_parse(data)
    for args in ([bad, refs, str(tmp_path / "out")], [bad, "--gidx", str(tmp_path / "no.gidx"), str(tmp_path / "out")]):
        p = subprocess.run([exe] + args, capture_output=True, timeout=120)
        err = p.stderr.decode()
        assert p.returncode == 1 and "Error reading " + bad in err, err
        assert QC.refusal_of(err.strip().splitlines()[-1]) == (line, reason) == (7, 1), err
        assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]
    p = subprocess.run([exe, good, refs, str(tmp_path / "out")], capture_output=True, timeout=600)
    assert b"Error reading" not in p.stderr, p.stderr
    p = subprocess.run([exe, str(tmp_path / "no_such.fastq"), refs, str(tmp_path / "out")], capture_output=True, timeout=120)
    assert p.returncode != 0 and b"Error reading" in p.stderr
