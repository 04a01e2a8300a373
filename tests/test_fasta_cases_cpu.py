"""Without a GPU: the numpy models of tests/fasta_cases.py (what tests/test_fasta_edges_gpu.py holds the kernels against) give what
lime_fasta_read gives, rc 0 and 1, on every case and on the seeded strings; the device FASTA path's symbols, program and constant exist."""
import os
import re
import subprocess

import numpy as np

from tests import fasta_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(tmp_path, data, rc):
    from lime_amd import api
    p = str(tmp_path / "in.fasta")
    with open(p, "wb") as f:
        f.write(data)
    return FC.records(api.fasta_read(p, rc=rc))


def _check(tmp_path, name, data):
    text, off = FC.model_parse(data)
    h_text, h_off = _host(tmp_path, data, False)
    assert np.array_equal(off, h_off), (name, off[:8], h_off[:8])
    assert np.array_equal(text, h_text), name
    r_text, r_off = _host(tmp_path, data, True)
    assert np.array_equal(r_off, off) and np.array_equal(FC.model_revcomp(text, off), r_text), name


def test_models_match_lime_fasta_read_on_every_case(tmp_path):
    from lime_amd import api
    for name, data in FC.cases(api.FASTA_BLOCK).items():
        _check(tmp_path, name, data)


def test_models_match_lime_fasta_read_on_seeded_strings(tmp_path):
    from lime_amd import api
    with_docs = 0
    for case in range(FC.FUZZ_CASES):
        data = FC.fuzz_bytes(FC.SEED, case, api.FASTA_BLOCK)
        _check(tmp_path, f"fuzz_bytes({FC.SEED}, {case})", data)
        with_docs += len(FC.model_parse(data)[1]) > 2
    assert FC.FUZZ_CASES == 200 and with_docs > 100


def test_revcomp_model_on_the_collections():
    """the model against a plain per-document loop (lime_fasta_read cannot hold 0x0A / 0x0D as symbols)"""
    for name, docs in FC.revcomp_collections(4096).items():
        text, off = FC.records(docs)
        want = b"".join(bytes(FC.COMP[np.frombuffer(d, np.uint8)][::-1].tobytes()) for d in docs)
        assert FC.model_revcomp(text, off).tobytes() == want, name


def test_symbols_exist():
    from lime_amd import _lib, api
    lib = _lib.load()
    names = ["lime_docs_from_fasta", "lime_docs_from_bytes", "lime_docs_from_bytes_dev", "lime_docs_from_arrays_dev", "lime_docs_revcomp",
             "lime_docs_info", "lime_docs_device", "lime_docs_get", "lime_docs_free", "lime_classify_sample_dev"]
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    for n in names:
        assert n in _lib.SYMBOLS and hasattr(lib, n) and re.search(r"\b%s\(" % n, header), n
    for n in ("Docs", "lime_fasta", "FASTA_BLOCK"):
        assert hasattr(api, n), n
    for n in ("docs_from_fasta", "docs_from_bytes", "docs_from_bytes_dev", "docs_from_arrays_dev", "classify_sample"):
        assert hasattr(api.Context, n), n
    for n in ("info", "get", "revcomp", "close"):
        assert hasattr(api.Docs, n), n


def test_lime_fasta_usage():
    exe = os.path.join(ROOT, "lime_amd", "bin", "LiME_fasta")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    for args in ([], ["reads.fasta"], ["a", "b", "c", "--refs", "r", "--lineage", "l", "--readlen", "100", "--out", "o"],
                 ["a", "--refs", "r", "--gidx", "g", "--lineage", "l", "--readlen", "100", "--out", "o"], ["a", "--refs", "r", "--lineage", "l", "--out", "o"]):
        p = subprocess.run([exe] + args, capture_output=True, timeout=60)
        assert p.returncode == 1 and b"Error usage" in p.stderr, args


def test_fasta_block_is_the_headers():
    from lime_amd import api
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    m = re.search(r"#define\s+LIME_FASTA_BLOCK\s+(\d+)u", header)
    assert m and int(m.group(1)) == api.FASTA_BLOCK
    csrc = os.path.join(ROOT, "lime_amd", "csrc")
    shared, kernel = open(os.path.join(csrc, "lime_bytes.h")).read(), open(os.path.join(csrc, "lime_fasta_kernel.hip")).read()
    assert shared.count("static_assert(LIME_FASTA_BLOCK == BY_WG * BY_LANE") == 1 and len(re.findall(r"static_assert\(\s*LIME_FASTA_BLOCK", shared)) == 1
    assert '#include "lime_bytes.h"' in kernel and "LIME_FASTA_BLOCK ==" not in kernel
    assert not re.search(r"\b\w*(WG|LANE)\s*=[^=]", kernel)           # no workgroup size or bytes per lane of its own: lime_bytes.h's
