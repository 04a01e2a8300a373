"""The index builder's host side (include/lime_hip.h: lime_fasta_read, lime_index_size, the argument checks of lime_build_index that
need no device, bin/BuildIndex's usage).  No GPU here; the sort itself is tests/test_index_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lime_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_INDEX = os.path.join(ROOT, "lime_amd", "bin", "BuildIndex")

PAIRS = "ATCGRYKMBVDH"
COMP = bytes.maketrans((PAIRS + PAIRS.lower() + "Uu").encode(), ("TAGCYRMKVBHD" + "TAGCYRMKVBHD".lower() + "Aa").encode())


def py_fasta(data, rc=False):
    """restatement of lime_fasta_read: '>' at a line's start opens a record; other lines' bytes without CR / LF are its symbols"""
    docs = None
    for line in data.split(b"\n"):
        if line.startswith(b">"):
            docs = (docs or []) + [b""]
        elif docs:
            docs[-1] += line.replace(b"\r", b"")
    docs = docs or []
    return [d.translate(COMP)[::-1] for d in docs] if rc else docs


FASTA_CASES = {
    "multi_line": b">r1 first\nACGT\nTTGA\nC\n>r2\nGGGG\n",
    "crlf": b">r1\r\nACGT\r\nTT\r\n>r2\r\nGA\r\n",
    "empty_records": b">e1\n>e2\n\n>r\nAC\n>e3\n",
    "no_final_newline": b">r1\nACGT\n>r2\nTTG",
    "lower_case": b">r\nacgtNnacGT\n",
    "iupac": b">r\nACGTURYKMBVDHSWN-*acgturykmbvdhswn\n>s\nNNRY\n",
    "text_before_header": b"ACGT\n>r\nTT\n",
    "no_records": b"",
    "header_only": b">x",
}


@pytest.mark.parametrize("name", sorted(FASTA_CASES))
@pytest.mark.parametrize("rc", [False, True])
def test_fasta_read_matches_restatement(tmp_path, name, rc):
    data = FASTA_CASES[name]
    p = tmp_path / "in.fasta"
    p.write_bytes(data)
    got = api.fasta_read(str(p), rc=rc)
    assert got == py_fasta(data, rc)
    if name == "iupac" and rc:
        assert got[0] == b"nwsdhbvkmryaacgt*-NWSDHBVKMRYAACGT" and got[1] == b"RYNN"


def test_fasta_rc_is_the_example_generators_rc(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_example", os.path.join(ROOT, "tests", "golden", "make_golden_example.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    rng = np.random.default_rng(5)
    reads = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(n)).tobytes()) for n in rng.integers(0, 150, size=40)]
    p = tmp_path / "r.fasta"
    p.write_bytes(b"".join(b">%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    assert api.fasta_read(str(p)) == reads
    assert api.fasta_read(str(p), rc=True) == [mg.rc(r) for r in reads]


def test_fasta_read_errors(tmp_path):
    with pytest.raises(api.LimeError) as e:
        api.fasta_read(str(tmp_path / "missing.fasta"))
    assert e.value.code == _lib.ERR_IO
    lib = _lib.load()
    nd = C.c_uint32()
    assert lib.lime_fasta_read(None, 0, None, None, C.byref(nd)) == _lib.ERR_ARG


def test_index_size():
    assert api.index_size([0]) == 0
    assert api.index_size([0, 0, 0]) == 2                       # two empty documents: their terminators
    assert api.index_size([0, 100, 250, 250, 1000]) == 1004
    assert _lib.load().lime_index_size(None, 3) == 0
    text, off = api.pack_documents([b"ACG", "TT"], [b"", b"ACGTACGT"])
    assert text.tobytes() == b"ACGTTACGTACGT" and off.tolist() == [0, 3, 5, 5, 13] and api.index_size(off) == 17


def test_argument_errors_that_need_no_device():
    lib = _lib.load()
    off = np.array([0, 4], dtype=np.uint64)
    text = np.frombuffer(b"ACGT", np.uint8)
    out = np.zeros(8, np.uint32)
    assert lib.lime_build_index(None, text.ctypes.data, off.ctypes.data, 1, 0, 0, None, out.ctypes.data, None) == _lib.ERR_ARG
    assert b"ctx is NULL" in lib.lime_last_error()
    assert lib.lime_build_index_dev(None, None, None, 1, 4, 0, 0, None, None, None, None) == _lib.ERR_ARG
    assert b"ctx is NULL" in lib.lime_last_error()
    v = (C.c_double * 8)()
    assert lib.lime_get_index_info(None, v) == _lib.ERR_ARG


def test_new_symbols_are_exported():
    lib = _lib.load()
    for name in ("lime_index_size", "lime_build_index", "lime_build_index_dev", "lime_get_index_info", "lime_fasta_read"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    for name in ("build_index", "build_index_dev", "fasta_read"):
        assert callable(getattr(api, name))
    assert callable(api.Context.build_index) and callable(api.Context.build_index_dev)


def _ensure_program():
    if not os.path.exists(BUILD_INDEX):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    assert os.path.exists(BUILD_INDEX)


@pytest.mark.parametrize("args", [[], ["reads.fasta"], ["a", "b"], ["a", "b", "c", "d"], ["a", "b", "c", "--trlcp"], ["a", "b", "c", "--trlcp", "x"]])
def test_buildindex_usage(args):
    _ensure_program()
    r = subprocess.run([BUILD_INDEX] + args, capture_output=True, timeout=60)
    assert r.returncode == 1
    assert b"usage" in r.stderr and b"reads.fasta refs.fasta outBase [--rc] [--trlcp k]" in r.stderr


def test_buildindex_missing_input_is_an_io_error(tmp_path):
    _ensure_program()
    r = subprocess.run([BUILD_INDEX, str(tmp_path / "no_reads.fasta"), str(tmp_path / "no_refs.fasta"), str(tmp_path / "out")],
                       capture_output=True, timeout=60)
    assert r.returncode == -_lib.ERR_IO and b"Error reading" in r.stderr
    assert not os.path.exists(str(tmp_path / "out.lcp"))
