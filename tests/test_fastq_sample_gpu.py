"""One sample from FASTQ bytes to verdicts on the device: the example at full size (tests/golden/example_full.npz) written as four-line FASTQ.
The classification file of bin/LiME_fasta, api.lime_fasta and Context.classify_sample must be the reference's own Classify output for these
collections, byte for byte (the golden tests/test_fasta_sample_gpu.py uses) -- both mates FASTQ, and FASTQ with FASTA; a malformed mate
ends the program with the file's name and the line; BuildIndex gives the same three files from reads.fastq as from reads.fasta."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fastq_cases as QC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lime_amd", "bin")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

ALPHA, READ_LEN, BETA = 16, 100, 0.25
NORM = READ_LEN + 1 - ALPHA


@functools.lru_cache(maxsize=None)
def _example():
    import make_golden_example as G
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_full.npz"))
    genomes, sets = G.collections(z["reads_1"], z["reads_2"], z["src"])
    return genomes, sets, bytes(z["lineage"]), bytes(z["classification"])


def _fasta(docs, width=None, eol=b"\n"):
    out = []
    for k, d in enumerate(docs):
        out.append(b">seq%d some text" % k + eol)
        out.extend(d[o:o + width] + eol for o in range(0, len(d), width)) if width else out.append(d + eol)
    return b"".join(out)


def _fastq(docs, eol=b"\n", odd_qualities=False):
    """four-line records; with odd_qualities every third record's quality string begins with '@' or '+'"""
    out = []
    for k, d in enumerate(docs):
        q = bytes(33 + (7 * k + j) % 41 for j in range(len(d)))
        if odd_qualities and k % 3 == 0 and q:
            q = (b"@" if k % 2 else b"+") + q[1:]
        out.append(b"@seq%d/1 some text" % k + eol + d + eol + (b"+" if k % 5 else b"+seq%d" % k) + eol + q + eol)
    return b"".join(out)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """reads_1 as FASTQ with LF, reads_2 as FASTQ with CRLF, both also as FASTA, the genomes in 60-column lines, the lineage, the genome index"""
    genomes, sets, lineage, _ = _example()
    d = str(tmp_path_factory.mktemp("sample_fastq"))
    f = {k: os.path.join(d, k) for k in ("reads_1.fastq", "reads_2.fastq", "reads_1.fasta", "reads_2.fasta", "refs.fasta", "LineageFile.csv", "g.gidx")}
    open(f["reads_1.fastq"], "wb").write(_fastq(sets["F1"], odd_qualities=True))
    open(f["reads_2.fastq"], "wb").write(_fastq(sets["F2"], eol=b"\r\n"))
    open(f["reads_1.fasta"], "wb").write(_fasta(sets["F1"]))
    open(f["reads_2.fasta"], "wb").write(_fasta(sets["F2"], eol=b"\r\n"))
    open(f["refs.fasta"], "wb").write(_fasta(genomes, width=60))
    open(f["LineageFile.csv"], "wb").write(lineage)
    for exe in ("LiME_fasta", "BuildIndex"):
        if not os.path.exists(os.path.join(BIN, exe)):
            subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    p = subprocess.run([os.path.join(BIN, "BuildIndex"), "--refs", f["refs.fasta"], os.path.join(d, "g")], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    f["dir"] = d
    return f


def test_the_files_are_what_the_test_means(files):
    from lime_amd import api
    _, sets, _, _ = _example()
    raw = open(files["reads_1.fastq"], "rb").read()
    lines = raw.split(b"\n")
    assert sum(1 for q in lines[3::4] if q[:1] in b"@+") >= len(sets["F1"]) // 3 and b"\r" not in raw
    assert open(files["reads_2.fastq"], "rb").read().count(b"\r\n") == 4 * len(sets["F2"])
    assert api.fastq_read(files["reads_1.fastq"]) == list(sets["F1"]) and api.fastq_read(files["reads_2.fastq"], rc=True) == list(sets["F2RC"])


@pytest.mark.parametrize("form", ["fastq fastq gidx", "fastq fastq refs", "fastq fasta gidx", "fasta fastq gidx"])
def test_lime_fasta_on_fastq_gives_the_references_classification(files, form):
    _, sets, _, want = _example()
    m1, m2, index = form.split()
    out = os.path.join(files["dir"], "classification_" + form.replace(" ", "_") + ".txt")
    args = [files["reads_1." + m1], files["reads_2." + m2], "--lineage", files["LineageFile.csv"], "--readlen", str(READ_LEN), "--out", out]
    args += ["--refs", files["refs.fasta"]] if index == "refs" else ["--gidx", files["g.gidx"]]
    before = set(os.listdir(files["dir"]))
    p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=600, cwd=files["dir"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert open(out, "rb").read() == want
    assert set(os.listdir(files["dir"])) - before == {os.path.basename(out)}           # nothing else is written
    assert b"numReads: %d\nnumGenomes: 3\n" % len(sets["F1"]) in p.stdout


def test_classify_sample_and_the_python_mirror(files, tmp_path):
    import torch
    from lime_amd import api
    genomes, sets, _, want = _example()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    try:
        mates = [ctx.docs_from_fastq(files["reads_1.fastq"]), ctx.docs_from_file(files["reads_2.fastq"])]
        for m, name in zip(mates, ("F1", "F2")):
            text, off = m.get()
            w_text, w_off = QC.records(list(sets[name]))
            assert np.array_equal(off, w_off) and np.array_equal(text, w_text), name
        gi = ctx.load_genome_index(files["g.gidx"])
        tx = api.Taxonomy(files["LineageFile.csv"], 1, False, len(genomes))
        v, counts, _ = ctx.classify_sample(mates, gi, tx, ALPHA, NORM, BETA)
        out = str(tmp_path / "classification.txt")
        api.write_classification(out, v)
        assert open(out, "rb").read() == want
        tx.close()
    finally:
        ctx.close()
    out2 = str(tmp_path / "classification_py.txt")
    counts2 = api.lime_fasta([files["reads_1.fastq"], files["reads_2.fasta"]], files["LineageFile.csv"], READ_LEN, out2, gidx=files["g.gidx"])
    assert open(out2, "rb").read() == want and counts2 == counts


def test_a_malformed_mate_ends_the_program(files):
    raw = open(files["reads_2.fastq"], "rb").read()
    lines = raw.split(b"\n")
    lines[4 * 1234 + 3] = lines[4 * 1234 + 3][:-2] + b"\r"                  # record 1234's quality string one short (the line keeps its CR)
    bad = os.path.join(files["dir"], "broken_2.fastq")
    open(bad, "wb").write(b"\n".join(lines))
    out = os.path.join(files["dir"], "no.txt")
    p = subprocess.run([os.path.join(BIN, "LiME_fasta"), files["reads_1.fastq"], bad, "--gidx", files["g.gidx"], "--lineage", files["LineageFile.csv"],
                        "--readlen", "100", "--out", out], capture_output=True, timeout=600)
    err = p.stderr.decode()
    assert p.returncode != 0 and "Error reading " + bad in err, err
    assert QC.refusal_of(err.strip().splitlines()[-1]) == (4 * 1234 + 4, 2), err
    assert not os.path.exists(out)


@pytest.mark.parametrize("rc", [[], ["--rc"]])
def test_buildindex_on_fastq_gives_the_fasta_forms_files(files, rc):
    got = {}
    for ext in ("fasta", "fastq"):
        base = os.path.join(files["dir"], "idx_" + ext + ("_rc" if rc else ""))
        p = subprocess.run([os.path.join(BIN, "BuildIndex"), files["reads_1." + ext], "--gidx", files["g.gidx"], base] + rc, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        got[ext] = [open(base + e, "rb").read() for e in (".ebwt", ".lcp", ".da")], p.stdout
        for e in (".ebwt", ".lcp", ".da"):
            os.remove(base + e)
    assert got["fasta"][0] == got["fastq"][0] and all(len(x) > 0 for x in got["fastq"][0])
    assert got["fasta"][1] == got["fastq"][1] and b"numReads: " in got["fastq"][1]
