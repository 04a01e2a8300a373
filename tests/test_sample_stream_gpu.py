"""A sample classified batch by batch (lime_classify_sample_stream, bin/LiME_fasta --batch-reads, api.lime_fasta(batch_reads=...)): the example
at full size (tests/golden/example_full.npz, 10 000 pairs) must give the reference's own Classify output byte for byte at every batch
size, as FASTA and as FASTQ, through large and small windows; on the first 50 pairs the verdicts and summed counts are those of
Context.classify_sample, the existing call on the whole 50; mates of different lengths, a malformed mate and a failing sink end the
call and leave no output file; without --batch-reads the program prints and writes what it did before."""
import functools
import os
import re
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


def _fastq(docs, eol=b"\n"):
    """four-line records; every third record's quality string begins with '@' or '+'"""
    out = []
    for k, d in enumerate(docs):
        q = bytes(33 + (7 * k + j) % 41 for j in range(len(d)))
        if k % 3 == 0 and q:
            q = (b"@" if k % 2 else b"+") + q[1:]
        out.append(b"@seq%d/1 some text" % k + eol + d + eol + (b"+" if k % 5 else b"+seq%d" % k) + eol + q + eol)
    return b"".join(out)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """both mates as FASTQ (reads_2 with CRLF) and as FASTA (reads_1 in 60-column lines), their first 50 records, the genomes, the lineage, the index"""
    genomes, sets, lineage, _ = _example()
    d = str(tmp_path_factory.mktemp("sample_stream"))
    names = ("reads_1.fastq", "reads_2.fastq", "reads_1.fasta", "reads_2.fasta", "head_1.fastq", "head_2.fastq", "head_1.fasta", "head_2.fasta", "short_2.fastq",
             "refs.fasta", "LineageFile.csv", "g.gidx")
    f = {k: os.path.join(d, k) for k in names}
    for stem, n in (("reads", None), ("head", 50)):
        open(f[stem + "_1.fastq"], "wb").write(_fastq(sets["F1"][:n]))
        open(f[stem + "_2.fastq"], "wb").write(_fastq(sets["F2"][:n], eol=b"\r\n"))
        open(f[stem + "_1.fasta"], "wb").write(_fasta(sets["F1"][:n], width=60))
        open(f[stem + "_2.fasta"], "wb").write(_fasta(sets["F2"][:n], eol=b"\r\n"))
    open(f["short_2.fastq"], "wb").write(_fastq(sets["F2"][:49], eol=b"\r\n"))
    open(f["refs.fasta"], "wb").write(_fasta(genomes, width=60))
    open(f["LineageFile.csv"], "wb").write(lineage)
    for exe in ("LiME_fasta", "BuildIndex"):
        if not os.path.exists(os.path.join(BIN, exe)):
            subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    p = subprocess.run([os.path.join(BIN, "BuildIndex"), "--refs", f["refs.fasta"], os.path.join(d, "g")], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    f["dir"] = d
    return f


def _run(files, reads, out, extra):
    args = list(reads) + ["--gidx", files["g.gidx"], "--lineage", files["LineageFile.csv"], "--readlen", str(READ_LEN), "--out", out] + list(extra)
    return subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=600, cwd=files["dir"])


@pytest.mark.parametrize("ext", ["fasta", "fastq"])
@pytest.mark.parametrize("batch", [3333, 4096, 10000, 10001])
def test_the_program_in_batches_gives_the_references_classification(files, batch, ext):
    _, sets, _, want = _example()
    for window in (1_000_000, 4097):
        out = os.path.join(files["dir"], f"classification_{ext}_{batch}_{window}.txt")
        before = set(os.listdir(files["dir"]))
        p = _run(files, [files["reads_1." + ext], files["reads_2." + ext]], out, ["--batch-reads", str(batch), "--window-bytes", str(window)])
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert open(out, "rb").read() == want
        assert set(os.listdir(files["dir"])) - before == {os.path.basename(out)}       # nothing else is written
        n_batches = -(-len(sets["F1"]) // batch)
        assert b"numGenomes: 3\n" in p.stdout and b"numReads: %d (%d batches of at most %d)\n" % (len(sets["F1"]), n_batches, batch) in p.stdout
        assert p.stdout.count(b"clusters summed over the batches, maximum length") == 4
        os.remove(out)


@pytest.fixture(scope="module")
def head(files):
    """the first 50 pairs through the existing calls: Context.classify_sample on whole Docs, single-end and paired, with and without ebwt"""
    import torch
    from lime_amd import api
    genomes, _, _, _ = _example()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    gi = ctx.load_genome_index(files["g.gidx"])
    tx = api.Taxonomy(files["LineageFile.csv"], 1, False, len(genomes))
    want = {}
    for n_mates in (1, 2):
        for ebwt in (True, False):
            mates = [ctx.docs_from_file(files["head_%d.fastq" % (m + 1)]) for m in range(n_mates)]
            v, counts, _ = ctx.classify_sample(mates, gi, tx, ALPHA, NORM, BETA, ebwt=ebwt)
            want[(n_mates, ebwt)] = (v.copy(), counts)
            for m in mates:
                m.close()
    yield ctx, gi, tx, want
    tx.close()
    ctx.close()


@pytest.mark.parametrize("ebwt", [True, False], ids=["ebwt", "no ebwt"])
@pytest.mark.parametrize("n_mates", [1, 2], ids=["single-end", "paired"])
def test_the_stream_call_gives_the_whole_calls_verdicts(files, head, n_mates, ebwt):
    ctx, gi, tx, want = head
    w_v, w_counts = want[(n_mates, ebwt)]
    assert len(w_v) == 50 and sum(w_counts) == 50 and w_counts[0] > 0
    for k, batch in enumerate((1, 2, 7, 49, 50)):
        ext = "fastq" if k % 2 == 0 else "fasta"
        readers = [ctx.seq_reader(files["head_%d.%s" % (m + 1, ext)], (0, 4097, 700)[k % 3]) for m in range(n_mates)]
        v, counts, stats = ctx.classify_sample_stream(readers, gi, tx, ALPHA, NORM, BETA, batch, ebwt=ebwt)
        assert v.tobytes() == w_v.tobytes() and counts == w_counts, (batch, counts, w_counts)
        assert len(stats) == -(-50 // batch) and all(len(s) == 2 * n_mates for s in stats)
        seen = []
        n, counts2, n_batches = ctx.classify_sample_stream([ctx.seq_reader(files["head_%d.%s" % (m + 1, ext)]) for m in range(n_mates)], gi, tx, ALPHA, NORM,
                                                           BETA, batch, ebwt=ebwt, sink=lambda first, vv, st: seen.append((first, vv.copy())))
        assert (n, counts2, n_batches) == (50, w_counts, len(stats)) and [f for f, _ in seen] == list(range(0, 50, batch))
        assert np.concatenate([x for _, x in seen]).tobytes() == w_v.tobytes()
        for r in readers:
            assert r.info()["records"] == 50
            r.close()


def test_refusals_of_the_stream_call(files, head):
    from lime_amd import _lib, api
    ctx, gi, tx, _ = head
    new = lambda *names: [ctx.seq_reader(files[n]) for n in names]
    # mates of 50 and 49 records: both counts
    for batch in (7, 49, 50, 100):
        with pytest.raises(api.LimeError) as e:
            ctx.classify_sample_stream(new("head_1.fastq", "short_2.fastq"), gi, tx, ALPHA, NORM, BETA, batch)
        assert e.value.code == _lib.ERR_ARG and "the read sets hold different numbers of reads (50 in set 0, 49 in set 1)" in str(e.value), str(e.value)
    # the argument refusals come before any read
    r = new("head_1.fastq")
    for kwargs, text in ((dict(alpha=0), "alpha is 0"), (dict(batch=0), "batch_reads is 0"), (dict(lcp_cap=3), "lcp values capped at 3")):
        with pytest.raises(api.LimeError) as e:
            ctx.classify_sample_stream(r, gi, tx, kwargs.get("alpha", ALPHA), NORM, BETA, kwargs.get("batch", 10), lcp_cap=kwargs.get("lcp_cap", 0))
        assert e.value.code == _lib.ERR_ARG and text in str(e.value) and r[0].info()["records"] == 0, str(e.value)
    with pytest.raises(api.LimeError) as e:
        ctx.classify_sample_stream([], gi, tx, ALPHA, NORM, BETA, 10)
    assert e.value.code == _lib.ERR_ARG and "n_mates is 0" in str(e.value)
    # a sink that returns 5 ends the call with 5, after the first batch
    calls = []
    with pytest.raises(api.LimeError) as e:
        ctx.classify_sample_stream(r, gi, tx, ALPHA, NORM, BETA, 10, sink=lambda first, v, st: calls.append(first) or 5)
    assert e.value.code == 5 and calls == [0] and r[0].info()["records"] == 10
    # a sink that raises: the exception comes out
    with pytest.raises(KeyError):
        ctx.classify_sample_stream(r, gi, tx, ALPHA, NORM, BETA, 10, sink=lambda first, v, st: {}["x"])
    # an empty sample
    empty = os.path.join(files["dir"], "empty.fasta")
    open(empty, "wb").write(b"")
    with pytest.raises(api.LimeError) as e:
        ctx.classify_sample_stream([ctx.seq_reader(empty)], gi, tx, ALPHA, NORM, BETA, 10)
    assert e.value.code == _lib.ERR_ARG and "hold no reads" in str(e.value)


def test_the_program_refuses_and_leaves_no_output(files):
    out = os.path.join(files["dir"], "no.txt")
    before = set(os.listdir(files["dir"]))
    p = _run(files, [files["head_1.fastq"], files["short_2.fastq"]], out, ["--batch-reads", "7"])
    assert p.returncode != 0 and b"different numbers of reads (50 in set 0, 49 in set 1)" in p.stderr, p.stderr
    assert set(os.listdir(files["dir"])) == before
    # a mate malformed in its third batch: the file's line
    lines = open(files["head_2.fastq"], "rb").read().split(b"\n")
    lines[4 * 17 + 3] = lines[4 * 17 + 3][:-2] + b"\r"                      # record 17's quality string one short (the line keeps its CR)
    bad = os.path.join(files["dir"], "broken_2.fastq")
    open(bad, "wb").write(b"\n".join(lines))
    before = set(os.listdir(files["dir"]))
    p = _run(files, [files["head_1.fastq"], bad], out, ["--batch-reads", "7", "--window-bytes", "4097"])
    err = p.stderr.decode()
    assert p.returncode != 0 and QC.refusal_of(err.strip().splitlines()[-1]) == (4 * 17 + 4, 2), err
    assert set(os.listdir(files["dir"])) == before
    for extra in (["--batch-reads", "0"], ["--window-bytes", "100"], ["--batch-reads"]):
        p = _run(files, [files["head_1.fastq"]], out, extra)
        assert p.returncode == 1 and b"Error usage" in p.stderr and b"--batch-reads N" in p.stderr
    assert set(os.listdir(files["dir"])) == before


def test_the_python_mirror(files, tmp_path):
    from lime_amd import api
    _, _, _, want = _example()
    out = str(tmp_path / "classification_py.txt")
    counts = api.lime_fasta([files["reads_1.fastq"], files["reads_2.fasta"]], files["LineageFile.csv"], READ_LEN, out, gidx=files["g.gidx"], batch_reads=3333,
                            window_bytes=1 << 20)
    assert open(out, "rb").read() == want and sum(counts) == 10000 and os.listdir(tmp_path) == ["classification_py.txt"]
    whole = str(tmp_path / "whole.txt")
    assert api.lime_fasta([files["reads_1.fastq"], files["reads_2.fasta"]], files["LineageFile.csv"], READ_LEN, whole, gidx=files["g.gidx"]) == counts
    assert open(whole, "rb").read() == want
    with pytest.raises(api.LimeError):               # a failure half-way leaves no output file
        api.lime_fasta([files["head_1.fastq"], files["short_2.fastq"]], files["LineageFile.csv"], READ_LEN, str(tmp_path / "no.txt"), gidx=files["g.gidx"],
                       batch_reads=7)
    assert sorted(os.listdir(tmp_path)) == ["classification_py.txt", "whole.txt"]


def test_without_the_flag_the_program_is_what_it_was(files):
    """stdout in the order and words of the unbatched program (numReads and numGenomes together in front of the lineage, one line per
    collection with its clusters and maximum length), the same file"""
    _, sets, _, want = _example()
    out = os.path.join(files["dir"], "classification_whole.txt")
    p = _run(files, [files["reads_1.fastq"], files["reads_2.fasta"]], out, [])
    assert p.returncode == 0 and open(out, "rb").read() == want
    text = p.stdout.decode()
    assert "numReads: 10000\nnumGenomes: 3\nReading " in text and "batches" not in text
    assert len(re.findall(r": \d+ clusters, maximum length \d+\.\n", text)) == 4
    assert "Number of successfully classified reads: " in text and re.search(r"\nTime: [0-9.]+\n$", text)
    os.remove(out)
