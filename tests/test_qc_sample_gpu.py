"""The read statistics of a sample through the program (`LiME_fasta --qc-report FILE [--qc-positions P]`) and its Python mirror.  The sample is
the one tests/test_filter_sample_gpu.py makes of the example's first 120 pairs (G tails, N's, low complexity planted), as FASTQ with
sequencer-like qualities and as FASTA.  From FASTQ with --trim-qual, --trim-adapter, --trim-polyx, --min-len and --trim-overlap the report's
`before` must be the numpy model's tables of the raw reads (with the quality tables) and `after` those of the reads that the existing models
of the stages make of them, in the program's order; from FASTA with no stage `after` is `before`.  The same report comes with --batch-reads
7, the classification file is byte for byte that of the run without the flag, nothing else is written, and api.lime_fasta(qc_report=) gives
the same."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from tests import adapter_cases as A
from tests import filter_cases as F
from tests import overlap_cases as V
from tests import qc_cases as Q
from tests import trim_cases as T
from tests.test_fasta_sample_gpu import BIN, READ_LEN, ROOT, _example, _fasta
from tests.test_filter_sample_gpu import PAIRS, _sample

pytestmark = pytest.mark.gpu

A20 = A.TRUSEQ_R1[:20]
FLT = F.params(F.G_, polyx_min=10, min_len=30)
STAGE_ARGS = ["--trim-qual", "20", "--trim-adapter", A20.decode(), "--trim-polyx", "G", "--min-len", "30", "--trim-overlap", "30"]
STAGE_KW = dict(trim_qual=20, trim_adapter=A20.decode(), trim_polyx="G", min_len=30, trim_overlap=30)


@functools.lru_cache(maxsize=None)
def _reads():
    """-> (raw reads per mate, their qualities per mate, the reads as they enter classification per mate)"""
    raw = _sample()[0]
    quals = [T.sample_quals_for(raw[m], seed=31 + m) for m in range(2)]
    done = []
    for m in range(2):
        q = T.trim_model(raw[m], quals[m], 0, 20)[0]
        a = A.trim_model(q, A20, 3, 10)[0]
        done.append(F.filter_model(a, FLT)[0])
    c1, c2, _, _ = V.cut_model(done[0], done[1], 30, 10, insert=V.insert_masks)
    return raw, quals, [c1, c2]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import torch
    from lime_amd import api
    genomes, _, lineage, _ = _example()
    raw, quals, _ = _reads()
    d = str(tmp_path_factory.mktemp("sample_qc"))
    names = ["refs.fasta", "LineageFile.csv", "g.gidx", "raw_1.fasta", "raw_2.fasta", "raw_1.fastq", "raw_2.fastq"]
    f = {k: os.path.join(d, k) for k in names}
    for m in range(2):
        open(f[f"raw_{m + 1}.fastq"], "wb").write(T.fastq_of(raw[m], quals[m], eol=b"\r\n" if m else b"\n"))
        open(f[f"raw_{m + 1}.fasta"], "wb").write(F.fasta_of(raw[m]))
    open(f["refs.fasta"], "wb").write(_fasta(genomes, width=60))
    open(f["LineageFile.csv"], "wb").write(lineage)
    if not os.path.exists(os.path.join(BIN, "LiME_fasta")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    gi = ctx.build_genome_index(genomes)
    gi.save(f["g.gidx"])
    gi.close()
    ctx.close()
    f["dir"] = d
    return f


def _run(files, reads, out, extra, readlen="auto"):
    args = [files[r] for r in reads] + ["--lineage", files["LineageFile.csv"], "--readlen", readlen, "--out", os.path.join(files["dir"], out), "--gidx", files["g.gidx"]] + extra
    before = set(os.listdir(files["dir"]))
    p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=600, cwd=files["dir"])
    return p, set(os.listdir(files["dir"])) - before


def _read(files, name):
    return open(os.path.join(files["dir"], name), "rb").read()


def _load(files, name):
    return json.load(open(os.path.join(files["dir"], name)), object_pairs_hook=Q.key_order)


def test_the_stages_change_what_the_report_shows():
    raw, quals, done = _reads()
    for m in range(2):
        assert sum(map(len, done[m])) < sum(map(len, raw[m])) - 1000 and len({len(r) for r in done[m]}) >= 20 and any(r == b"" for r in done[m])
        assert all(len(r) == READ_LEN for r in raw[m]) and len(raw[m]) == PAIRS
    assert Q.section(Q.model(raw[0], quals[0], 64), 64, True)["q30"] > 0


@pytest.mark.parametrize("n_pos", [None, 64, 100])
def test_fastq_through_every_stage(files, n_pos):
    raw, quals, done = _reads()
    P = 256 if n_pos is None else n_pos
    names = [files["raw_1.fastq"], files["raw_2.fastq"]]
    want = Q.report(names, ["fastq", "fastq"], P, [Q.model(raw[m], quals[m], P) for m in range(2)], [Q.model(done[m], None, P) for m in range(2)])
    p, new = _run(files, ("raw_1.fastq", "raw_2.fastq"), f"plain_{P}.txt", STAGE_ARGS)
    assert p.returncode == 0 and new == {f"plain_{P}.txt"}, p.stderr.decode()[-2000:]
    pos = [] if n_pos is None else ["--qc-positions", str(n_pos)]
    for k, extra in enumerate(([], ["--batch-reads", "7"])):
        out, rep = f"got_{P}_{k}.txt", f"qc_{P}_{k}.json"
        p, new = _run(files, ("raw_1.fastq", "raw_2.fastq"), out, STAGE_ARGS + ["--qc-report", os.path.join(files["dir"], rep)] + pos + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert new == {out, rep}                                             # nothing else is written
        assert _read(files, out) == _read(files, f"plain_{P}.txt")           # the classification file of the run without the flag
        got = _load(files, rep)
        assert got == want, (P, extra)
        lines = [ln for ln in p.stdout.decode().splitlines() if os.path.join(files["dir"], rep) in ln]
        assert len(lines) == 1 and str(P) in lines[0], p.stdout.decode()
    assert _read(files, f"qc_{P}_0.json") == _read(files, f"qc_{P}_1.json")  # the report is identical in both


def test_fasta_with_no_stage_and_one_file(files):
    raw, _, _ = _reads()
    P = 256
    for reads, readlen in ((("raw_1.fasta", "raw_2.fasta"), str(READ_LEN)), (("raw_2.fasta",), "auto"), (("raw_1.fastq", "raw_2.fasta"), "auto")):
        mates = [0, 1] if len(reads) == 2 else [1]
        names = [files[r] for r in reads]
        fmts = [r.rsplit(".", 1)[1] for r in reads]
        quals = _reads()[1]
        tables = [Q.model(raw[m], quals[m] if f == "fastq" else None, P) for m, f in zip(mates, fmts)]
        want = Q.report(names, fmts, P, tables, tables)
        tag = "_".join(fmts) + readlen
        p, new = _run(files, reads, f"plain_{tag}.txt", [], readlen=readlen)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        for k, extra in enumerate(([], ["--batch-reads", "7"])):
            out, rep = f"got_{tag}_{k}.txt", f"qc_{tag}_{k}.json"
            p, new = _run(files, reads, out, ["--qc-report", rep] + extra, readlen=readlen)          # (a relative name: the program runs in the directory)
            assert p.returncode == 0 and new == {out, rep}, p.stderr.decode()[-2000:]
            assert _read(files, out) == _read(files, f"plain_{tag}.txt")
            got = _load(files, rep)
            assert got == want
            for f in got["files"]:                                           # with no stage, after is before's base-derived part
                assert f["after"] == {k2: v for k2, v in f["before"].items() if k2 in f["after"]} and "q20" not in f["after"]
                assert ("q20" in f["before"]) == (f["format"] == "fastq")


def test_through_the_library(files, tmp_path):
    import torch
    from lime_amd import api
    raw, quals, done = _reads()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    try:
        pair = [files["raw_1.fastq"], files["raw_2.fastq"]]
        want_file, out, rep = str(tmp_path / "want.txt"), str(tmp_path / "got.txt"), str(tmp_path / "qc.json")
        c_want = api.lime_fasta(pair, files["LineageFile.csv"], "auto", want_file, gidx=files["g.gidx"], ctx=ctx, **STAGE_KW)
        assert sorted(os.listdir(str(tmp_path))) == ["want.txt"]
        for P, more in ((256, {}), (100, {"qc_positions": 100}), (100, {"qc_positions": 100, "batch_reads": 7})):
            want = Q.report(pair, ["fastq", "fastq"], P, [Q.model(raw[m], quals[m], P) for m in range(2)], [Q.model(done[m], None, P) for m in range(2)])
            c = api.lime_fasta(pair, files["LineageFile.csv"], "auto", out, gidx=files["g.gidx"], ctx=ctx, qc_report=rep, **STAGE_KW, **more)
            assert c == c_want and open(out, "rb").read() == open(want_file, "rb").read()
            assert json.load(open(rep), object_pairs_hook=Q.key_order) == want
            assert sorted(os.listdir(str(tmp_path))) == ["got.txt", "qc.json", "want.txt"]
            os.remove(out); os.remove(rep)
        # no stage and a fixed read length: the FASTQ files are parsed with their qualities for the report alone; after is before's base part
        tables = [Q.model(raw[m], quals[m], 256) for m in range(2)]
        c_plain = api.lime_fasta(pair, files["LineageFile.csv"], READ_LEN, want_file, gidx=files["g.gidx"], ctx=ctx)
        for more in ({}, {"batch_reads": 7}):
            c = api.lime_fasta(pair, files["LineageFile.csv"], READ_LEN, out, gidx=files["g.gidx"], ctx=ctx, qc_report=rep, **more)
            assert c == c_plain and open(out, "rb").read() == open(want_file, "rb").read()
            assert json.load(open(rep), object_pairs_hook=Q.key_order) == Q.report(pair, ["fastq", "fastq"], 256, tables, tables)
            os.remove(out); os.remove(rep)
        # the pieces: Context.docs_qc on the parsed file, SeqReader.set_qc over its batches
        d = ctx.docs_from_fastq_qual(pair[0])
        assert np.array_equal(ctx.docs_qc(d, 64)["tables"], Q.model(raw[0], quals[0], 64))
        d.close()
        r = ctx.seq_reader(pair[1])
        r.set_qc(64)
        for b in r:
            b.close()
        assert np.array_equal(r.qc("raw")["tables"], Q.model(raw[1], quals[1], 64)) and np.array_equal(r.qc("out")["tables"], Q.model(raw[1], None, 64))
        r.close()
    finally:
        ctx.close()
