"""A sample filtered on the device (`LiME_fasta --trim-polyx --max-n --min-complexity --min-len --max-len`, lime_docs_filter_dev,
lime_seq_reader_set_filter) against the existing path fed with reads that were filtered beforehand.  The first 120 pairs of the example
(tests/golden/example_full.npz) are planted: every fourth read ends in a G tail of 15 .. 50 symbols with about 5 % of them wrong; in every
tenth pair both mates hold six adjacent N's in the middle (the flanks still carry 16-mers, so the raw run classifies them); some reads are
replaced by (AC)* -- which fastp's measure lets through: every neighbour differs -- and some by A*.  The numpy model of the rule filters
them and the result is written as a plain FASTQ pair, emptied reads as empty records.  The oracle is the existing program: `LiME_fasta
--readlen auto` on the filtered pair.  `LiME_fasta --readlen auto --trim-polyx G --max-n 5 --min-complexity 30 --min-len 30` on the RAW
pair must write the same classification file byte for byte -- whole and with --batch-reads 7, from FASTQ and from FASTA -- and nothing
else, and print the model's counts.  The comparison shows something only if the filter changes verdicts: the test asserts that the
classification differs from the flagless run's and that the pairs with N's move from C to U."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import filter_cases as F
from tests.test_fasta_sample_gpu import ALPHA, BETA, BIN, READ_LEN, ROOT, _example, _fasta, _to_dev

pytestmark = pytest.mark.gpu

PAIRS = 120
FLT = F.params(F.G_, polyx_min=10, min_len=30, max_n=5, min_complexity=30)
FLT_ARGS = ["--trim-polyx", "G", "--max-n", "5", "--min-complexity", "30", "--min-len", "30"]
FIXED = F.params(max_n=5, min_complexity=30)                                # what a fixed --readlen takes: these only empty reads
FIXED_ARGS = ["--max-n", "5", "--min-complexity", "30"]
N_PAIRS = tuple(range(3, PAIRS, 10))                                        # the pairs whose two mates hold six N's


@functools.lru_cache(maxsize=None)
def _sample():
    """-> (raw reads per mate, filtered reads per mate, the model's info per mate)"""
    _, sets, _, _ = _example()
    rng = np.random.default_rng([F.SEED, 20])
    raw = []
    for m, key in enumerate(("F1", "F2")):
        reads = []
        for k, r in enumerate(sets[key][:PAIRS]):
            r = bytes(r)
            if k in N_PAIRS:
                r = r[:47] + b"NNNNNN" + r[53:]
            elif (k + m) % 4 == 0:
                r = F.plant(rng, r, int(rng.integers(15, 51)), b"G", 0.05)
            elif k % 30 == 7 + m:
                r = (b"AC" * len(r))[:len(r)]
            elif k % 30 == 17 + m:
                r = b"A" * len(r)
            reads.append(r)
        raw.append(reads)
    done, infos = zip(*[F.filter_model(raw[m], FLT) for m in range(2)])
    return raw, list(done), list(infos)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import torch
    from lime_amd import api
    genomes, _, lineage, _ = _example()
    raw, done, _ = _sample()
    d = str(tmp_path_factory.mktemp("sample_filter"))
    names = ["refs.fasta", "LineageFile.csv", "g.gidx", "raw_1.fasta", "raw_2.fasta"] + [f"{k}_{m}.fastq" for k in ("raw", "done", "fixed") for m in (1, 2)]
    f = {k: os.path.join(d, k) for k in names}
    for m in range(2):
        open(f[f"raw_{m + 1}.fastq"], "wb").write(F.fastq_of(raw[m], eol=b"\r\n" if m else b"\n"))
        open(f[f"raw_{m + 1}.fasta"], "wb").write(F.fasta_of(raw[m]))
        open(f[f"done_{m + 1}.fastq"], "wb").write(F.fastq_of(done[m]))
        open(f[f"fixed_{m + 1}.fastq"], "wb").write(F.fastq_of(F.filter_model(raw[m], FIXED)[0]))
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


LINE = (r"^(\S+): read filter \(poly-X (\S+),(\d+), max-len (\d+), min-len (\d+), max-n (\S+), min-complexity (\d+)%\): (\d+) of (\d+) reads with a poly-X tail, "
        r"(\d+) capped, (\d+) short, (\d+) with many N, (\d+) of low complexity, (\d+) symbols before, (\d+) after\.$")


def _counts(ln):
    keys = ("n_polyx", "n_reads", "n_capped", "n_short", "n_many_n", "n_low_complexity", "symbols_in", "symbols_out")
    return dict(zip(keys, (int(x) for x in ln[7:])))


def _read(files, name):
    return open(os.path.join(files["dir"], name), "rb").read()


def test_the_generator_gives_the_comparison_something_to_show():
    raw, done, infos = _sample()
    tot = {k: infos[0][k] + infos[1][k] for k in F.INFO_KEYS}
    print(tot)
    assert tot["n_polyx"] >= 40 and tot["n_many_n"] == 2 * len(N_PAIRS) and tot["n_low_complexity"] >= 4 and tot["n_capped"] == 0
    for m in range(2):
        assert F.filter_model(raw[m], FLT, keep=F.keep_words)[0] == done[m]
        assert all(len(r) == READ_LEN for r in raw[m]) and all(done[m][k] == b"" for k in N_PAIRS)
        assert any(r == (b"AC" * 50) for r in done[m])                      # (AC)* passes the measure: every neighbour differs
    assert len({len(r) for m in range(2) for r in done[m]}) >= 20


def test_the_program_on_raw_reads_gives_the_prefiltered_runs_file(files):
    _, _, infos = _sample()
    p, new = _run(files, ("done_1.fastq", "done_2.fastq"), "want.txt", [])                 # the oracle: today's program on the filtered pair
    assert p.returncode == 0 and new == {"want.txt"}, p.stderr.decode()[-2000:]
    want = _read(files, "want.txt")
    assert want.count(b"\n") >= PAIRS
    for fmt in ("fastq", "fasta"):
        for extra in ([], ["--batch-reads", "7"]):
            out = f"got_{fmt}_{len(extra)}.txt"
            p, new = _run(files, (f"raw_1.{fmt}", f"raw_2.{fmt}"), out, FLT_ARGS + extra)
            assert p.returncode == 0, p.stderr.decode()[-2000:]
            assert _read(files, out) == want, (fmt, extra)
            assert new == {out}                                              # nothing else is written
            lines = re.findall(LINE, p.stdout.decode(), re.M)
            assert len(lines) == 2, p.stdout.decode()
            for m, ln in enumerate(lines):
                assert ln[:7] == (files[f"raw_{m + 1}.{fmt}"], "G", "10", "0", "30", "5", "30"), ln
                assert _counts(ln) == infos[m], (ln, infos[m])
            assert b"numReads: %d" % PAIRS in p.stdout


def test_the_filter_changes_verdicts_and_the_n_reads_go_from_c_to_u(files):
    p, _ = _run(files, ("raw_1.fastq", "raw_2.fastq"), "flagless.txt", [])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    p, _ = _run(files, ("raw_1.fastq", "raw_2.fastq"), "filtered.txt", FLT_ARGS)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    a, b = _read(files, "flagless.txt").split(b"\n")[1:], _read(files, "filtered.txt").split(b"\n")[1:]      # (behind the header line: read k is line k)
    assert len(a) == PAIRS + 1 and a[0].split(b",")[1] == b"0"
    differ = sum(x != y for x, y in zip(a, b))
    c_to_u = [k for k in N_PAIRS if a[k].startswith(b"C,") and b[k].startswith(b"U,")]
    print("lines on which the filtered run differs from the flagless --readlen auto run of the raw files:", differ, "of", len(a), "; C -> U among the N pairs:", len(c_to_u))
    assert len(a) == len(b) and differ >= 1
    assert all(b[k].startswith(b"U,") for k in N_PAIRS) and len(c_to_u) >= 1


def test_a_fixed_readlen_takes_the_three_filters(files):
    raw, _, _ = _sample()
    p, _ = _run(files, ("fixed_1.fastq", "fixed_2.fastq"), "want_fixed.txt", [], readlen=str(READ_LEN))
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    for k, extra in enumerate(([], ["--batch-reads", "7"])):
        p, new = _run(files, ("raw_1.fastq", "raw_2.fasta"), f"got_fixed_{k}.txt", FIXED_ARGS + extra, readlen=str(READ_LEN))
        assert p.returncode == 0 and new == {f"got_fixed_{k}.txt"}, p.stderr.decode()[-2000:]
        assert _read(files, f"got_fixed_{k}.txt") == _read(files, "want_fixed.txt")
        lines = re.findall(LINE, p.stdout.decode(), re.M)
        assert [ln[1:7] for ln in lines] == [("-", "0", "0", "0", "5", "30")] * 2
        assert [_counts(ln) for ln in lines] == [F.filter_model(raw[m], FIXED)[1] for m in range(2)]


@pytest.mark.parametrize("extra", [["--trim-polyx", "G"], ["--max-len", "90"], ["--max-n", "5", "--trim-polyx", "G,12"]])
def test_a_flag_that_changes_lengths_needs_readlen_auto(files, extra):
    p, new = _run(files, ("raw_1.fastq", "raw_2.fastq"), "no.txt", extra, readlen=str(READ_LEN))
    assert p.returncode == 1 and b"Error usage" in p.stderr and b"--trim-polyx" in p.stderr and not new


def test_reads_of_300_symbols_run_with_max_len_255(files, tmp_path):
    """a read of 300 symbols ends a --readlen auto run as before; --max-len 255 cuts it and the run is that of the file cut beforehand"""
    raw, _, _ = _sample()
    rng = np.random.default_rng([F.SEED, 21])
    reads = [list(raw[0][:20]), list(raw[1][:20])]
    reads[1][13] = reads[1][13] + F.no_tail(rng, 200)
    reads[0][4] = reads[0][4] + F.no_tail(rng, 156)                         # 256 symbols: one more than fits
    p255 = F.params(max_len=255)
    paths = {k: [str(tmp_path / f"{k}_{m + 1}.fastq") for m in range(2)] for k in ("long", "cut")}
    for m in range(2):
        open(paths["long"][m], "wb").write(F.fastq_of(reads[m]))
        open(paths["cut"][m], "wb").write(F.fastq_of(F.filter_model(reads[m], p255)[0]))
    base = ["--lineage", files["LineageFile.csv"], "--readlen", "auto", "--gidx", files["g.gidx"]]
    want = str(tmp_path / "want.txt")
    p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + paths["cut"] + base + ["--out", want], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    for extra in ([], ["--batch-reads", "6"]):
        out = str(tmp_path / "out.txt")
        p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + paths["long"] + base + ["--out", out] + extra, capture_output=True, timeout=600)
        assert p.returncode == 1 and "read 4 holds 256 symbols" in p.stderr.decode(), p.stderr.decode()
        assert not [n for n in os.listdir(str(tmp_path)) if n.startswith("out.txt")]
        p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + paths["long"] + base + ["--out", out, "--max-len", "255"] + extra, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert open(out, "rb").read() == open(want, "rb").read()
        lines = re.findall(LINE, p.stdout.decode(), re.M)
        assert [_counts(ln)["n_capped"] for ln in lines] == [1, 1] and [ln[3] for ln in lines] == ["255", "255"]
        os.remove(out)


def test_a_pair_with_one_mate_emptied(files, tmp_path):
    """read 5 of the first mates is only G: an empty read in its place, its pair classified by the other mate alone"""
    raw, done, _ = _sample()
    reads = [list(raw[0][:20]), list(raw[1][:20])]
    cut = [list(done[0][:20]), list(done[1][:20])]
    assert 5 not in N_PAIRS and cut[1][5]
    reads[0][5] = b"G" * 100
    cut[0][5] = b""
    assert F.keep_loop(reads[0][5], FLT) == (0, {"n_polyx", "n_short"})
    paths = {k: [str(tmp_path / f"{k}_{m + 1}.fastq") for m in range(2)] for k in ("raw", "cut")}
    for m in range(2):
        open(paths["raw"][m], "wb").write(F.fastq_of(reads[m]))
        open(paths["cut"][m], "wb").write(F.fastq_of(cut[m]))
    base = ["--lineage", files["LineageFile.csv"], "--readlen", "auto", "--gidx", files["g.gidx"]]
    want = str(tmp_path / "want.txt")
    p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + paths["cut"] + base + ["--out", want], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    for extra in ([], ["--batch-reads", "6"]):
        out = str(tmp_path / "out.txt")
        p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + paths["raw"] + base + ["--out", out] + FLT_ARGS + extra, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert open(out, "rb").read() == open(want, "rb").read()
        first = _counts(re.findall(LINE, p.stdout.decode(), re.M)[0])
        assert first == F.filter_model(reads[0], FLT)[1] and first["n_short"] >= 1
        os.remove(out)


def test_through_the_library(files, tmp_path):
    import torch
    from lime_amd import api
    genomes, _, _, _ = _example()
    raw, done, infos = _sample()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    tx = api.Taxonomy(files["LineageFile.csv"], 1, False, len(genomes))
    try:
        gi = ctx.load_genome_index(files["g.gidx"])
        fixed = [ctx.docs_from_arrays_dev(*_to_dev(done[m])) for m in range(2)]
        want, w_counts, _ = ctx.classify_sample(fixed, gi, tx, ALPHA, api.NORM_PER_READ, BETA)
        mates = []
        for m in range(2):
            d = ctx.docs_from_file(files[f"raw_{m + 1}.fastq"])
            t, info = ctx.docs_filter(d, **FLT)
            assert info == infos[m]
            assert np.array_equal(t.get()[0], fixed[m].get()[0]) and np.array_equal(t.get()[1], fixed[m].get()[1])
            mates.append(t)
            d.close()
        got, counts, _ = ctx.classify_sample(mates, gi, tx, ALPHA, api.NORM_PER_READ, BETA)
        assert got.dtype.names == want.dtype.names and all(np.array_equal(got[k], want[k]) for k in want.dtype.names) and counts == w_counts
        readers = [ctx.seq_reader(files[f"raw_{m + 1}.fastq"]) for m in range(2)]
        for r in readers:
            r.set_filter(**FLT)
        streamed, s_counts, per_batch = ctx.classify_sample_stream(readers, gi, tx, ALPHA, api.NORM_PER_READ, BETA, 7)
        assert streamed.tobytes() == want.tobytes() and s_counts == w_counts and len(per_batch) == (PAIRS + 6) // 7
        assert [r.filter_info() for r in readers] == infos
        for x in fixed + mates + readers:
            x.close()
        gi.close()
        # the Python mirror of the program
        want_file, out = str(tmp_path / "want.txt"), str(tmp_path / "got.txt")
        api.write_classification(want_file, want)
        pair = [files["raw_1.fastq"], files["raw_2.fastq"]]
        kw = dict(max_n=5, min_complexity=30, min_len=30)
        for more in ({"trim_polyx": "G"}, {"trim_polyx": ("g", 10), "batch_reads": 7}, {"trim_polyx": "G,10", "max_len": 255}):
            c = api.lime_fasta(pair, files["LineageFile.csv"], "auto", out, gidx=files["g.gidx"], ctx=ctx, **kw, **more)
            assert c == w_counts and open(out, "rb").read() == open(want_file, "rb").read()
            os.remove(out)
        # a fixed read length takes the filters that only empty reads
        c_want = api.lime_fasta([files["fixed_1.fastq"], files["fixed_2.fastq"]], files["LineageFile.csv"], READ_LEN, want_file, gidx=files["g.gidx"], ctx=ctx)
        for more in ({}, {"batch_reads": 7}):
            c = api.lime_fasta(pair, files["LineageFile.csv"], READ_LEN, out, gidx=files["g.gidx"], ctx=ctx, max_n=5, min_complexity=30, **more)
            assert c == c_want and open(out, "rb").read() == open(want_file, "rb").read()
            os.remove(out)
        for bad in (dict(read_len=100, trim_polyx="G"), dict(read_len=100, max_len=90), dict(trim_polyx="N"), dict(trim_polyx="G,0"), dict(trim_polyx="G,256"),
                    dict(min_complexity=101), dict(max_n=-1), dict(min_len=-1)):
            k2 = dict(read_len="auto"); k2.update(bad)
            with pytest.raises(ValueError):
                api.lime_fasta(pair, files["LineageFile.csv"], k2.pop("read_len"), out, gidx=files["g.gidx"], ctx=ctx, **k2)
        assert not os.path.exists(out)
    finally:
        tx.close()
        ctx.close()
