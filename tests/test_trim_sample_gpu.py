"""A sample trimmed by quality on the device (`LiME_fasta --trim-qual`, lime_docs_trim_dev, lime_seq_reader_set_trim) against the existing path
fed with reads that were trimmed beforehand.  The first 120 pairs of the example (tests/golden/example_full.npz) get synthetic qualities
from the seeded generator of tests/trim_cases.py; the numpy model of the rule trims them and the result is written as a plain FASTQ pair,
empty reads included.  The oracle is the existing program: `LiME_fasta --readlen auto` on the trimmed pair.  `LiME_fasta --readlen auto
--trim-qual 20,20` on the RAW pair must write the same classification file byte for byte -- whole and with --batch-reads 7, with one --gidx,
two index shards and --refs -- and nothing else, and print the model's counts.  Through the library the comparison is with documents made
from the model's arrays.  The comparison shows something only if the trim changes verdicts: the test asserts that it changes many reads,
empties some, leaves many lengths and moves at least five verdicts away from the untrimmed run's."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import trim_cases as T
from tests.test_fasta_sample_gpu import ALPHA, BETA, BIN, ROOT, _example, _fasta, _to_dev

pytestmark = pytest.mark.gpu

PAIRS = 120
Q5, Q3 = 20, 20


def _sample():
    """-> (raw reads per mate, qualities per mate, trimmed reads per mate, the model's info per mate)"""
    _, sets, _, _ = _example()
    raw = [[bytes(r) for r in sets[k][:PAIRS]] for k in ("F1", "F2")]
    quals = [T.sample_quals_for(raw[0], seed=7), T.sample_quals_for(raw[1], seed=8)]
    trimmed, infos = zip(*[T.trim_model(raw[m], quals[m], Q5, Q3) for m in range(2)])
    return raw, quals, list(trimmed), list(infos)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import torch
    from lime_amd import api
    genomes, _, lineage, _ = _example()
    raw, quals, trimmed, _ = _sample()
    d = str(tmp_path_factory.mktemp("sample_trim"))
    f = {k: os.path.join(d, k) for k in ("raw_1.fastq", "raw_2.fastq", "cut_1.fastq", "cut_2.fastq", "refs.fasta", "LineageFile.csv", "g.gidx", "s0.gidx", "s1.gidx")}
    for m in range(2):
        open(f[f"raw_{m + 1}.fastq"], "wb").write(T.fastq_of(raw[m], quals[m], eol=b"\r\n" if m else b"\n"))
        open(f[f"cut_{m + 1}.fastq"], "wb").write(T.fastq_of(trimmed[m], [b"I" * len(r) for r in trimmed[m]]))
    open(f["refs.fasta"], "wb").write(_fasta(genomes, width=60))
    open(f["LineageFile.csv"], "wb").write(lineage)
    if not os.path.exists(os.path.join(BIN, "LiME_fasta")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    for name, part in (("g.gidx", genomes), ("s0.gidx", genomes[:1]), ("s1.gidx", genomes[1:])):
        gi = ctx.build_genome_index(part)
        gi.save(f[name])
        gi.close()
    ctx.close()
    f["dir"] = d
    return f


def _run(files, reads, out, index, extra):
    args = [files[r] for r in reads] + ["--lineage", files["LineageFile.csv"], "--readlen", "auto", "--out", os.path.join(files["dir"], out)] + index + extra
    before = set(os.listdir(files["dir"]))
    p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=600, cwd=files["dir"])
    return p, set(os.listdir(files["dir"])) - before


def _index_args(files, index):
    return {"gidx": ["--gidx", files["g.gidx"]], "two shards": ["--gidx", files["s0.gidx"], "--gidx", files["s1.gidx"]], "refs": ["--refs", files["refs.fasta"]]}[index]


def test_the_generator_gives_the_comparison_something_to_show():
    raw, quals, trimmed, infos = _sample()
    changed = [len(trimmed[m][i]) != len(raw[m][i]) for m in range(2) for i in range(PAIRS)]
    pairs_changed = sum(1 for i in range(PAIRS) if changed[i] or changed[PAIRS + i])
    emptied = infos[0]["n_empty"] + infos[1]["n_empty"]
    lengths = {len(r) for m in range(2) for r in trimmed[m]}
    cut5 = sum(1 for m in range(2) for b in quals[m] if T.bounds_loop(b, Q5, Q3)[0] > 0)
    print("pairs with a changed mate", pairs_changed, "reads emptied", emptied, "distinct lengths", len(lengths), "reads with a 5' cut", cut5)
    assert pairs_changed >= 30 and emptied >= 3 and len(lengths) >= 10 and cut5 >= 5
    assert any(0 < len(r) < ALPHA for m in range(2) for r in trimmed[m])     # (a read cut below alpha: norm 1, empty rows)
    for m in range(2):
        assert T.trim_model(raw[m], quals[m], Q5, Q3, bounds=T.bounds_loop)[0] == trimmed[m]


@pytest.mark.parametrize("index", ["gidx", "two shards", "refs"])
def test_the_program_on_raw_reads_gives_the_pretrimmed_runs_file(files, index):
    _, _, _, infos = _sample()
    ix = _index_args(files, index)
    tag = index.replace(" ", "_")
    p, new = _run(files, ("cut_1.fastq", "cut_2.fastq"), f"want_{tag}.txt", ix, [])           # the oracle: today's program on the trimmed pair
    assert p.returncode == 0 and new == {f"want_{tag}.txt"}, p.stderr.decode()[-2000:]
    want = open(os.path.join(files["dir"], f"want_{tag}.txt"), "rb").read()
    assert want.count(b"\n") >= PAIRS
    for extra in ([], ["--batch-reads", "7"]):
        out = f"got_{tag}_{len(extra)}.txt"
        p, new = _run(files, ("raw_1.fastq", "raw_2.fastq"), out, ix, ["--trim-qual", f"{Q5},{Q3}"] + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert open(os.path.join(files["dir"], out), "rb").read() == want, (index, extra)
        assert new == {out}                                                  # nothing else is written
        lines = re.findall(r"^(\S+): quality trim (\d+),(\d+): (\d+) of (\d+) reads changed, (\d+) emptied, (\d+) symbols before, (\d+) after\.$", p.stdout.decode(), re.M)
        assert len(lines) == 2, p.stdout.decode()
        for m, ln in enumerate(lines):
            i = infos[m]
            assert ln[0] == files[f"raw_{m + 1}.fastq"] and [int(x) for x in ln[1:]] == [Q5, Q3, i["n_changed"], i["n_reads"], i["n_empty"], i["symbols_in"], i["symbols_out"]], ln
        assert b"numReads: %d" % PAIRS in p.stdout


def test_the_trim_moves_verdicts_and_one_cutoff_trims_the_3_prime_end_only(files):
    p, _ = _run(files, ("raw_1.fastq", "raw_2.fastq"), "untrimmed.txt", _index_args(files, "gidx"), [])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    p, _ = _run(files, ("raw_1.fastq", "raw_2.fastq"), "trimmed.txt", _index_args(files, "gidx"), ["--trim-qual", f"{Q5},{Q3}"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    a = open(os.path.join(files["dir"], "untrimmed.txt"), "rb").read().split(b"\n")
    b = open(os.path.join(files["dir"], "trimmed.txt"), "rb").read().split(b"\n")
    differ = sum(x != y for x, y in zip(a, b))
    print("lines on which the trimmed run differs from the untrimmed --readlen auto run of the raw files:", differ, "of", len(a))
    assert len(a) == len(b) and differ >= 5
    # --trim-qual Q is --trim-qual 0,Q
    raw, quals, _, _ = _sample()
    p, _ = _run(files, ("raw_1.fastq",), "q.txt", _index_args(files, "gidx"), ["--trim-qual", "20"])
    q, _ = _run(files, ("raw_1.fastq",), "0q.txt", _index_args(files, "gidx"), ["--trim-qual", "0,20"])
    assert p.returncode == 0 and q.returncode == 0, p.stderr.decode()[-2000:]
    assert open(os.path.join(files["dir"], "q.txt"), "rb").read() == open(os.path.join(files["dir"], "0q.txt"), "rb").read()
    i = T.trim_model(raw[0], quals[0], 0, 20)[1]
    assert b"quality trim 0,20: %d of %d reads changed, %d emptied, %d symbols before, %d after." % (i["n_changed"], PAIRS, i["n_empty"], i["symbols_in"], i["symbols_out"]) in p.stdout


def test_through_the_library(files, tmp_path):
    import torch
    from lime_amd import api
    genomes, _, _, _ = _example()
    raw, quals, trimmed, infos = _sample()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    tx = api.Taxonomy(files["LineageFile.csv"], 1, False, len(genomes))
    try:
        gi = ctx.load_genome_index(files["g.gidx"])
        fixed = [ctx.docs_from_arrays_dev(*_to_dev(trimmed[m])) for m in range(2)]
        want, w_counts, _ = ctx.classify_sample(fixed, gi, tx, ALPHA, api.NORM_PER_READ, BETA)
        mates = []
        for m in range(2):
            d = ctx.docs_from_fastq_qual(files[f"raw_{m + 1}.fastq"])
            t, info = ctx.docs_trim(d, Q5, Q3)
            assert info == infos[m]
            assert np.array_equal(t.get()[0], fixed[m].get()[0]) and np.array_equal(t.get()[1], fixed[m].get()[1])
            mates.append(t)
            d.close()
        got, counts, _ = ctx.classify_sample(mates, gi, tx, ALPHA, api.NORM_PER_READ, BETA)
        assert got.dtype.names == want.dtype.names and all(np.array_equal(got[k], want[k]) for k in want.dtype.names) and counts == w_counts
        emptied_both = [i for i in range(PAIRS) if not trimmed[0][i] and not trimmed[1][i]]
        assert all(got[i]["type"] == ord("U") for i in emptied_both)
        readers = [ctx.seq_reader(files[f"raw_{m + 1}.fastq"]) for m in range(2)]
        for r in readers:
            r.set_trim(Q5, Q3)
        streamed, s_counts, per_batch = ctx.classify_sample_stream(readers, gi, tx, ALPHA, api.NORM_PER_READ, BETA, 7)
        assert streamed.tobytes() == want.tobytes() and s_counts == w_counts and len(per_batch) == (PAIRS + 6) // 7
        assert [r.trim_info() for r in readers] == infos
        for x in fixed + mates + readers:
            x.close()
        gi.close()
        # the Python mirror of the program
        want_file, out = str(tmp_path / "want.txt"), str(tmp_path / "got.txt")
        api.write_classification(want_file, want)
        for kw in ({}, {"batch_reads": 7}):
            c = api.lime_fasta([files["raw_1.fastq"], files["raw_2.fastq"]], files["LineageFile.csv"], "auto", out, gidx=files["g.gidx"], ctx=ctx, trim_qual=(Q5, Q3), **kw)
            assert c == w_counts and open(out, "rb").read() == open(want_file, "rb").read()
            os.remove(out)
        with pytest.raises(ValueError):
            api.lime_fasta([files["raw_1.fastq"]], files["LineageFile.csv"], 100, out, gidx=files["g.gidx"], ctx=ctx, trim_qual=20)
        with pytest.raises(ValueError):
            api.lime_fasta([files["refs.fasta"]], files["LineageFile.csv"], "auto", out, gidx=files["g.gidx"], ctx=ctx, trim_qual="5,20")
        assert not os.path.exists(out)
    finally:
        tx.close()
        ctx.close()


def test_a_fasta_reads_file_is_named_and_leaves_no_output(files):
    p, new = _run(files, ("raw_1.fastq", "refs.fasta"), "no.txt", _index_args(files, "gidx"), ["--trim-qual", "20,20"])
    assert p.returncode == 1 and files["refs.fasta"].encode() in p.stderr and b"FASTQ" in p.stderr and not new


def test_the_255_symbol_limit_holds_for_the_trimmed_length(files, tmp_path):
    """a raw read of 300 symbols trimmed to 240 passes; one whose trimmed length is 256 is refused as an untrimmed one of 256 is, with the read
    set and the read's index"""
    _, sets, _, _ = _example()
    reads = [[bytes(r) for r in sets[k][:20]] for k in ("F1", "F2")]
    quals = [[bytes([T.Q(35)]) * len(r) for r in reads[m]] for m in range(2)]
    long_read = (reads[1][13] * 3)[:300]
    for keep, ok in ((240, True), (256, False)):
        reads[1][13] = long_read
        quals[1][13] = bytes([T.Q(35)]) * keep + bytes([T.Q(2)]) * (300 - keep)
        assert T.bounds_loop(quals[1][13], Q5, Q3) == (0, keep)
        paths = [str(tmp_path / f"long_{keep}_{m + 1}.fastq") for m in range(2)]
        for pth, r, q in zip(paths, reads, quals):
            open(pth, "wb").write(T.fastq_of(r, q))
        for extra in ([], ["--batch-reads", "6"]):
            out = str(tmp_path / "out.txt")
            p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + paths + ["--lineage", files["LineageFile.csv"], "--readlen", "auto", "--out", out, "--gidx",
                                                                           files["g.gidx"], "--trim-qual", f"{Q5},{Q3}"] + extra, capture_output=True, timeout=600)
            if ok:
                assert p.returncode == 0 and os.path.exists(out), p.stderr.decode()[-2000:]
                os.remove(out)
            else:
                assert p.returncode == 1 and "read set 1: read 13 holds 256 symbols" in p.stderr.decode(), p.stderr.decode()
                assert not [n for n in os.listdir(str(tmp_path)) if n.startswith("out.txt")]
