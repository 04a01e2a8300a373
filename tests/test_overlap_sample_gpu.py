"""A sample cut at its mates' overlap on the device (`LiME_fasta --trim-overlap`, lime_docs_trim_overlap_dev, lime_seq_reader_next_pair) against
the existing path fed with reads that were cut beforehand.  The first 120 pairs of the example (tests/golden/example_full.npz) are made
read-through pairs: the fragment is the first I symbols of the first mate, I seeded in 35 .. 140, the first mate reads it into the R1
adapter and the second mate reads its reverse complement into the R2 adapter, with about 3 % of the fragment's symbols changed; in a fifth
of the pairs I is 98 or 99, so that fewer than 3 adapter symbols are left in a read of 100.  The numpy model of the rule cuts them and the
result is written as a plain FASTQ pair.  The oracle is the existing program: `LiME_fasta --readlen auto` on the cut pair.
`LiME_fasta --readlen auto --trim-overlap 30` on the RAW pair must write the same classification file byte for byte -- whole and with
--batch-reads 7, from FASTQ and from FASTA, with one --gidx, two index shards and --refs -- and nothing else, and print the model's counts.
The comparison shows something only if the cut changes verdicts: the test asserts that more than a third of the pairs are cut, that the
classification differs from the flagless run's, that a read moves from U to a classified verdict, and that a cut pair is one that
--trim-adapter with the same adapters leaves unchanged."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import adapter_cases as A
from tests import overlap_cases as V
from tests.test_fasta_sample_gpu import ALPHA, BETA, BIN, ROOT, _example, _fasta, _to_dev

pytestmark = pytest.mark.gpu

PAIRS = 120
ADAPTERS = (V.TRUSEQ_R1, V.TRUSEQ_R2)
O, E = 30, 10


def _sample():
    """-> (raw mates, cut mates, the model's inserts, the model's info)"""
    _, sets, _, _ = _example()
    rng = np.random.default_rng([V.SEED, 20])
    r1, r2 = [], []
    for k, read in enumerate(sets["F1"][:PAIRS]):
        read = bytes(read)
        I = int(rng.integers(98, 100)) if k % 5 == 2 else int(rng.integers(35, 141))
        n = V.places(len(read), len(read), I)[1] - V.places(len(read), len(read), I)[0]
        a, b = V.plant(rng, read, I, ADAPTERS[0], ADAPTERS[1], int(rng.binomial(n, 0.03)))
        r1.append(a); r2.append(b)
    c1, c2, ins, info = V.cut_model(r1, r2, O, E)
    return (r1, r2), (c1, c2), ins, info


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import torch
    from lime_amd import api
    genomes, _, lineage, _ = _example()
    raw, cut, _, _ = _sample()
    d = str(tmp_path_factory.mktemp("sample_overlap"))
    names = ["refs.fasta", "LineageFile.csv", "g.gidx", "s0.gidx", "s1.gidx", "raw_1.fasta", "raw_2.fasta"] + [f"{k}_{m}.fastq" for k in ("raw", "cut") for m in (1, 2)]
    f = {k: os.path.join(d, k) for k in names}
    for m in range(2):
        open(f[f"raw_{m + 1}.fastq"], "wb").write(V.fastq_of(raw[m], eol=b"\r\n" if m else b"\n"))
        open(f[f"raw_{m + 1}.fasta"], "wb").write(V.fasta_of(raw[m]))
        open(f[f"cut_{m + 1}.fastq"], "wb").write(V.fastq_of(cut[m]))
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


OVERLAP_ARGS = ["--trim-overlap", str(O)]
LINE = r"^(\S+) \+ (\S+): overlap trim \(overlap (\d+), error (\d+)%\): (\d+) of (\d+) pairs with an overlap, (\d+) cut, (\d+) symbols before, (\d+) after\.$"


def _read(files, name):
    return open(os.path.join(files["dir"], name), "rb").read()


def test_the_generator_gives_the_comparison_something_to_show():
    raw, cut, ins, info = _sample()
    print("pairs cut", info["n_cut"], "with an overlap", info["n_overlap"], "of", PAIRS)
    assert 3 * info["n_cut"] > PAIRS                                          # more than a third of the pairs
    assert V.cut_model(raw[0], raw[1], O, E, insert=V.insert_masks) == (cut[0], cut[1], ins, info)
    assert all(len(r) == 100 for m in range(2) for r in raw[m])
    assert info["n_overlap"] > info["n_cut"]                                  # and some long fragments that overlap and are left whole
    # the short-remnant fifth: a pair that the model cuts and that the adapter trim with the kit's own adapters leaves unchanged
    by_adapter = [A.trim_model(raw[m], ADAPTERS[m], 3, 10)[0] for m in range(2)]
    missed = [k for k in range(PAIRS) if 0 < ins[k] < 100 and by_adapter[0][k] == raw[0][k] and by_adapter[1][k] == raw[1][k]]
    print("cut pairs that --trim-adapter leaves unchanged:", missed)
    assert len(missed) >= 1 and all(ins[k] in (98, 99) for k in missed)


def _check_line(files, p, fmt="fastq"):
    _, _, _, info = _sample()
    lines = re.findall(LINE, p.stdout.decode(), re.M)
    assert len(lines) == 1, p.stdout.decode()
    ln = lines[0]
    assert ln[0] == files[f"raw_1.{fmt}"] and ln[1] == files[f"raw_2.{fmt}"], ln
    assert [int(x) for x in ln[2:]] == [O, E, info["n_overlap"], info["n_pairs"], info["n_cut"], info["symbols_in"], info["symbols_out"]], ln
    assert b"numReads: %d" % PAIRS in p.stdout


@pytest.mark.parametrize("index", ["gidx", "two shards", "refs"])
def test_the_program_on_raw_reads_gives_the_precut_runs_file(files, index):
    ix = _index_args(files, index)
    tag = index.replace(" ", "_")
    p, new = _run(files, ("cut_1.fastq", "cut_2.fastq"), f"want_{tag}.txt", ix, [])           # the oracle: today's program on the cut pair
    assert p.returncode == 0 and new == {f"want_{tag}.txt"}, p.stderr.decode()[-2000:]
    want = _read(files, f"want_{tag}.txt")
    assert want.count(b"\n") >= PAIRS
    for extra in ([], ["--batch-reads", "7"]):
        out = f"got_{tag}_{len(extra)}.txt"
        p, new = _run(files, ("raw_1.fastq", "raw_2.fastq"), out, ix, OVERLAP_ARGS + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert _read(files, out) == want, (index, extra)
        assert new == {out}                                                  # nothing else is written
        _check_line(files, p)


def test_fasta_input_and_the_explicit_error_rate(files):
    ix = _index_args(files, "gidx")
    p, _ = _run(files, ("cut_1.fastq", "cut_2.fastq"), "want_fa.txt", ix, [])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    want = _read(files, "want_fa.txt")
    for k, extra in enumerate((OVERLAP_ARGS, OVERLAP_ARGS + ["--batch-reads", "7"], ["--trim-overlap", f"{O},{E}"])):
        p, new = _run(files, ("raw_1.fasta", "raw_2.fasta"), f"got_fa_{k}.txt", ix, extra)
        assert p.returncode == 0 and new == {f"got_fa_{k}.txt"}, p.stderr.decode()[-2000:]
        assert _read(files, f"got_fa_{k}.txt") == want
        _check_line(files, p, "fasta")


def test_the_cut_moves_reads_from_unclassified_to_classified(files):
    ix = _index_args(files, "gidx")
    p, _ = _run(files, ("raw_1.fastq", "raw_2.fastq"), "uncut.txt", ix, [])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    p, _ = _run(files, ("raw_1.fastq", "raw_2.fastq"), "cut.txt", ix, OVERLAP_ARGS)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    a, b = _read(files, "uncut.txt").split(b"\n"), _read(files, "cut.txt").split(b"\n")
    differ = sum(x != y for x, y in zip(a, b))
    u_to_c = sum(1 for x, y in zip(a, b) if x.startswith(b"U,") and y.startswith(b"C,"))
    print("lines on which the cut run differs from the flagless --readlen auto run of the raw files:", differ, "of", len(a), "; U -> C:", u_to_c)
    assert len(a) == len(b) and differ >= 1 and u_to_c >= 1


def test_through_the_library(files, tmp_path):
    import torch
    from lime_amd import api
    genomes, _, _, _ = _example()
    raw, cut, ins, info = _sample()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    tx = api.Taxonomy(files["LineageFile.csv"], 1, False, len(genomes))
    try:
        gi = ctx.load_genome_index(files["g.gidx"])
        fixed = [ctx.docs_from_arrays_dev(*_to_dev(cut[m])) for m in range(2)]
        want, w_counts, _ = ctx.classify_sample(fixed, gi, tx, ALPHA, api.NORM_PER_READ, BETA)
        whole = [ctx.docs_from_file(files[f"raw_{m + 1}.fastq"]) for m in range(2)]
        d1, d2, got_info, got_ins = ctx.docs_trim_overlap(whole[0], whole[1], O, E, want_insert=True)
        assert got_info == info and got_ins.tolist() == ins
        for d, f in zip((d1, d2), fixed):
            assert np.array_equal(d.get()[0], f.get()[0]) and np.array_equal(d.get()[1], f.get()[1])
        got, counts, _ = ctx.classify_sample([d1, d2], gi, tx, ALPHA, api.NORM_PER_READ, BETA)
        assert got.dtype.names == want.dtype.names and all(np.array_equal(got[k], want[k]) for k in want.dtype.names) and counts == w_counts
        readers = [ctx.seq_reader(files[f"raw_{m + 1}.fastq"]) for m in range(2)]
        readers[0].set_overlap(readers[1], O, E)
        streamed, s_counts, per_batch = ctx.classify_sample_stream(readers, gi, tx, ALPHA, api.NORM_PER_READ, BETA, 7)
        assert streamed.tobytes() == want.tobytes() and s_counts == w_counts and len(per_batch) == (PAIRS + 6) // 7
        assert readers[0].overlap_info() == info and readers[1].overlap_info() == info
        # a reader linked to one that is not in the call is refused, before any read
        lone = [ctx.seq_reader(files[f"raw_{m + 1}.fastq"]) for m in (0, 1, 1)]
        lone[0].set_overlap(lone[2], O, E)
        for rs in (lone[:2], lone[:1]):
            with pytest.raises(api.LimeError) as e:
                ctx.classify_sample_stream(rs, gi, tx, ALPHA, api.NORM_PER_READ, BETA, 7)
            assert "not in the call" in str(e.value)
        assert lone[0].info()["records"] == 0
        for x in fixed + whole + [d1, d2] + readers + lone:
            x.close()
        gi.close()
        # the Python mirror of the program
        want_file, out = str(tmp_path / "want.txt"), str(tmp_path / "got.txt")
        api.write_classification(want_file, want)
        pair = [files["raw_1.fastq"], files["raw_2.fastq"]]
        for kw in ({}, {"batch_reads": 7}):
            for ov in (O, (O, E), f"{O},{E}"):
                c = api.lime_fasta(pair, files["LineageFile.csv"], "auto", out, gidx=files["g.gidx"], ctx=ctx, trim_overlap=ov, **kw)
                assert c == w_counts and open(out, "rb").read() == open(want_file, "rb").read()
                os.remove(out)
        for bad in (dict(read_len=100, trim_overlap=30), dict(trim_overlap=0), dict(trim_overlap=(30, 51)), dict(trim_overlap=(30, 10, 1))):
            kw = dict(read_len="auto"); kw.update(bad)
            with pytest.raises(ValueError):
                api.lime_fasta(pair, files["LineageFile.csv"], kw.pop("read_len"), out, gidx=files["g.gidx"], ctx=ctx, **kw)
        with pytest.raises(ValueError):
            api.lime_fasta(pair[:1], files["LineageFile.csv"], "auto", out, gidx=files["g.gidx"], ctx=ctx, trim_overlap=30)
        assert not os.path.exists(out)
    finally:
        tx.close()
        ctx.close()
