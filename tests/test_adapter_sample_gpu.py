"""A sample cut at its adapters on the device (`LiME_fasta --trim-adapter`, lime_docs_trim_adapter_dev, lime_seq_reader_set_adapter) against
the existing path fed with reads that were trimmed beforehand.  The first 120 pairs of the example (tests/golden/example_full.npz) get
read-through planted: every read's insert is cut at a seeded length in 20 .. 100 and a TruSeq-like adapter (R1's for the first mates, R2's
for the second) with about 5 % of its symbols changed, then filler, follows up to 100 symbols.  The numpy model of the rule trims them and
the result is written as a plain FASTQ pair.  The oracle is the existing program: `LiME_fasta --readlen auto` on the trimmed pair.
`LiME_fasta --readlen auto --trim-adapter A1,A2` on the RAW pair must write the same classification file byte for byte -- whole and with
--batch-reads 7, with one --gidx, two index shards and --refs, from FASTQ and from FASTA, and with --trim-qual in front -- and nothing else,
and print the model's counts.  The comparison shows something only if the trim changes verdicts: the test asserts that it changes more
than half of the reads, that the classification differs from the untrimmed run's and that a read moves from U to a classified verdict."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import adapter_cases as A
from tests import trim_cases as T
from tests.test_fasta_sample_gpu import ALPHA, BETA, BIN, ROOT, _example, _fasta, _to_dev

pytestmark = pytest.mark.gpu

PAIRS = 120
ADAPTERS = (A.TRUSEQ_R1, A.TRUSEQ_R2)
O, E = 3, 10
Q5, Q3 = 20, 20


def _sample():
    """-> (raw reads per mate, trimmed reads per mate, the model's info per mate)"""
    _, sets, _, _ = _example()
    rng = np.random.default_rng([A.SEED, 20])
    raw = []
    for m, k in enumerate(("F1", "F2")):
        raw.append([A.plant(rng, bytes(r), int(rng.integers(20, 101)), ADAPTERS[m], int(rng.binomial(len(ADAPTERS[m]), 0.05))) for r in sets[k][:PAIRS]])
    trimmed, infos = zip(*[A.trim_model(raw[m], ADAPTERS[m], O, E) for m in range(2)])
    return raw, list(trimmed), list(infos)


def _quals():
    raw, _, _ = _sample()
    return [T.sample_quals_for(raw[0], seed=17), T.sample_quals_for(raw[1], seed=18)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    import torch
    from lime_amd import api
    genomes, _, lineage, _ = _example()
    raw, trimmed, _ = _sample()
    quals = _quals()
    both = [A.trim_model(T.trim_model(raw[m], quals[m], Q5, Q3)[0], ADAPTERS[m], O, E)[0] for m in range(2)]
    d = str(tmp_path_factory.mktemp("sample_adapter"))
    names = ["refs.fasta", "LineageFile.csv", "g.gidx", "s0.gidx", "s1.gidx", "raw_1.fasta", "raw_2.fasta"] + [f"{k}_{m}.fastq" for k in ("raw", "cut", "rawq", "cutq") for m in (1, 2)]
    f = {k: os.path.join(d, k) for k in names}
    for m in range(2):
        open(f[f"raw_{m + 1}.fastq"], "wb").write(A.fastq_of(raw[m], eol=b"\r\n" if m else b"\n"))
        open(f[f"raw_{m + 1}.fasta"], "wb").write(A.fasta_of(raw[m]))
        open(f[f"cut_{m + 1}.fastq"], "wb").write(A.fastq_of(trimmed[m]))
        open(f[f"rawq_{m + 1}.fastq"], "wb").write(A.fastq_of(raw[m], quals[m]))
        open(f[f"cutq_{m + 1}.fastq"], "wb").write(A.fastq_of(both[m]))
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


ADAPTER_ARGS = ["--trim-adapter", (ADAPTERS[0] + b"," + ADAPTERS[1]).decode()]
LINE = r"^(\S+): adapter trim (\S+) \(overlap (\d+), error (\d+)%\): (\d+) of (\d+) reads changed, (\d+) emptied, (\d+) symbols before, (\d+) after\.$"


def _read(files, name):
    return open(os.path.join(files["dir"], name), "rb").read()


def test_the_generator_gives_the_comparison_something_to_show():
    raw, trimmed, infos = _sample()
    changed = infos[0]["n_changed"] + infos[1]["n_changed"]
    lengths = {len(r) for m in range(2) for r in trimmed[m]}
    print("reads changed", changed, "of", 2 * PAIRS, "distinct lengths", len(lengths))
    assert changed > PAIRS                                                   # more than half of the reads
    assert len(lengths) >= 30
    for m in range(2):
        assert A.trim_model(raw[m], ADAPTERS[m], O, E, keep=A.keep_masks)[0] == trimmed[m]
        assert all(len(r) == 100 for r in raw[m])
    assert A.trim_model(raw[1], ADAPTERS[0], O, E)[0] != trimmed[1]          # the second adapter is no polish: R1's cuts the second mates elsewhere


@pytest.mark.parametrize("index", ["gidx", "two shards", "refs"])
def test_the_program_on_raw_reads_gives_the_pretrimmed_runs_file(files, index):
    _, _, infos = _sample()
    ix = _index_args(files, index)
    tag = index.replace(" ", "_")
    p, new = _run(files, ("cut_1.fastq", "cut_2.fastq"), f"want_{tag}.txt", ix, [])           # the oracle: today's program on the trimmed pair
    assert p.returncode == 0 and new == {f"want_{tag}.txt"}, p.stderr.decode()[-2000:]
    want = _read(files, f"want_{tag}.txt")
    assert want.count(b"\n") >= PAIRS
    for extra in ([], ["--batch-reads", "7"]):
        out = f"got_{tag}_{len(extra)}.txt"
        p, new = _run(files, ("raw_1.fastq", "raw_2.fastq"), out, ix, ADAPTER_ARGS + extra)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert _read(files, out) == want, (index, extra)
        assert new == {out}                                                  # nothing else is written
        lines = re.findall(LINE, p.stdout.decode(), re.M)
        assert len(lines) == 2, p.stdout.decode()
        for m, ln in enumerate(lines):
            i = infos[m]
            assert ln[0] == files[f"raw_{m + 1}.fastq"] and ln[1] == ADAPTERS[m].decode(), ln
            assert [int(x) for x in ln[2:]] == [O, E, i["n_changed"], i["n_reads"], i["n_empty"], i["symbols_in"], i["symbols_out"]], ln
        assert b"numReads: %d" % PAIRS in p.stdout


def test_the_trim_moves_reads_from_unclassified_to_classified(files):
    ix = _index_args(files, "gidx")
    p, _ = _run(files, ("raw_1.fastq", "raw_2.fastq"), "untrimmed.txt", ix, [])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    p, _ = _run(files, ("raw_1.fastq", "raw_2.fastq"), "trimmed.txt", ix, ADAPTER_ARGS)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    a, b = _read(files, "untrimmed.txt").split(b"\n"), _read(files, "trimmed.txt").split(b"\n")
    differ = sum(x != y for x, y in zip(a, b))
    u_to_c = sum(1 for x, y in zip(a, b) if x.startswith(b"U,") and y.startswith(b"C,"))
    print("lines on which the trimmed run differs from the untrimmed --readlen auto run of the raw files:", differ, "of", len(a), "; U -> C:", u_to_c)
    assert len(a) == len(b) and differ >= 1 and u_to_c >= 1


def test_fasta_input_explicit_defaults_and_one_adapter_for_both_mates(files):
    ix = _index_args(files, "gidx")
    p, _ = _run(files, ("cut_1.fastq", "cut_2.fastq"), "want_fa.txt", ix, [])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    want = _read(files, "want_fa.txt")
    for k, extra in enumerate(([], ["--batch-reads", "7"], ["--adapter-overlap", str(O), "--adapter-error", str(E)])):
        p, new = _run(files, ("raw_1.fasta", "raw_2.fasta"), f"got_fa_{k}.txt", ix, ADAPTER_ARGS + extra)
        assert p.returncode == 0 and new == {f"got_fa_{k}.txt"}, p.stderr.decode()[-2000:]
        assert _read(files, f"got_fa_{k}.txt") == want and len(re.findall(LINE, p.stdout.decode(), re.M)) == 2
    # one SEQ serves every mate: the first mates alone, and the pair of first mates twice
    raw, _, infos = _sample()
    p, _ = _run(files, ("raw_1.fastq", "raw_1.fasta"), "one.txt", ix, ["--trim-adapter", ADAPTERS[0].decode()])
    q, _ = _run(files, ("cut_1.fastq", "cut_1.fastq"), "one_want.txt", ix, [])
    assert p.returncode == 0 and q.returncode == 0, p.stderr.decode()[-2000:]
    assert _read(files, "one.txt") == _read(files, "one_want.txt")
    lines = re.findall(LINE, p.stdout.decode(), re.M)
    assert [ln[1] for ln in lines] == [ADAPTERS[0].decode()] * 2 and [int(ln[4]) for ln in lines] == [infos[0]["n_changed"]] * 2


def test_quality_trim_first_adapter_trim_second(files):
    raw, _, _ = _sample()
    quals = _quals()
    ix = _index_args(files, "gidx")
    p, _ = _run(files, ("cutq_1.fastq", "cutq_2.fastq"), "want_q.txt", ix, [])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    for k, extra in enumerate(([], ["--batch-reads", "7"])):
        p, new = _run(files, ("rawq_1.fastq", "rawq_2.fastq"), f"got_q_{k}.txt", ix, ADAPTER_ARGS + ["--trim-qual", f"{Q5},{Q3}"] + extra)
        assert p.returncode == 0 and new == {f"got_q_{k}.txt"}, p.stderr.decode()[-2000:]
        assert _read(files, f"got_q_{k}.txt") == _read(files, "want_q.txt")
        out = p.stdout.decode()
        assert out.count("quality trim") == 2 and len(re.findall(LINE, out, re.M)) == 2
        for m, ln in enumerate(re.findall(LINE, out, re.M)):
            q_reads, q_info = T.trim_model(raw[m], quals[m], Q5, Q3)
            i = A.trim_model(q_reads, ADAPTERS[m], O, E)[1]
            assert [int(x) for x in ln[4:]] == [i["n_changed"], i["n_reads"], i["n_empty"], q_info["symbols_out"], i["symbols_out"]], ln


def test_through_the_library(files, tmp_path):
    import torch
    from lime_amd import api
    genomes, _, _, _ = _example()
    raw, trimmed, infos = _sample()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    tx = api.Taxonomy(files["LineageFile.csv"], 1, False, len(genomes))
    try:
        gi = ctx.load_genome_index(files["g.gidx"])
        fixed = [ctx.docs_from_arrays_dev(*_to_dev(trimmed[m])) for m in range(2)]
        want, w_counts, _ = ctx.classify_sample(fixed, gi, tx, ALPHA, api.NORM_PER_READ, BETA)
        mates = []
        for m in range(2):
            d = ctx.docs_from_file(files[f"raw_{m + 1}.fastq"])
            t, info = ctx.docs_trim_adapter(d, ADAPTERS[m], O, E)
            assert info == infos[m]
            assert np.array_equal(t.get()[0], fixed[m].get()[0]) and np.array_equal(t.get()[1], fixed[m].get()[1])
            mates.append(t)
            d.close()
        got, counts, _ = ctx.classify_sample(mates, gi, tx, ALPHA, api.NORM_PER_READ, BETA)
        assert got.dtype.names == want.dtype.names and all(np.array_equal(got[k], want[k]) for k in want.dtype.names) and counts == w_counts
        readers = [ctx.seq_reader(files[f"raw_{m + 1}.fastq"]) for m in range(2)]
        for m, r in enumerate(readers):
            r.set_adapter(ADAPTERS[m], O, E)
        streamed, s_counts, per_batch = ctx.classify_sample_stream(readers, gi, tx, ALPHA, api.NORM_PER_READ, BETA, 7)
        assert streamed.tobytes() == want.tobytes() and s_counts == w_counts and len(per_batch) == (PAIRS + 6) // 7
        assert [r.adapter_info() for r in readers] == infos
        for x in fixed + mates + readers:
            x.close()
        gi.close()
        # the Python mirror of the program
        want_file, out = str(tmp_path / "want.txt"), str(tmp_path / "got.txt")
        api.write_classification(want_file, want)
        pair = [files["raw_1.fastq"], files["raw_2.fastq"]]
        for kw in ({}, {"batch_reads": 7}, {"adapter_overlap": O, "adapter_error": E}):
            for ad in (ADAPTERS, (ADAPTERS[0] + b"," + ADAPTERS[1]).decode()):
                c = api.lime_fasta(pair, files["LineageFile.csv"], "auto", out, gidx=files["g.gidx"], ctx=ctx, trim_adapter=ad, **kw)
                assert c == w_counts and open(out, "rb").read() == open(want_file, "rb").read()
                os.remove(out)
        for bad in (dict(read_len=100, trim_adapter="ACGT"), dict(trim_adapter="ACGN"), dict(trim_adapter="A" * 65), dict(trim_adapter="ACGT", adapter_overlap=5),
                    dict(trim_adapter="ACGT", adapter_error=51), dict(trim_adapter=("ACGT", "ACGT", "ACGT"))):
            kw = dict(read_len="auto"); kw.update(bad)
            with pytest.raises(ValueError):
                api.lime_fasta(pair, files["LineageFile.csv"], kw.pop("read_len"), out, gidx=files["g.gidx"], ctx=ctx, **kw)
        with pytest.raises(ValueError):
            api.lime_fasta(pair[:1], files["LineageFile.csv"], "auto", out, gidx=files["g.gidx"], ctx=ctx, trim_adapter="ACGT,ACGT")
        assert not os.path.exists(out)
    finally:
        tx.close()
        ctx.close()


def test_a_pair_with_one_mate_emptied_by_the_adapter(files, tmp_path):
    """read 5 of the first mates IS the adapter and what follows it: an empty read in its place, its pair classified by the other mate alone"""
    raw, trimmed, _ = _sample()
    rng = np.random.default_rng([A.SEED, 21])
    reads = [list(raw[0][:20]), list(raw[1][:20])]
    cut = [list(trimmed[0][:20]), list(trimmed[1][:20])]
    reads[0][5] = (ADAPTERS[0] + A.bases(rng, 100))[:100]
    cut[0][5] = b""
    assert A.keep_loop(reads[0][5], ADAPTERS[0], O, E) == 0
    paths = {k: [str(tmp_path / f"{k}_{m + 1}.fastq") for m in range(2)] for k in ("raw", "cut")}
    for m in range(2):
        open(paths["raw"][m], "wb").write(A.fastq_of(reads[m]))
        open(paths["cut"][m], "wb").write(A.fastq_of(cut[m]))
    base = ["--lineage", files["LineageFile.csv"], "--readlen", "auto", "--gidx", files["g.gidx"]]
    want = str(tmp_path / "want.txt")
    p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + paths["cut"] + base + ["--out", want], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    for extra in ([], ["--batch-reads", "6"]):
        out = str(tmp_path / "out.txt")
        p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + paths["raw"] + base + ["--out", out] + ADAPTER_ARGS + extra, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert open(out, "rb").read() == open(want, "rb").read()
        first = re.findall(LINE, p.stdout.decode(), re.M)[0]
        assert int(first[6]) == 1 and int(first[5]) == 20                   # one read emptied, of 20
        os.remove(out)


def test_the_255_symbol_limit_holds_for_the_trimmed_length(files, tmp_path):
    """a raw read of 300 symbols cut to 240 by its adapter passes; one whose trimmed length is 256 is refused as an untrimmed one of 256 is, with
    the read set and the read's index"""
    raw, _, _ = _sample()
    rng = np.random.default_rng([A.SEED, 22])
    reads = [list(raw[0][:20]), list(raw[1][:20])]
    body = A.far_from(rng, 300, ADAPTERS[1], O, E)
    for keep, ok in ((240, True), (256, False)):
        reads[1][13] = (body[:keep] + ADAPTERS[1] + body)[:300]
        assert A.keep_loop(reads[1][13], ADAPTERS[1], O, E) == keep
        paths = [str(tmp_path / f"long_{keep}_{m + 1}.fastq") for m in range(2)]
        for pth, r in zip(paths, reads):
            open(pth, "wb").write(A.fastq_of(r))
        for extra in ([], ["--batch-reads", "6"]):
            out = str(tmp_path / "out.txt")
            p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + paths + ["--lineage", files["LineageFile.csv"], "--readlen", "auto", "--out", out, "--gidx",
                                                                           files["g.gidx"]] + ADAPTER_ARGS + extra, capture_output=True, timeout=600)
            if ok:
                assert p.returncode == 0 and os.path.exists(out), p.stderr.decode()[-2000:]
                os.remove(out)
            else:
                assert p.returncode == 1 and "read set 1: read 13 holds 256 symbols" in p.stderr.decode(), p.stderr.decode()
                assert not [n for n in os.listdir(str(tmp_path)) if n.startswith("out.txt")]
