"""A sample classified against a genome database cut into index shards (lime_classify_sample_shards_dev, lime_classify_sample_stream_shards,
BuildIndex --refs --shard-positions, LiME_fasta with --gidx given several times, api.lime_fasta(gidx=[...])).
(a) the example at full size (tests/golden/example_full.npz, 3 genomes, 10 000 pairs) through the programs: the classification file must
    be the reference's own Classify output byte for byte for the shards 2 + 1 and 1 + 1 + 1 that BuildIndex cuts at budgets computed
    with the plan from the genomes' lengths, and for 1 + 2, with and without --batch-reads 4096.  The example's genomes are equally
    long, and with equal lengths no budget makes the greedy plan cut 1 + 2 (a budget that holds genomes 1 and 2 holds 0 and 1): those
    two shards are saved from the library instead and go through LiME_fasta like the others;
(b) on the first 50 pairs: the verdicts of classify_sample_shards are classify_sample's with the one index, in every field, single-end and
    paired, with and without ebwt, lcp_cap 0 and 20; one shard is today's call, stats included; the refusals."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_fasta_sample_gpu import ALPHA, BETA, BIN, NORM, READ_LEN, ROOT, _example, _fasta, _to_dev

pytestmark = pytest.mark.gpu

HEAD = 50


def _budget_for(lengths, want):
    """the smallest budget at which the plan cuts `want`, among the sums of consecutive genomes' positions"""
    from lime_amd import api
    off = np.concatenate([[0], np.cumsum(lengths)])
    pos = [n + 1 for n in lengths]
    sums = sorted({sum(pos[a:b]) for a in range(len(pos)) for b in range(a + 1, len(pos) + 1)})
    for budget in sums:
        if budget >= max(pos) and api.gindex_shard_plan(off, budget) == want:
            return budget
    return None


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the mates, the genomes in 60-column lines, the lineage, and the index shards: 2 + 1 and 1 + 1 + 1 from BuildIndex, 1 + 2 from the library"""
    import torch
    from lime_amd import api
    genomes, sets, lineage, _ = _example()
    d = str(tmp_path_factory.mktemp("sample_shards"))
    f = {k: os.path.join(d, k) for k in ("reads_1.fasta", "reads_2.fasta", "refs.fasta", "LineageFile.csv")}
    open(f["reads_1.fasta"], "wb").write(_fasta(sets["F1"]))
    open(f["reads_2.fasta"], "wb").write(_fasta(sets["F2"], eol=b"\r\n"))
    open(f["refs.fasta"], "wb").write(_fasta(genomes, width=60))
    open(f["LineageFile.csv"], "wb").write(lineage)
    for exe in ("LiME_fasta", "BuildIndex"):
        if not os.path.exists(os.path.join(BIN, exe)):
            subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    lengths = [len(g) for g in genomes]
    assert len(genomes) == 3 and _budget_for(lengths, [0, 1, 3]) is None          # (equal lengths: see the head of the file)
    f["shards"] = {}
    for name, want in (("2+1", [0, 2, 3]), ("1+1+1", [0, 1, 2, 3])):
        budget = _budget_for(lengths, want)
        assert budget is not None, name
        base = os.path.join(d, "s" + str(len(want) - 1))
        p = subprocess.run([os.path.join(BIN, "BuildIndex"), "--refs", f["refs.fasta"], base, "--shard-positions", str(budget)], capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        out = p.stdout.decode()
        names = [f"{base}.{s:03d}.gidx" for s in range(len(want) - 1)]
        assert f"numGenomes: 3\n" in out and f"shards: {len(want) - 1}\n" in out, out
        for s, n in enumerate(names):
            cnt = want[s + 1] - want[s]
            assert f"{n}: {cnt} genomes, {sum(lengths[want[s]:want[s + 1]]) + cnt} positions\n" in out, out
            assert api.gindex_probe(n)["n_docs"] == cnt
        assert not os.path.exists(f"{base}.{len(names):03d}.gidx") and not os.path.exists(base + ".gidx")
        f["shards"][name] = names
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    names = [os.path.join(d, "lib.0.gidx"), os.path.join(d, "lib.1.gidx")]
    for n, part in zip(names, (genomes[:1], genomes[1:])):
        gi = ctx.build_genome_index(part)
        gi.save(n)
        gi.close()
    ctx.close()
    f["shards"]["1+2"] = names
    f["dir"] = d
    return f


@pytest.mark.parametrize("batched", [False, True], ids=["whole", "batch-reads 4096"])
@pytest.mark.parametrize("cut", ["1+2", "2+1", "1+1+1"])
def test_lime_fasta_over_index_shards_gives_the_references_classification(files, cut, batched):
    _, sets, _, want = _example()
    out = os.path.join(files["dir"], f"classification_{cut}_{int(batched)}.txt")
    args = [files["reads_1.fasta"], files["reads_2.fasta"], "--lineage", files["LineageFile.csv"], "--readlen", str(READ_LEN), "--out", out]
    for n in files["shards"][cut]:
        args += ["--gidx", n]
    if batched:
        args += ["--batch-reads", "4096"]
    before = set(os.listdir(files["dir"]))
    p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=600, cwd=files["dir"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert open(out, "rb").read() == want
    assert set(os.listdir(files["dir"])) - before == {os.path.basename(out)}           # nothing else is written
    assert b"numGenomes: 3\n" in p.stdout and b"numReads: %d" % len(sets["F1"]) in p.stdout
    assert p.stdout.count(b" shards, maximum length ") == 4 and b"Number of successfully classified reads" in p.stdout


def test_the_python_mirror(files, tmp_path):
    from lime_amd import api
    _, _, _, want = _example()
    for k, kw in enumerate((dict(), dict(batch_reads=3000))):
        out = str(tmp_path / f"classification_{k}.txt")
        counts = api.lime_fasta([files["reads_1.fasta"], files["reads_2.fasta"]], files["LineageFile.csv"], READ_LEN, out, gidx=files["shards"]["1+1+1"], **kw)
        assert open(out, "rb").read() == want and sum(counts) == 10_000


@pytest.fixture(scope="module")
def small(files):
    """the first 50 pairs, the genomes' one index and their shards (built with lcp_cap 0) and the taxonomy on one context"""
    import torch
    from lime_amd import api
    genomes, sets, _, _ = _example()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    gi = ctx.build_genome_index(genomes)
    shards = {"1+2": [ctx.build_genome_index(genomes[:1]), ctx.build_genome_index(genomes[1:])],
              "1+1+1": [ctx.build_genome_index([g]) for g in genomes]}
    tx = api.Taxonomy(files["LineageFile.csv"], 1, False, len(genomes))
    mates = [ctx.docs_from_arrays_dev(*_to_dev(sets[k][:HEAD])) for k in ("F1", "F2")]
    yield ctx, gi, shards, tx, mates
    tx.close()
    ctx.close()


@pytest.mark.parametrize("lcp_cap", [0, 20])
@pytest.mark.parametrize("ebwt", [True, False], ids=["ebwt", "no ebwt"])
@pytest.mark.parametrize("paired", [False, True], ids=["single-end", "paired"])
def test_the_verdicts_are_the_one_indexs(small, paired, ebwt, lcp_cap):
    ctx, gi, shards, tx, mates = small
    m = mates if paired else mates[:1]
    want_v, want_counts, want_stats = ctx.classify_sample(m, gi, tx, ALPHA, NORM, BETA, ebwt=ebwt, lcp_cap=lcp_cap)
    assert sum(want_counts) == HEAD and want_counts[0] > 0
    for name, sh in shards.items():
        v, counts, stats = ctx.classify_sample_shards(m, sh, tx, ALPHA, NORM, BETA, ebwt=ebwt, lcp_cap=lcp_cap)
        assert v.tobytes() == want_v.tobytes() and counts == want_counts, name
        assert len(stats) == len(sh) * 2 * len(m) and want_stats[0].n_clusters > 0, name
        for k in range(2 * len(m)):                      # per-shard figures: a cluster with genomes of two shards counts twice
            assert sum(stats[s * 2 * len(m) + k].n_clusters for s in range(len(sh))) >= want_stats[k].n_clusters, (name, k)


def test_one_shard_is_todays_call(small):
    ctx, gi, _, tx, mates = small
    want_v, want_counts, want_stats = ctx.classify_sample(mates, gi, tx, ALPHA, NORM, BETA)
    v, counts, stats = ctx.classify_sample_shards(mates, [gi], tx, ALPHA, NORM, BETA)
    assert v.tobytes() == want_v.tobytes() and counts == want_counts and len(stats) == len(want_stats) == 4
    assert [bytes(s) for s in stats] == [bytes(s) for s in want_stats]


def test_refusals(small, files):
    import sys
    from lime_amd import _lib, api
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_classify as M
    ctx, gi, shards, tx, mates = small
    genomes = _example()[0]
    two = os.path.join(files["dir"], "two.csv")
    open(two, "wb").write(M.taxonomy(2, np.random.default_rng(3), False))
    tx2 = api.Taxonomy(two, 1, False, 2)
    capped = ctx.build_genome_index(genomes[1:], 0, 20)
    ctx2 = api.Context(0)
    foreign = ctx2.build_genome_index(genomes[1:])
    a = shards["1+2"]
    bad = {"shards built with different caps": dict(sh=[a[0], capped], text="lcp_cap 20"),
           "a lineage of 2 genomes": dict(tx=tx2, text="taxonomy holds 2 genomes"),
           "a lineage of 3 genomes for 2": dict(sh=a[1:], text="taxonomy holds 3 genomes"),
           "no shard": dict(sh=[], text="n_shards is 0"),
           "a NULL shard": dict(sh=[a[0], None], text="shard 1 is NULL"),
           "a shard of another context": dict(sh=[a[0], foreign], text="shard 1 belongs to another context"),
           "a cap below alpha": dict(lcp_cap=ALPHA - 1, text="alpha")}
    for name, kw in bad.items():
        with pytest.raises(api.LimeError) as e:
            ctx.classify_sample_shards(mates, kw.get("sh", a), kw.get("tx", tx), ALPHA, NORM, BETA, lcp_cap=kw.get("lcp_cap", 0))
        assert e.value.code == _lib.ERR_ARG and kw["text"] in str(e.value), (name, e.value)
    tx2.close(); capped.close()
    ctx2.close()
