"""One sample from FASTA bytes to verdicts on the device: bin/LiME_fasta, api.lime_fasta and Context.classify_sample.
(a) the example at full size (tests/golden/example_full.npz): the classification file must be the reference's own Classify output for these
    collections, byte for byte -- from --refs, from --gidx after BuildIndex --refs, and with --trlcp 16 / 20 (a cap >= alpha changes nothing);
(b) single-end on 300 of those reads: the verdicts of lime_classify_lists_dev over the two lists the existing calls make;
(c) the refusals of lime_classify_sample_dev: LIME_ERR_ARG with a text, nothing left allocated."""
import functools
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

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
        if width:
            out.extend(d[o:o + width] + eol for o in range(0, len(d), width))
        else:
            out.append(d + eol)
    return b"".join(out)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """reads_1 with LF, reads_2 with CRLF, the genomes in 60-column lines, the lineage, and the genome index BuildIndex --refs writes"""
    genomes, sets, lineage, _ = _example()
    d = str(tmp_path_factory.mktemp("sample"))
    f = {k: os.path.join(d, k) for k in ("reads_1.fasta", "reads_2.fasta", "refs.fasta", "LineageFile.csv", "g.gidx", "g20.gidx")}
    open(f["reads_1.fasta"], "wb").write(_fasta(sets["F1"]))
    open(f["reads_2.fasta"], "wb").write(_fasta(sets["F2"], eol=b"\r\n"))
    open(f["refs.fasta"], "wb").write(_fasta(genomes, width=60))
    open(f["LineageFile.csv"], "wb").write(lineage)
    for exe in ("LiME_fasta", "BuildIndex"):
        if not os.path.exists(os.path.join(BIN, exe)):
            subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    for base, flags in (("g", []), ("g20", ["--trlcp", "20"])):
        p = subprocess.run([os.path.join(BIN, "BuildIndex"), "--refs", f["refs.fasta"], os.path.join(d, base)] + flags, capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
    f["dir"] = d
    return f


@pytest.mark.parametrize("form", ["refs", "gidx", "refs trlcp 16", "gidx trlcp 20", "gidx20", "gidx20 trlcp 16"])
def test_lime_fasta_gives_the_references_classification(files, form):
    _, sets, _, want = _example()
    out = os.path.join(files["dir"], "classification_" + form.replace(" ", "_") + ".txt")
    args = [files["reads_1.fasta"], files["reads_2.fasta"], "--lineage", files["LineageFile.csv"], "--readlen", str(READ_LEN), "--out", out]
    args += {"refs": ["--refs", files["refs.fasta"]], "gidx": ["--gidx", files["g.gidx"]], "gidx20": ["--gidx", files["g20.gidx"]]}[form.split()[0]]
    if "trlcp" in form:
        args += ["--trlcp", form.split()[-1]]
    before = set(os.listdir(files["dir"]))
    p = subprocess.run([os.path.join(BIN, "LiME_fasta")] + args, capture_output=True, timeout=600, cwd=files["dir"])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert open(out, "rb").read() == want
    assert set(os.listdir(files["dir"])) - before == {os.path.basename(out)}           # nothing else is written
    assert b"numReads: %d\nnumGenomes: 3\n" % len(sets["F1"]) in p.stdout
    assert p.stdout.count(b" clusters, maximum length ") == 4 and b"Number of successfully classified reads" in p.stdout


def test_lime_fasta_refusals(files):
    run = lambda extra: subprocess.run([os.path.join(BIN, "LiME_fasta"), files["reads_1.fasta"], "--lineage", files["LineageFile.csv"], "--readlen", "100",
                                        "--out", os.path.join(files["dir"], "no.txt")] + extra, capture_output=True, timeout=600)
    p = run(["--gidx", files["g20.gidx"], "--trlcp", "21"])                  # an index built with --trlcp 20 cannot serve 21
    assert p.returncode == 1 and b"20" in p.stderr and b"21" in p.stderr
    p = run(["--gidx", files["g20.gidx"], "--alpha", "21"])                  # nor clusters of alpha 21
    assert p.returncode == 1 and b"alpha" in p.stderr
    p = run(["--refs", os.path.join(files["dir"], "no_such.fasta")])
    assert p.returncode != 0 and b"Error reading" in p.stderr
    assert not os.path.exists(os.path.join(files["dir"], "no.txt"))


def _to_dev(docs):
    import torch
    from lime_amd import api
    text, off = api.pack_documents(docs, [])
    return torch.from_numpy(text.copy()).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), len(docs), int(off[-1])


def _lists_the_old_way(ctx, gi, docs, n_refs, ebwt=True):
    """merge_index_dev + fused_choose_lists_dev on one collection -> (Lists, Stats)"""
    t, o, nd, nt = _to_dev(docs)
    e, l, d = ctx.merge_index_dev(t, o, nd, nt, gi)
    return ctx.fused_choose_lists_dev(l, d, e if ebwt else None, len(l), nd, n_refs, ALPHA, NORM, BETA)


def test_classify_sample_and_the_python_mirror(files, tmp_path):
    import torch
    from lime_amd import api
    genomes, sets, _, want = _example()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    try:
        mates = [ctx.docs_from_fasta(files["reads_1.fasta"]), ctx.docs_from_fasta(files["reads_2.fasta"])]
        gi = ctx.load_genome_index(files["g.gidx"])
        tx = api.Taxonomy(files["LineageFile.csv"], 1, False, len(genomes))
        v, counts, stats = ctx.classify_sample(mates, gi, tx, ALPHA, NORM, BETA)
        out = str(tmp_path / "classification.txt")
        api.write_classification(out, v)
        assert open(out, "rb").read() == want
        assert sum(counts) == len(v) == len(sets["F1"]) and [int((v["type"] == ord(t)).sum()) for t in "CUAH"] == counts
        for k, name in enumerate(("F1", "F1RC", "F2", "F2RC")):
            li, s = _lists_the_old_way(ctx, gi, sets[name], len(genomes))
            li.close()
            assert (stats[k].n_clusters, stats[k].max_len) == (s.n_clusters, s.max_len) and s.n_clusters > 0, name
        tx.close()
    finally:
        ctx.close()
    out2 = str(tmp_path / "classification_py.txt")
    counts2 = api.lime_fasta([files["reads_1.fasta"], files["reads_2.fasta"]], files["LineageFile.csv"], READ_LEN, out2, refs=files["refs.fasta"])
    assert open(out2, "rb").read() == want and counts2 == counts


@pytest.fixture(scope="module")
def small():
    """300 of the example's pairs, the genomes' index and the taxonomy on one context"""
    import torch
    from lime_amd import api
    genomes, sets, lineage, _ = _example()
    torch.cuda.set_device(0)
    ctx = api.Context(0)
    pick = list(range(0, 10_000, 33))[:300]
    f1, f1rc = [sets["F1"][i] for i in pick], [sets["F1RC"][i] for i in pick]
    gi = ctx.build_genome_index(genomes)
    yield ctx, gi, f1, f1rc, len(genomes)
    ctx.close()


@pytest.mark.parametrize("ebwt", [True, False])
@pytest.mark.parametrize("binary", [True, False])
def test_single_end_matches_the_existing_calls(small, files, ebwt, binary):
    from lime_amd import api
    ctx, gi, f1, f1rc, n_refs = small
    tx = api.Taxonomy(files["LineageFile.csv"], 1, False, n_refs)
    lists = [_lists_the_old_way(ctx, gi, docs, n_refs, ebwt)[0] for docs in (f1, f1rc)]
    want_v, want_counts = ctx.classify_lists_dev(lists, n_refs, tx, binary)
    for li in lists:
        li.close()
    mate = ctx.docs_from_arrays_dev(*_to_dev(f1))
    v, counts, stats = ctx.classify_sample([mate], gi, tx, ALPHA, NORM, BETA, ebwt=ebwt, binary=binary)
    mate.close(); tx.close()
    assert len(stats) == 2 and counts == want_counts and sum(counts) == 300 and counts[0] > 0
    assert v.tobytes() == want_v.tobytes()


def _free_bytes():
    import torch
    from lime_amd import api
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


def test_classify_sample_refusals(small, files):
    from lime_amd import _lib, api
    ctx, gi, f1, f1rc, n_refs = small
    tx = api.Taxonomy(files["LineageFile.csv"], 1, False, n_refs)
    # a lineage of four genomes
    import make_golden_classify as M
    other = os.path.join(files["dir"], "four.csv")
    open(other, "wb").write(M.taxonomy(n_refs + 1, np.random.default_rng(3), False))
    tx2 = api.Taxonomy(other, 1, False, n_refs + 1)
    gi16 = ctx.build_genome_index([b"ACGTACGTACGTACGTACGTAAA"] * n_refs, 0, 16)
    a, b = ctx.docs_from_arrays_dev(*_to_dev(f1)), ctx.docs_from_arrays_dev(*_to_dev(f1[:299]))
    empty = ctx.docs_from_bytes(b"no header at all\n")
    assert empty.info() == (0, 0)
    ctx.classify_sample([b], gi, tx, ALPHA, NORM, BETA)                       # a whole call first: what the runtime allocates on first launches
    before = _free_bytes()
    bad = {"three read sets": dict(mates=[a, a, a]), "no read set": dict(mates=[]), "different document counts": dict(mates=[a, b]),
           "a read set without documents": dict(mates=[empty]), "alpha 0": dict(alpha=0), "another taxonomy": dict(tx=tx2),
           "a cap below alpha": dict(lcp_cap=ALPHA - 1), "an index cap below alpha": dict(gi=gi16, alpha=17), "a cap the index cannot serve": dict(gi=gi16, lcp_cap=17)}
    for name, kw in bad.items():
        args = dict(mates=[a], gi=gi, tx=tx, alpha=ALPHA, lcp_cap=0)
        args.update(kw)
        with pytest.raises(api.LimeError) as e:
            ctx.classify_sample(args["mates"], args["gi"], args["tx"], args["alpha"], NORM, BETA, lcp_cap=args["lcp_cap"])
        assert e.value.code == _lib.ERR_ARG and len(str(e.value)) > len("lime error -1: ") + 10, (name, e.value)
    assert _free_bytes() == before
    for x in (a, b, empty, gi16, tx, tx2):
        x.close()
