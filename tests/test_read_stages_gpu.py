"""Every read-preparation stage at once: the stage chain of the readers (lime_seq_reader_set_trim, _set_adapter, _set_filter, _set_qc,
_set_overlap; lime_seq_reader_next_pair) against the chained public calls on the whole files, and the stage lines that LiME_fasta prints.
The input is 23 pairs of at most 125 symbols over three seeded genomes of 4000 symbols: read-through pairs that run into the R1 / R2
adapters, pairs whose adapter remnant is one or two symbols (only the overlap cut finds them), long fragments that overlap without a cut,
G tails, an N-rich read, a read of low quality throughout and sequencer-like qualities with low ends, as a FASTQ pair (mate 2 with CRLF).
The models of tests/trim_cases.py, adapter_cases.py, filter_cases.py and overlap_cases.py say that every stage changes a read and that reads
are emptied.
tests/golden/lime_fasta_stage_lines.json holds the program's stdout (without the `Time:` line) and its usage text as a build of the parent
commit named in the fixture printed them on an MI355X, from the files' directory with relative names, by
    LiME_fasta r1.fastq r2.fastq --gidx g.gidx --lineage LineageFile.csv --readlen auto --out out.txt --trim-qual 20
               --trim-adapter AGATCGGAAGAGCACACGTCTGAACTCCAGTCA,AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT --trim-polyx G --min-len 20 --max-n 5
               --trim-overlap 30 --qc-report qc.json --qc-positions 64 [--batch-reads 7]
(`python -m tests.test_read_stages_gpu COMMIT` writes the files, runs the two commands and records the fixture)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import adapter_cases as A
from tests import filter_cases as F
from tests import overlap_cases as V
from tests import trim_cases as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lime_amd", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lime_fasta_stage_lines.json")
SEED = 20317
PAIRS = 23
Q5, Q3 = 0, 20
ADAPTERS = (A.TRUSEQ_R1, A.TRUSEQ_R2)
AD_O, AD_E = 3, 10
FILTER = F.params(polyx=F.G_, min_len=20, max_n=5)
OV_O, OV_E = 30, 10
QC_POS = 64
BATCHES = (1, 7, 64)                             # one record, a batch that does not divide the file, more than the file
LINEAGE = (b"Acc_Num;Species_TaxID;Genus_TaxID;Family_TaxID;Order_TaxID;Class_TaxID;Phylum_TaxID\r\nAP009048;562;561;543;91347;1236;1224\r\n"
           b"CP001845;1313;1301;1300;186826;91061;1239\r\nCR543861;62977;469;468;72274;1236;1224\r\n")
STAGE_ARGS = ["--trim-qual", str(Q3), "--trim-adapter", (ADAPTERS[0] + b"," + ADAPTERS[1]).decode(), "--trim-polyx", "G", "--min-len", "20", "--max-n", "5",
              "--trim-overlap", str(OV_O), "--qc-report", "qc.json", "--qc-positions", str(QC_POS)]
BASE_ARGS = ["--gidx", "g.gidx", "--lineage", "LineageFile.csv", "--readlen", "auto", "--out", "out.txt"]


@functools.lru_cache(maxsize=None)
def _sample():
    """-> (genomes, (mates 1, mates 2), (qualities 1, qualities 2))"""
    rng = np.random.default_rng([SEED, 1])
    genomes = [T.bases(rng, 4000) for _ in range(3)]
    good = lambda L: bytes([T.Q(38)]) * L
    r, q = ([], []), ([], [])
    for k in range(PAIRS):
        g, at = genomes[k % 3], 150 * k
        read, far = g[at:at + 100], V.revcomp(g[at + 300:at + 400])
        if k < 6:                                # read-through into the adapters, one wrong symbol in the fragment
            a, b = V.plant(rng, read, int(rng.integers(40, 91)), *ADAPTERS, n_err=1)
            qa, qb = good(len(a)), good(len(b))
        elif k < 9:                              # one or two adapter symbols left: no adapter hit, the overlap cut alone finds it
            a, b = V.plant(rng, read, 98 + k % 2, *ADAPTERS)
            qa, qb = good(len(a)), good(len(b))
        elif k < 11:                             # a fragment of 150 in mates of 125: an overlap and no cut
            a, b = V.plant(rng, g[at:at + 150], 150, *ADAPTERS, La=125, Lb=125)
            qa, qb = good(125), good(125)
        else:                                    # mates of a fragment of 400 that do not meet, of odd lengths
            a, b = read[:(100, 61, 33, 100)[k % 4]], far[:(100, 100, 87, 45)[k % 4]]
            if k in (11, 12):
                a = F.plant(rng, a, 25, b"G")    # a G tail
            if k == 13:
                b = F.plant(rng, b, 14, b"G", 0.05)
            if k == 15:                          # an N-rich read
                x = bytearray(a)
                x[10:70:5] = b"N" * 12
                a = bytes(x)
            qa, qb = T.sample_quals(rng, len(a)), T.sample_quals(rng, len(b))
            if k in (11, 12):
                qa = good(len(a))                # (a two-colour instrument calls its G tails with high quality)
            if k == 13:
                qb = good(len(b))
            if k == 16:
                qb = bytes([T.Q(5)]) * len(b)    # low throughout: the quality trim empties it
        for m, (s, ql) in enumerate(((a, qa), (b, qb))):
            r[m].append(s); q[m].append(ql)
    return genomes, r, q


@functools.lru_cache(maxsize=None)
def _models():
    """-> per mate the models' [trimmed, adapter-trimmed, filtered, cut] reads and their infos, and the overlap cut's info"""
    _, r, q = _sample()
    reads, infos = [], []
    for m in range(2):
        t, ti = T.trim_model(r[m], q[m], Q5, Q3)
        a, ai = A.trim_model(t, ADAPTERS[m], AD_O, AD_E)
        f, fi = F.filter_model(a, FILTER)
        reads.append([t, a, f]); infos.append([ti, ai, fi])
    c1, c2, _, oi = V.cut_model(reads[0][2], reads[1][2], OV_O, OV_E)
    reads[0].append(c1); reads[1].append(c2)
    return reads, infos, oi


def _write(d):
    genomes, r, q = _sample()
    for m in range(2):
        open(os.path.join(d, f"r{m + 1}.fastq"), "wb").write(T.fastq_of(r[m], q[m], eol=b"\r\n" if m else b"\n"))
    open(os.path.join(d, "r1.fasta"), "wb").write(A.fasta_of(r[0]))
    open(os.path.join(d, "LineageFile.csv"), "wb").write(LINEAGE)
    return genomes


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory, ctx):
    d = str(tmp_path_factory.mktemp("read_stages"))
    gi = ctx.build_genome_index(_write(d))
    gi.save(os.path.join(d, "g.gidx"))
    gi.close()
    return d


def _flat(qc):
    return qc["tables"].tolist()


@pytest.fixture(scope="module")
def whole(ctx, files):
    """the chained public calls on the whole files, once -> text, doc_off and raw / out tables per mate, the infos"""
    w = {"text": [], "doc_off": [], "raw": [], "out": [], "trim": [], "adapter": [], "filter": []}
    left = []
    for m in range(2):
        raw = ctx.docs_from_fastq_qual(os.path.join(files, f"r{m + 1}.fastq"))
        w["raw"].append(_flat(ctx.docs_qc(raw, QC_POS)))
        t, ti = ctx.docs_trim(raw, Q5, Q3)
        a, ai = ctx.docs_trim_adapter(t, ADAPTERS[m], AD_O, AD_E)
        f, fi = ctx.docs_filter(a, **FILTER)
        w["trim"].append(ti); w["adapter"].append(ai); w["filter"].append(fi)
        for x in (raw, t, a):
            x.close()
        left.append(f)
    cut = ctx.docs_trim_overlap(left[0], left[1], OV_O, OV_E)
    w["overlap"] = cut[2]
    for m in range(2):
        text, off = cut[m].get()
        w["text"].append(text.tobytes()); w["doc_off"].append(off.tolist())
        w["out"].append(_flat(ctx.docs_qc(cut[m], QC_POS)))
        cut[m].close(); left[m].close()
    return w


def test_every_stage_changes_a_read_and_reads_are_emptied():
    _, r, _ = _sample()
    reads, infos, oi = _models()
    assert len(r[0]) == len(r[1]) == PAIRS and max(len(x) for m in range(2) for x in r[m]) <= 125
    for m in range(2):
        ti, ai, fi = infos[m]
        print("mate", m + 1, ti, ai, fi)
        assert ti["n_changed"] >= 1 and ai["n_changed"] >= 1 and fi["symbols_out"] < fi["symbols_in"]
    print(oi)
    assert infos[1][0]["n_empty"] >= 1                                       # the read of low quality throughout
    assert infos[0][2]["n_polyx"] >= 1 and infos[1][2]["n_polyx"] >= 1 and infos[0][2]["n_many_n"] >= 1 and infos[0][2]["n_short"] >= 1
    assert oi["n_cut"] >= 3 and oi["n_overlap"] > oi["n_cut"]                # the short remnants; the long fragments
    assert any(len(x) == 0 for x in reads[0][3]) and any(len(x) == 0 for x in reads[1][3])


def test_the_whole_file_chain_gives_the_models_reads(whole):
    reads, infos, oi = _models()
    for m in range(2):
        text, off = T.records(reads[m][3])
        assert whole["text"][m] == text.tobytes() and whole["doc_off"][m] == off.tolist()
        assert [whole[k][m] for k in ("trim", "adapter", "filter")] == infos[m]
    assert whole["overlap"] == oi


@pytest.mark.parametrize("max_reads", BATCHES)
def test_linked_readers_with_every_stage_give_the_whole_file_chain(ctx, files, whole, max_reads):
    rs = [ctx.seq_reader(os.path.join(files, f"r{m + 1}.fastq")) for m in range(2)]
    for m, r in enumerate(rs):
        r.set_trim(Q5, Q3)
        r.set_adapter(ADAPTERS[m], AD_O, AD_E)
        r.set_filter(**FILTER)
        r.set_qc(QC_POS)
    rs[0].set_overlap(rs[1], OV_O, OV_E)
    text, off, n_batches = [b"", b""], [[0], [0]], 0
    while True:
        b = rs[0].next_pair(rs[1], max_reads)
        if b is None:
            break
        assert b[2] == len(off[0]) - 1                                       # the number of the batch's first record
        for m in range(2):
            assert not b[m].has_qual
            t, o = b[m].get()
            off[m] += [int(x) + len(text[m]) for x in o[1:]]
            text[m] += t.tobytes()
            b[m].close()
        n_batches += 1
    assert n_batches == (PAIRS + max_reads - 1) // max_reads
    for m, r in enumerate(rs):
        assert text[m] == whole["text"][m] and off[m] == whole["doc_off"][m]
        assert r.trim_info() == whole["trim"][m] and r.adapter_info() == whole["adapter"][m] and r.filter_info() == whole["filter"][m]
        assert r.overlap_info() == whole["overlap"]
        assert _flat(r.qc("raw")) == whole["raw"][m] and _flat(r.qc("out")) == whole["out"][m]
        r.close()


def test_the_report_alone_keeps_no_qualities(ctx, files):
    for name, parse in (("r1.fastq", ctx.docs_from_fastq_qual), ("r1.fasta", ctx.docs_from_file)):
        path = os.path.join(files, name)
        r = ctx.seq_reader(path)
        r.set_qc(QC_POS)
        n = 0
        while True:
            b = r.next(7)
            if b is None:
                break
            assert not b[0].has_qual and b[1] == n
            n += b[0].info()[0]
            b[0].close()
        assert n == PAIRS
        d = parse(path)
        want = ctx.docs_qc(d, QC_POS)
        raw, out = r.qc("raw"), r.qc("out")
        assert _flat(raw) == _flat(want)
        quality_columns = int(raw["rows"][:, 5:].sum())
        assert (quality_columns > 0) == name.endswith("fastq"), (name, quality_columns)
        plain = ctx.docs_from_file(path)                                     # as handed out: the symbols alone
        assert _flat(out) == _flat(ctx.docs_qc(plain, QC_POS)) and int(out["rows"][:, 5:].sum()) == 0
        for x in (d, plain, r):
            x.close()


def _program(d, extra):
    """LiME_fasta on the pair with every stage flag, from the files' directory -> (exit status, stdout lines without `Time:`)"""
    p = subprocess.run([os.path.join(BIN, "LiME_fasta"), "r1.fastq", "r2.fastq"] + BASE_ARGS + STAGE_ARGS + extra, capture_output=True, timeout=600, cwd=d)
    return p.returncode, [ln for ln in p.stdout.decode().splitlines() if not ln.startswith("Time:")], p.stderr.decode()


REFUSED = (["r1.fastq", "--trim-qual", "20", "--readlen", "100"], ["r1.fastq", "--trim-overlap", "30", "--readlen", "auto"],
           ["r1.fastq", "--qc-positions", "64", "--readlen", "auto"])


def _usage(d, args):
    exe = os.path.join(BIN, "LiME_fasta")
    p = subprocess.run([exe] + args + ["--gidx", "g.gidx", "--lineage", "LineageFile.csv", "--out", "no.txt"], capture_output=True, timeout=600, cwd=d)
    return p.returncode, p.stdout.decode(), p.stderr.decode().replace(exe, "LiME_fasta")


@pytest.mark.parametrize("mode", ["whole", "batched"])
def test_the_programs_stage_lines_do_not_move(files, mode):
    want = json.load(open(GOLDEN))
    rc, lines, err = _program(files, ["--batch-reads", "7"] if mode == "batched" else [])
    print("\n".join(lines))
    assert rc == 0, err[-2000:]
    assert lines == want[mode]
    os.remove(os.path.join(files, "out.txt"))


@pytest.mark.parametrize("args", REFUSED, ids=lambda a: " ".join(a[1:]))
def test_a_refused_command_line_prints_the_usage_and_ends_with_1(files, args):
    rc, out, err = _usage(files, args)
    assert rc == 1 and out == "" and err == json.load(open(GOLDEN))["usage"]
    assert not os.path.exists(os.path.join(files, "no.txt"))


def _record(commit):
    """the fixture, from the program as it is built in this tree (a checkout of `commit`)"""
    import tempfile
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    with tempfile.TemporaryDirectory() as d:
        c = api.Context(0)
        gi = c.build_genome_index(_write(d))
        gi.save(os.path.join(d, "g.gidx"))
        gi.close(); c.close()
        rec = {"parent": commit}
        for mode, extra in (("whole", []), ("batched", ["--batch-reads", "7"])):
            rc, rec[mode], err = _program(d, extra)
            assert rc == 0, err
        usages = [_usage(d, a) for a in REFUSED]
        assert all(u == (1, "", usages[0][2]) for u in usages), usages
        rec["usage"] = usages[0][2]
    json.dump(rec, open(GOLDEN, "w"), indent=1)
    open(GOLDEN, "a").write("\n")


if __name__ == "__main__":
    _record(sys.argv[1])
