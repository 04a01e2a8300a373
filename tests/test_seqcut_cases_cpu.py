"""Without a GPU: the models of tests/seqcut_cases.py (the cut rule, and the reader's refill loop over it) against api.fastq_read /
api.fasta_read.  Every case of fastq_cases.py and fasta_cases.py and 400 seeded inputs per format are cut into batches at every
max_reads and window size of seqcut_cases.grid: the batches, each parsed on its own bytes, concatenate to the whole file's records; a
malformed FASTQ is refused in its first failing batch with the whole file's reason and, with the lines handed out before it, the whole
file's line.  The classification writer appended in parts gives lime_write_classification's file.  One premise test pins that a read's
row of the score table does not depend on the other reads of the collection."""
import os
import re

import numpy as np
import pytest

from tests import fastq_cases as QC
from tests import seqcut_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Host:
    """api.fastq_read / api.fasta_read on bytes, through a file; results are kept per distinct input"""

    def __init__(self, tmp_path):
        self.path, self.seen = str(tmp_path / "in.seq"), {}

    def __call__(self, fmt, data):
        from lime_amd import _lib, api
        key = (fmt, data)
        if key not in self.seen:
            with open(self.path, "wb") as f:
                f.write(data)
            try:
                self.seen[key] = (api.fastq_read if fmt == SC.FASTQ else api.fasta_read)(self.path)
            except api.LimeError as e:
                assert e.code == _lib.ERR_ARG and fmt == SC.FASTQ
                self.seen[key] = QC.refusal_of(str(e))
        return self.seen[key]


def _check_input(host, fmt, name, data):
    """-> the number of (max_reads, window) pairs checked"""
    whole = host(fmt, data)
    refused = isinstance(whole, tuple)
    n_rec = SC.parse(fmt, data[:0])[1][0] if refused else len(whole)
    if refused:                                      # the grid's "more than the records" from the lines there are
        n_rec = (data.count(b"\n") + 1) // 4
    done = 0
    by_max_reads = {}
    for max_reads, window in SC.grid(n_rec):
        batches, cap = SC.model_reader(data, fmt, max_reads, window)
        what = (name, max_reads, window)
        assert b"".join(batches) == data[:sum(len(b) for b in batches)], what
        assert by_max_reads.setdefault(max_reads, batches) == batches, what      # the batches do not depend on the window
        got, lines_before, failure = [], 0, None
        for k, b in enumerate(batches):
            r = host(fmt, b)
            if isinstance(r, tuple):
                failure = (lines_before + r[0], r[1])
                break
            assert len(r) == max_reads or k == len(batches) - 1, what           # every batch but the last is full
            assert 1 <= len(r) <= max_reads or (fmt == SC.FASTA and not r), what
            got.extend(r)
            lines_before += 4 * len(r)
        if refused:
            assert failure == whole, (what, failure, whole)
            assert got == _valid_prefix(fmt, data, len(got)), what
        else:
            assert failure is None and got == whole, what
            assert sum(len(b) for b in batches) == len(data), what
        assert cap >= (window or 1) and (cap == (window or min(64 << 20, max(len(data), 1))) or window), what
        done += 1
    return done


def _valid_prefix(fmt, data, n_records):
    """the first n_records reads of a FASTQ input whose later part is malformed: its first 4 * n_records lines, read on their own"""
    lines = data.split(b"\n")
    return [ln.replace(b"\r", b"") for ln in lines[1:4 * n_records:4]]


@pytest.mark.parametrize("fmt", [SC.FASTQ, SC.FASTA], ids=["fastq", "fasta"])
def test_the_models_batches_concatenate_to_the_whole_file(tmp_path, fmt):
    from lime_amd import api
    host = _Host(tmp_path)
    inputs = SC.inputs(fmt, api.FASTA_BLOCK)
    assert sum(1 for k in inputs if k.startswith("fuzz_")) == SC.FUZZ_CASES == 400
    refused = 0
    for name, data in inputs.items():
        assert _check_input(host, fmt, name, data) == len(SC.MAX_READS) * len(SC.WINDOWS) == 40
        refused += isinstance(host(fmt, data), tuple)
    assert (refused >= 100) == (fmt == SC.FASTQ), refused


def test_the_fast_model_is_the_rule_on_the_windows_own_bytes():
    """model_reader cuts with the file's markers; model_cut, the rule on a window's own bytes, gives the same cuts"""
    from lime_amd import api
    for fmt in (SC.FASTQ, SC.FASTA):
        for k, (name, data) in enumerate(SC.inputs(fmt, api.FASTA_BLOCK).items()):
            if k % 7 or len(data) > 3000:
                continue
            for max_reads in (1, 2, 3):
                batches, _ = SC.model_reader(data, fmt, max_reads, 0)
                at = 0
                for b in batches:
                    cut, m, _ = SC.model_cut(data[at:], fmt, max_reads, True)
                    assert cut == len(b), (name, max_reads, at)
                    at += cut


def test_model_cut_by_hand():
    q = QC.rec() * 3                                 # 3 records of 15 bytes
    assert len(QC.rec()) == 15
    assert SC.model_cut(q, SC.FASTQ, 2, False) == (30, 2, 12) and SC.model_cut(q, SC.FASTQ, 5, False) == (45, 3, 12)
    assert SC.model_cut(q, SC.FASTQ, 5, True) == (45, 3, 12) and SC.model_cut(q[:-1], SC.FASTQ, 5, True) == (44, 3, 11)
    assert SC.model_cut(q[:-1], SC.FASTQ, 5, False) == (30, 2, 11) and SC.model_cut(q[:14], SC.FASTQ, 1, False) == (0, 0, 3)
    assert SC.model_cut(q[:-1], SC.FASTQ, 2, True) == (30, 2, 11) and SC.model_cut(b"", SC.FASTQ, 1, True) == (0, 0, 0)
    a = b"xx\n>a\nAC\n>b\nGG\nT>\n>c\n"
    assert SC.model_cut(a, SC.FASTA, 5, False) == (18, 2, 3) and SC.model_cut(a, SC.FASTA, 5, True) == (len(a), 3, 3)
    assert SC.model_cut(a, SC.FASTA, 1, False) == (9, 1, 3) and SC.model_cut(a, SC.FASTA, 2, True) == (18, 2, 3)
    assert SC.model_cut(b"xx\n>a\nAC", SC.FASTA, 1, False) == (3, 0, 1) and SC.model_cut(b"xx\nAC", SC.FASTA, 1, False) == (0, 0, 0)
    assert SC.model_cut(b"xx\nAC", SC.FASTA, 1, True) == (5, 0, 0) and SC.model_cut(b"A\r>x\n", SC.FASTA, 1, True) == (5, 0, 0)


def test_the_writer_in_parts_gives_the_whole_files_bytes(tmp_path):
    from lime_amd import api
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_full.npz"))
    golden = bytes(z["classification"])
    lines = golden.split(b"\n")[1:-1]
    v = np.zeros(len(lines), dtype=api.VERDICT)
    for k, ln in enumerate(lines):                   # the golden's verdict lines back into records
        t, r, taxon, sim = ln.split(b",")
        assert int(r) == k
        v["type"][k] = t[0]
        if t in (b"C", b"H"):
            v["taxon"][k], v["sim"][k] = int(taxon), np.float32(float(sim))
    for name, arr in (("golden", v), ("seeded", SC.seeded_verdicts(1000)), ("none", v[:0])):
        whole = str(tmp_path / (name + ".whole"))
        api.write_classification(whole, arr)
        want = open(whole, "rb").read()
        if name == "golden":
            assert want == golden
        for part in (1, 7, max(len(arr), 1)):
            p = str(tmp_path / f"{name}.{part}")
            w = api.ClassificationWriter(p)
            for at in range(0, len(arr), part):
                w.append(at, arr[at:at + part])
                assert not os.path.exists(p)         # (under a temporary name until it is closed)
            w.close(commit=True)
            assert open(p, "rb").read() == want, (name, part)
    before = set(os.listdir(tmp_path))
    w = api.ClassificationWriter(str(tmp_path / "dropped"))
    w.append(0, v[:5])
    assert len(set(os.listdir(tmp_path)) - before) == 1
    w.close(commit=False)
    assert set(os.listdir(tmp_path)) == before
    with pytest.raises(ZeroDivisionError):
        with api.ClassificationWriter(str(tmp_path / "raised")) as w:
            w.append(0, v[:5])
            1 / 0
    assert set(os.listdir(tmp_path)) == before


def test_symbols_exist():
    from lime_amd import _lib, api
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    for n in ("lime_seq_cut_dev", "lime_seq_reader_open", "lime_seq_reader_open_bytes", "lime_seq_reader_next", "lime_seq_reader_info", "lime_seq_reader_close",
              "lime_classify_sample_stream", "lime_classification_writer_open", "lime_classification_writer_append", "lime_classification_writer_close"):
        assert n in _lib.SYMBOLS and hasattr(lib, n) and re.search(r"\b%s\(" % n, header), n
    for n in ("seq_reader", "seq_reader_bytes", "seq_cut_dev", "classify_sample_stream"):
        assert hasattr(api.Context, n), n
    assert hasattr(api, "ClassificationWriter") and hasattr(api.SeqReader, "next") and hasattr(api.SeqReader, "__iter__")
    csrc = os.path.join(ROOT, "lime_amd", "csrc")
    shared, kernel = open(os.path.join(csrc, "lime_bytes.h")).read(), open(os.path.join(csrc, "lime_seqcut_kernel.hip")).read()
    assert shared.count("static_assert(LIME_FASTA_BLOCK == BY_WG * BY_LANE") == 1 and len(re.findall(r"static_assert\(\s*LIME_FASTA_BLOCK", shared)) == 1
    assert '#include "lime_bytes.h"' in kernel and "LIME_FASTA_BLOCK ==" not in kernel
    assert not re.search(r"\b\w*(WG|LANE)\s*=[^=]", kernel)           # no workgroup size or bytes per lane of its own: lime_bytes.h's
    assert "asm" not in kernel and "asm" not in shared
    make = open(os.path.join(ROOT, "lime_amd", "csrc", "Makefile")).read()
    # the resources target takes every file of KERNELS but lime_index_sort through kres.py, the spill gate and the lint, in one loop
    assert "lime_seqcut_kernel" in re.search(r"^KERNELS = (.+)$", make, re.M).group(1).split() and "LINTED = $(filter-out lime_index_sort,$(KERNELS))" in make
    assert "for f in $(LINTED)" in make and "$$f.hip -o $$d/$$b.s" in make and "_kres.txt && cat" in make


def test_the_usage_text_states_what_the_batched_counters_are(tmp_path):
    """LiME_fasta refuses --window-bytes without --batch-reads and a batch of 0 before it touches a device, and its usage text and DESIGN.md
    say that the clusters and the maximum length of a batched run are per-batch figures"""
    import subprocess
    exe = os.path.join(ROOT, "lime_amd", "bin", "LiME_fasta")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    base = [exe, "r.fastq", "--gidx", "g.gidx", "--lineage", "l.csv", "--readlen", "100", "--out", str(tmp_path / "out.txt")]
    for extra in (["--window-bytes", "4096"], ["--batch-reads", "0"], ["--batch-reads"], ["--batch-reads", "10", "--window-bytes", "0"]):
        p = subprocess.run(base + extra, capture_output=True, timeout=120)
        err = p.stderr.decode()
        assert p.returncode == 1 and "Error usage" in err and "[--batch-reads N [--window-bytes W]]" in err, err
        assert "per-batch figures" in err and "counts three times" in err, err
    assert not os.listdir(tmp_path)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**f10" in design and "per-batch figures" in design and "counts three times" in design


def test_premise_a_reads_row_does_not_depend_on_the_other_reads():
    """the score table of a collection computed on batches of its reads (each batch with all the genomes) and stacked is the whole
    collection's table: 30 seeded collections with duplicated reads, IUPAC symbols and 1 .. 4 genomes, alpha 3 and 5, with and without
    ebwt, batches of 1, 3 and 5 reads.  This does not exercise the batching code: it pins what it rests on."""
    from lime_amd import builder
    from oracle import oracle_py as oracle
    sym = np.frombuffer(b"ACGTACGTACGTNRY", dtype=np.uint8)
    n_cmp = 0
    for case in range(30):
        rng = np.random.default_rng([SC.SEED, 11, case])
        genomes = [sym[rng.integers(0, len(sym), size=int(rng.integers(20, 60)))].tobytes() for _ in range(int(rng.integers(1, 5)))]
        reads = []
        for _ in range(int(rng.integers(4, 9))):
            g = genomes[int(rng.integers(0, len(genomes)))]
            at = int(rng.integers(0, len(g) - 10))
            r = bytearray(g[at:at + int(rng.integers(8, 16))])
            if rng.random() < 0.5:
                r[int(rng.integers(0, len(r)))] = sym[int(rng.integers(0, len(sym)))]
            reads.append(bytes(r))
        reads.append(reads[0])                       # a duplicated read
        for alpha in (3, 5):
            for use_ebwt in (True, False):
                whole = _table(builder, oracle, reads, genomes, alpha, use_ebwt)
                for batch in (1, 3, 5):
                    parts = [_table(builder, oracle, reads[at:at + batch], genomes, alpha, use_ebwt) for at in range(0, len(reads), batch)]
                    assert np.array_equal(np.vstack(parts), whole), (case, alpha, use_ebwt, batch)
                    n_cmp += 1
    assert n_cmp == 360


def _table(builder, oracle, reads, genomes, alpha, use_ebwt):
    ebwt, lcp, da = builder.build_arrays(reads, genomes)[:3]
    clusters = oracle.detect(lcp, da, len(reads), alpha)[0]
    return oracle.score(da, ebwt if use_ebwt else None, clusters, len(reads), len(genomes))
