"""Without a GPU: what the genome-shard path rests on and its host-only parts.
  - the premise: a column of the score table does not depend on the other genomes of the collection (pinned like f10's premise about rows);
  - the numpy model of lime_lists_concat_dev's rule (tests/shard_cases.py) against clusterChoose of the whole table, at every kind of cut,
    at the 21 / 22 threshold of norm 85 and beta 0.25, and accumulated in two steps;
  - lime_gindex_shard_plan through ctypes;
  - LiME_fasta's usage text and its refusal of index shards built with different caps before any device is opened."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import shard_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(builder, oracle, reads, genomes, alpha, use_ebwt):
    ebwt, lcp, da = builder.build_arrays(reads, genomes)[:3]
    clusters = oracle.detect(lcp, da, len(reads), alpha)[0]
    return oracle.score(da, ebwt if use_ebwt else None, clusters, len(reads), len(genomes))


def test_premise_a_genomes_column_does_not_depend_on_the_other_genomes():
    """the score table of a collection computed against shards of its genomes (each shard with all the reads) and put side by side is the
    whole collection's table: 40 seeded collections with IUPAC symbols, a duplicated genome and a one-symbol variant of a genome appended
    (so that twins land in different shards), alpha 3 and 5, with and without ebwt, shards of 1, 2 and 3 genomes.  This does not exercise
    the shard code: it pins what it rests on."""
    from lime_amd import builder
    from oracle import oracle_py as oracle
    sym = np.frombuffer(b"ACGTACGTACGTNRY", dtype=np.uint8)
    n_cmp = 0
    for case in range(40):
        rng = np.random.default_rng([HC.SEED, 11, case])
        genomes = [sym[rng.integers(0, len(sym), size=int(rng.integers(20, 60)))].tobytes() for _ in range(int(rng.integers(2, 5)))]
        twin = bytearray(genomes[1])
        twin[int(rng.integers(0, len(twin)))] = sym[int(rng.integers(0, len(sym)))]
        genomes += [genomes[0], bytes(twin)]             # a duplicate and a one-symbol variant, behind the others
        reads = []
        for _ in range(int(rng.integers(4, 9))):
            g = genomes[int(rng.integers(0, len(genomes)))]
            at = int(rng.integers(0, len(g) - 10))
            r = bytearray(g[at:at + int(rng.integers(8, 16))])
            if rng.random() < 0.5:
                r[int(rng.integers(0, len(r)))] = sym[int(rng.integers(0, len(sym)))]
            reads.append(bytes(r))
        for alpha in (3, 5):
            for use_ebwt in (True, False):
                whole = _table(builder, oracle, reads, genomes, alpha, use_ebwt)
                assert whole.any()
                for shard in (1, 2, 3):
                    parts = [_table(builder, oracle, reads, genomes[at:at + shard], alpha, use_ebwt) for at in range(0, len(genomes), shard)]
                    assert np.array_equal(np.hstack(parts), whole), (case, alpha, use_ebwt, shard)
                    n_cmp += 1
    assert n_cmp == 480


def _parts_of(table, col_cuts, norm):
    return [HC.choose(t, norm, -1.0) for t in HC.split(table, col_cuts)]


def test_the_model_of_concatenation_gives_cluster_choose_of_the_whole_table():
    n_cases = 0
    for case in range(120):
        rng = np.random.default_rng([HC.SEED, 12, case])
        n_refs = int(rng.integers(1, 41))
        n_reads = int(rng.integers(1, 30))
        table = HC.sparse_table(n_reads, n_refs, rng, density=float(rng.choice([0.02, 0.1, 0.5])))
        for n_parts in sorted({1, min(2, n_refs), min(3, n_refs), min(7, n_refs), n_refs}):
            col_cuts = HC.cuts(n_refs, n_parts, rng)
            for norm, beta in ((HC.NORM, HC.BETA), (HC.NORM, 0.0), (HC.NORM, -1.0), (1, 0.5), (HC.NORM, 5.0)):
                want = HC.choose(table, norm, beta)
                got = HC.concat(_parts_of(table, col_cuts, norm), col_cuts[:-1], norm, beta)
                assert HC.same_lists(got, want), (case, n_parts, norm, beta)
                n_cases += 1
    assert n_cases >= 120 * 5 * 3


def test_the_model_on_the_rows_made_by_hand():
    col_cuts = [0, 3, 5, 9, 11]
    table, names = HC.handmade(col_cuts)
    want = HC.choose(table, HC.NORM, HC.BETA)
    parts = _parts_of(table, col_cuts, HC.NORM)
    got = HC.concat(parts, col_cuts[:-1], HC.NORM, HC.BETA)
    assert HC.same_lists(got, want)
    lens = dict(zip(names, np.diff(got[1].astype(np.int64))))
    assert not HC.passes(21, HC.NORM, HC.BETA) and HC.passes(22, HC.NORM, HC.BETA)
    assert lens["21 in every part: fails"] == 0 and lens["21 and 22: passes, the 21s listed too"] == 3 and lens["22 alone in the last part"] == 1
    assert lens["passes only through another part's maximum"] == 3 and lens["empty in all parts"] == 0 and lens["empty in some parts"] == 1
    # the first part alone, with the real beta, would have dropped the row that passes through the middle part's 22
    alone = HC.choose(HC.split(table, col_cuts)[0], HC.NORM, HC.BETA)
    r = names.index("passes only through another part's maximum")
    assert alone[1][r + 1] == alone[1][r] and parts[0][1][r + 1] - parts[0][1][r] == 2
    # with beta -1 a part lists every non-zero row and nothing else
    for t, p in zip(HC.split(table, col_cuts), parts):
        assert np.array_equal(np.diff(p[1].astype(np.int64)), (t != 0).sum(axis=1))


def test_accumulating_with_beta_minus_one_then_filtering_once_is_the_one_step_call():
    for case in range(40):
        rng = np.random.default_rng([HC.SEED, 13, case])
        n_refs = int(rng.integers(3, 30))
        table = HC.sparse_table(int(rng.integers(1, 20)), n_refs, rng, density=0.2)
        col_cuts = HC.cuts(n_refs, 3, rng)
        parts = _parts_of(table, col_cuts, HC.NORM)
        one = HC.concat(parts, col_cuts[:-1], HC.NORM, HC.BETA)
        acc = HC.concat(parts[:1], [0], HC.NORM, -1.0)
        for p, base in zip(parts[1:], col_cuts[1:-1]):
            acc = HC.concat([acc, p], [0, base], HC.NORM, -1.0)
        assert HC.same_lists(acc, HC.choose(table, HC.NORM, -1.0)), case
        assert HC.same_lists(HC.concat([acc], [0], HC.NORM, HC.BETA), one), case
        assert HC.same_lists(one, HC.choose(table, HC.NORM, HC.BETA)), case


def test_gindex_shard_plan():
    from lime_amd import _lib, api
    lens = [5, 3, 7, 1, 0, 4]                            # positions 6, 4, 8, 2, 1, 5
    off = np.concatenate([[0], np.cumsum(lens)])
    assert api.gindex_shard_plan(off, 10) == [0, 2, 4, 6]            # 6 + 4 fits exactly; 8 + 2 fits exactly; 1 + 5
    assert api.gindex_shard_plan(off, 9) == [0, 1, 2, 3, 6]          # one over: 6 + 4 no longer fits; 2 + 1 + 5 does
    assert api.gindex_shard_plan(off, 8) == [0, 1, 2, 3, 6]
    assert api.gindex_shard_plan(off, 26) == [0, 6] and api.gindex_shard_plan(off, 25) == [0, 5, 6]
    assert api.gindex_shard_plan(off, 2 ** 40) == [0, 6]
    assert api.gindex_shard_plan([0, 0, 0, 0], 1) == [0, 1, 2, 3]    # empty genomes: a terminator each
    assert api.gindex_shard_plan([0, 0, 0, 0], 2) == [0, 2, 3]
    assert api.gindex_shard_plan([0], 5) == [0]                      # no genome: no shard
    with pytest.raises(api.LimeError) as e:
        api.gindex_shard_plan(off, 7)                                # genome 2 holds 8 positions
    assert e.value.code == _lib.ERR_ARG and "genome 2 " in str(e.value) and "8 positions" in str(e.value)
    with pytest.raises(api.LimeError) as e:
        api.gindex_shard_plan(off, 0)
    assert e.value.code == _lib.ERR_ARG
    # cap: n_shards + 1 entries are written, never more
    lib = _lib.load()
    o = np.ascontiguousarray(off, dtype=np.uint64)
    for cap in range(0, 6):
        first = np.full(8, 0xFFFFFFFF, dtype=np.uint32)
        ns = np.zeros(1, dtype=np.uint32)
        rc = lib.lime_gindex_shard_plan(o.ctypes.data, 6, 10, first.ctypes.data, cap, ns.ctypes.data_as(_lib.C.POINTER(_lib.C.c_uint32)))
        assert (first[cap:] == 0xFFFFFFFF).all(), cap
        if cap >= 4:
            assert rc == 0 and ns[0] == 3 and list(first[:4]) == [0, 2, 4, 6]
        else:
            assert rc == _lib.ERR_ARG and ns[0] == 0 and b"first_doc holds" in lib.lime_last_error(), cap


def test_symbols_exist():
    from lime_amd import _lib, api
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "lime_hip.h")).read()
    for n in ("lime_lists_concat_dev", "lime_gindex_shard_plan", "lime_classify_sample_shards_dev", "lime_classify_sample_stream_shards"):
        assert n in _lib.SYMBOLS and hasattr(lib, n) and re.search(r"\b%s\(" % n, header), n
    for n in ("lists_concat", "classify_sample_shards"):
        assert hasattr(api.Context, n), n
    assert hasattr(api, "gindex_shard_plan")
    kernel = open(os.path.join(ROOT, "lime_amd", "csrc", "lime_listcat_kernel.hip")).read()
    assert "k_lc_rows" in kernel and "k_lc_copy" in kernel and "asm" not in kernel
    make = open(os.path.join(ROOT, "lime_amd", "csrc", "Makefile")).read()
    # the resources target takes every file of KERNELS but lime_index_sort through kres.py, the spill gate and the lint, in one loop
    assert "lime_listcat_kernel" in re.search(r"^KERNELS = (.+)$", make, re.M).group(1).split() and "LINTED = $(filter-out lime_index_sort,$(KERNELS))" in make
    assert "for f in $(LINTED)" in make and "$$f.hip -o $$d/$$b.s" in make and "_kres.txt && cat" in make
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "**f11" in design and "per-shard figures" in design


def _gidx_header(n_docs, n_text, lcp_cap, term=0):
    """a genome index file that passes lime_gindex_probe: the 64-byte header and a body of zeros of the sizes it states"""
    up = lambda b: (b + 15) & ~15
    n = n_text + n_docs
    head = struct.pack("<4sHBBIIQQQQQII", b"LGIX", 1, term, 0, n_docs, lcp_cap, n_text, (n_docs + 1) * 8, n * 4, n * 4, n * 4, n_text, n)
    assert len(head) == 64
    return head + bytes(up((n_docs + 1) * 8) + 3 * up(n * 4) + up(n_text) + up(n))


def _exe():
    exe = os.path.join(ROOT, "lime_amd", "bin", "LiME_fasta")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    return exe


def test_lime_fasta_usage_text_states_what_the_sharded_counters_are(tmp_path):
    p = subprocess.run([_exe(), "r.fastq", "--gidx", "a.gidx", "--gidx"], capture_output=True, timeout=120)
    err = p.stderr.decode()
    assert p.returncode == 1 and "Error usage" in err and "--gidx file.gidx [--gidx next.gidx ...]" in err, err
    assert "index shards" in err and "per-shard figures" in err and "per-batch figures" in err, err
    p = subprocess.run([_exe(), "r.fastq", "--refs", "x.fasta", "--gidx", "a.gidx", "--lineage", "l.csv", "--readlen", "100", "--out", str(tmp_path / "o")],
                       capture_output=True, timeout=120)
    assert p.returncode == 1 and b"Error usage" in p.stderr                     # --refs stays one in-process index
    p = subprocess.run([os.path.join(os.path.dirname(_exe()), "BuildIndex"), "r.fasta", "g.fasta", "out", "--shard-positions", "100"], capture_output=True, timeout=120)
    assert p.returncode == 1 and b"--shard-positions P" in p.stderr             # only with --refs
    assert not os.listdir(tmp_path)


def test_lime_fasta_refuses_shards_that_do_not_agree_before_any_device_is_opened(tmp_path):
    from lime_amd import api
    a, b, c = (str(tmp_path / n) for n in ("a.gidx", "b.gidx", "c.gidx"))
    open(a, "wb").write(_gidx_header(2, 30, 0))
    open(b, "wb").write(_gidx_header(1, 12, 20))
    open(c, "wb").write(_gidx_header(1, 12, 0))
    assert api.gindex_probe(a)["lcp_cap"] == 0 and api.gindex_probe(b) == {"n_docs": 1, "n_text": 12, "lcp_cap": 20, "term": 0}
    lineage = str(tmp_path / "l.csv")
    open(lineage, "w").write("Accession_number;Species_TaxID;Genus_TaxID;Family_TaxID;Order_TaxID;Class_TaxID;Phylum_TaxID\n"
                             + "".join(f"ACC_{k:03d}.1;{100 + k};200;300;400;500;600\n" for k in range(2)))
    out = str(tmp_path / "out.txt")
    base = [_exe(), "r.fastq", "--lineage", lineage, "--readlen", "100", "--out", out]
    p = subprocess.run(base + ["--gidx", a, "--gidx", b], capture_output=True, timeout=120)
    err = p.stderr.decode()
    assert p.returncode == 1 and "--trlcp 20" in err and "--trlcp 0" in err and "b.gidx" in err and "a.gidx" in err, err
    assert "HIP" not in err and "device" not in err, err                        # refused before lime_init
    p = subprocess.run(base + ["--gidx", a, "--gidx", c], capture_output=True, timeout=120)      # 3 genomes, a lineage of 2
    err = p.stderr.decode()
    assert p.returncode == 1 and "3 genomes" in err and "l.csv" in err and "HIP" not in err, err
    p = subprocess.run(base + ["--gidx", a, "--gidx", str(tmp_path / "none.gidx")], capture_output=True, timeout=120)
    assert p.returncode == 1 and b"none.gidx" in p.stderr
    assert not os.path.exists(out)
