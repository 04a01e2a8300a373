"""The references of tests/test_index_edges_gpu.py are right before anything is asked of the GPU: the collections of tests/index_cases.py
have the properties their tests rely on, the naive and the prefix-doubling builder of lime_amd/builder.py agree on them, and the closed form
is what the builders give.  No GPU here."""
import numpy as np
import pytest

from lime_amd.builder import build_arrays, build_arrays_sa
from tests import index_cases as IC

SEED = 20261


def _equal(got, want, what):
    diff = IC.first_difference(got, want)
    assert diff is None, f"{what}: {diff}"


def test_width_of_is_the_builders_rule():
    # (bits, k_syms) by hand from lime_build_index_dev's expression, every alphabet size of the tests
    want = {1: (2, 32), 2: (2, 32), 3: (2, 32), 4: (3, 21), 5: (3, 21), 7: (3, 21), 8: (4, 16), 15: (4, 16), 16: (5, 12), 31: (5, 12),
            32: (6, 10), 63: (6, 10), 64: (7, 9), 127: (7, 9), 128: (8, 8), 255: (8, 8), 256: (9, 7)}
    assert tuple(sorted(want)) == IC.SIGMAS
    for sigma, w in want.items():
        assert IC.width_of(sigma) == w
    assert IC.width_of(0) == (2, 32)
    # every width the builder can choose is met, and k_syms * bits stops dividing 64 on the way
    assert sorted({IC.width_of(s)[1] for s in IC.SIGMAS}) == [7, 8, 9, 10, 12, 16, 21, 32]
    assert {64 - b * k for b, k in map(IC.width_of, IC.SIGMAS)} == {0, 1, 4}


@pytest.mark.parametrize("sigma", IC.SIGMAS)
def test_boundary_collection_has_what_it_promises(sigma):
    reads, genomes = IC.boundary_collection(sigma, SEED)
    docs = reads + genomes
    k = IC.width_of(sigma)[1]
    assert sum(len(d) + 1 for d in docs) <= 4100
    seen = set(b"".join(docs))
    assert len(seen) == sigma
    if sigma >= 2:
        assert max(seen) >= 0x80
    if sigma == 256:
        assert 0 in seen
    s = genomes[0]
    assert len(s) == 4 * k + 2
    lengths = [k - 1, k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1, 4 * k - 1, 4 * k, 4 * k + 1]
    assert IC.boundary_lengths(sigma) == lengths
    for L in lengths:                                                    # identical twins, one among the reads and one among the genomes
        assert reads.count(s[:L]) >= 1 and genomes.count(s[:L]) >= 1
    assert sum(1 for d in docs if d != s and len(d) > 0 and s.endswith(d)) >= 3        # whole documents that are suffixes of another
    assert docs.count(b"") == 2
    assert any(len(d) == 3 * k + 1 and len(set(d)) == 1 for d in docs)
    if sigma >= 2:
        assert any(len(d) == 3 * k + 1 and d[0] != d[1] and d == (d[:2] * (2 * k))[:3 * k + 1] for d in docs)
    assert IC.boundary_collection(sigma, SEED) == (reads, genomes)     # a fixed seed: the same collection every time


@pytest.mark.parametrize("term", [0, ord("$")])
@pytest.mark.parametrize("sigma", IC.SIGMAS)
def test_both_builders_agree_on_the_boundary_collections(sigma, term):
    reads, genomes = IC.boundary_collection(sigma, SEED)
    _equal(build_arrays_sa(reads, genomes, term), build_arrays(reads, genomes, term), f"sigma {sigma}")


def test_lcp_word_collection_has_what_it_promises():
    reads, genomes = IC.lcp_word_collection(SEED)
    docs = reads + genomes
    assert sum(len(d) + 1 for d in docs) <= 4100
    assert set(b"".join(docs)) == set(b"ACGTN")
    assert IC.width_of(5) == (3, 21)
    want = build_arrays(reads, genomes, ord("$"))
    _equal(build_arrays_sa(reads, genomes, ord("$")), want, "lcp words")
    assert set(range(41)) <= set(want[1].tolist())
    # the planted pairs are there: for every P two documents whose first difference is at P, and two where one ends at P inside the other
    def common(a, b):
        m = min(len(a), len(b))
        return next((i for i in range(m) if a[i] != b[i]), m)
    by_len = {}
    for d in docs:
        by_len.setdefault(len(d), []).append(d)
    for P in range(25):
        assert any(e[:P] == d and len(e) > P for d in by_len.get(P, []) for e in docs), P
    differ = {}
    for i, a in enumerate(docs):
        for b in docs[i + 1:]:
            c = common(a, b)
            if c < min(len(a), len(b)) and c // 8 * 8 + 8 <= min(len(a), len(b)):
                x = a[c] ^ b[c]
                differ.setdefault(c, set()).add((x & -x).bit_length() - 1)
    assert all(P in differ for P in range(41))
    # what the kernel's compare loop meets on the rows where it starts from 0: a first difference in every byte of a word, under more than one
    # lowest differing bit (ctz >> 3, not ctz), and a shorter suffix that ends at every distance from a word boundary
    mismatch, ends = IC.word_compares_at_document_starts(reads, genomes)
    for byte in range(8):
        assert len({bit for b, bit in mismatch if b == byte}) >= 2, (byte, sorted(mismatch))
    assert {bit for _, bit in mismatch} == {0, 1, 2}
    assert ends == set(range(8))
    # packed back to back, the documents start at every address mod 8
    from lime_amd import api
    _, off = api.pack_documents(reads, genomes)
    assert {int(o) % 8 for o in off[:-1]} == set(range(8))


@pytest.mark.parametrize("term", [0, ord("$")])
@pytest.mark.parametrize("shape", [(2, 1), (3, 4), (7, 16), (50, 16)])
def test_closed_form_is_what_the_builder_gives(shape, term):
    import torch
    n_docs, L = shape
    reads, genomes = IC.closed_form_documents(n_docs, L)
    want = build_arrays_sa(reads, genomes, term)
    got = IC.closed_form_runs(n_docs, L, term)
    _equal(got, want, f"closed form {shape}")
    e, l, d = IC.closed_form_runs_torch(n_docs, L, term)
    assert e.dtype == torch.uint8 and l.dtype == torch.int32 and d.dtype == torch.int32
    _equal((e.numpy(), l.numpy().view(np.uint32), d.numpy().view(np.uint32)), want, f"closed form with torch {shape}")


def test_fuzz_collections_are_small_varied_and_repeatable():
    seen_sigma, seen_cap, twins, empties = set(), set(), 0, 0
    for case in range(IC.FUZZ_CASES):
        reads, genomes, term, cap, desc = IC.fuzz_collection(SEED, case)
        docs = reads + genomes
        assert sum(len(d) + 1 for d in docs) <= IC.FUZZ_MAX_POSITIONS and 0 <= term < 256, desc
        seen_sigma.add(len(set(b"".join(docs))))
        seen_cap.add(cap > 0)
        twins += len(set(docs)) < len(docs)
        empties += b"" in docs
    assert IC.fuzz_collection(SEED, 17) == IC.fuzz_collection(SEED, 17)
    assert len({IC.width_of(s) for s in seen_sigma if s}) == 8 and seen_cap == {False, True} and twins > 50 and empties > 50
    # the two builders agree on a few of them (all 200 are compared with the device's result in test_seeded_fuzz)
    for case in range(0, IC.FUZZ_CASES, 25):
        reads, genomes, term, cap, desc = IC.fuzz_collection(SEED, case)
        _equal(build_arrays_sa(reads, genomes, term), build_arrays(reads, genomes, term), desc)


@pytest.mark.parametrize("rc", [False, True])
def test_real_world_fasta_reads_as_restated(tmp_path, rc):
    from lime_amd import api
    from tests.test_index_cpu import py_fasta
    for name, data, n in (("reads", IC.REAL_WORLD_READS, 5), ("refs", IC.REAL_WORLD_REFS, 4)):
        p = tmp_path / (name + ".fasta")
        p.write_bytes(data)
        docs = py_fasta(data, rc)
        assert api.fasta_read(str(p), rc=rc) == docs and len(docs) == n and b"" in docs
        assert not any(b"\r" in d or b"\n" in d for d in docs)
    reads, refs = py_fasta(IC.REAL_WORLD_READS, rc), py_fasta(IC.REAL_WORLD_REFS)
    assert len(set(b"".join(reads + refs))) > 16                         # case, N and IUPAC kept: more than 4 bits a code
    assert b"\r\n" in IC.REAL_WORLD_READS and not IC.REAL_WORLD_READS.endswith(b"\n")
    if rc:
        assert reads[4] == refs[3][:40] == b"TGTAATCNNNNNTGTAATCtgtaatcTGTAATCTGTAATC"
    _equal(build_arrays_sa(reads, refs, 0), build_arrays(reads, refs, 0), "real-world FASTA")


def test_tied_after_counts_the_suffixes_left_in_groups():
    # ABAB.. : with k = 2 the windows AB (x3, the last one of them followed by the terminator counts: two symbols in front of it), BA (x2)
    assert IC.tied_after([b"ABABAB"], [], 2) == 5
    assert IC.tied_after([b"ABABAB"], [], 4) == 2 and IC.tied_after([b"ABABAB"], [], 5) == 0
    assert IC.tied_after([b"AC", b"AC", b"A"], [b""], 2) == 2 and IC.tied_after([b"AC", b"AC", b"A"], [], 3) == 0
    assert IC.tied_after([b"AC"], [b"AC"], 1) == 4
    for sigma in IC.SIGMAS:                                              # the twins of 4k + 1 symbols alone leave 2 * (3k + 2) suffixes tied
        k = IC.width_of(sigma)[1]
        assert IC.tied_after(*IC.boundary_collection(sigma, SEED), k) >= 2 * (3 * k + 2)
