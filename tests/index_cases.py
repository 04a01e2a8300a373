"""Collections and references for the index builder's edge tests (tests/test_index_cases_cpu.py checks them without a GPU,
tests/test_index_edges_gpu.py runs them through lime_build_index / lime_build_index_dev, tools/fuzz_index.py soaks the random ones).
Everything here comes from fixed seeds or closed forms; lime_amd/builder.py stays the contract."""
import numpy as np

# the alphabet sizes on both sides of every change of the packing width, + ACGT (4) and ACGT + N (5)
SIGMAS = (1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 255, 256)
# document lengths, in units of k_syms and +- 1, at which the first sort (depth k) and the doubling rounds (2k, 4k) end
BOUNDARY_LENGTHS = ((1, -1), (1, 0), (1, 1), (2, -1), (2, 0), (2, 1), (4, -1), (4, 0), (4, 1))


def width_of(sigma):
    """(bits, k_syms) of lime_build_index_dev for `sigma` distinct bytes: codes 0 (terminator) .. sigma need bits_for(sigma) bits, never
    fewer than 2; as many codes as fit in 64 bits, at most 32 (lime_build.cpp, lime_build_index_dev:
    `bits = std::max(2u, bits_for(hw[1])), k_syms = std::min(64u / bits, 32u)`)"""
    bits = max(2, int(sigma).bit_length())
    return bits, min(64 // bits, 32)


def boundary_lengths(sigma):
    k = width_of(sigma)[1]
    return [m * k + d for m, d in BOUNDARY_LENGTHS]


def alphabet(rng, sigma):
    """sigma distinct byte values in random order; from two values on, one of them is >= 0x80 (a signed char would sort it first)"""
    a = rng.permutation(256)[:sigma].astype(np.uint8)
    if sigma >= 2 and int(a.max()) < 0x80:
        a[int(rng.integers(0, sigma))] = int(rng.integers(0x80, 0x100))
    assert len(set(a.tolist())) == sigma
    return a


def boundary_collection(sigma, seed):
    """(reads, genomes) over exactly `sigma` byte values with identical documents of the lengths at which the builder's rounds end"""
    rng = np.random.default_rng([int(seed), int(sigma)])
    k = width_of(sigma)[1]
    a = alphabet(rng, sigma)
    draw = lambda n: bytes(a[rng.integers(0, sigma, size=int(n))].tobytes())
    s = draw(4 * k + 2)
    twins = [s[:L] for L in boundary_lengths(sigma)]
    reads = twins + [b"", s[1:], s[k:], bytes(a.tobytes())]                    # the last one: every byte of the alphabet, so sigma is exact
    genomes = [s] + twins + [s[2 * k + 1:], s[4 * k:], b"", bytes([a[0]]) * (3 * k + 1)]
    if sigma >= 2:
        genomes.append((bytes([a[0], a[1]]) * (2 * k))[:3 * k + 1])
    assert sum(len(d) + 1 for d in reads + genomes) <= 4100
    return reads, genomes


ACGTN = np.frombuffer(b"ACGTN", np.uint8)
# differing symbols whose XOR has its lowest set bit at bit 0, 1 and 2: 'A' ^ 'T' = 0x15, 'A' ^ 'C' = 0x02, 'C' ^ 'G' = 0x04
XOR_PAIRS = ((b"A", b"T"), (b"A", b"C"), (b"C", b"G"))


def lcp_word_collection(seed):
    """(reads, genomes) over ACGTN.  For P = 0 .. 40 a pair of documents that share exactly P symbols and then differ (in XOR_PAIRS[P % 3]: of
    the pairs that meet one byte of an 8-byte word, P, P + 8, P + 16, at least three different lowest differing bits); both run on to the end
    of the word the difference is in, so the builder finds it by a word compare, and their lengths differ.  For P = 0 .. 24 a pair where
    one document is the other's first P symbols.  Packed back to back (api.pack_documents), the documents start at every address mod 8."""
    rng = np.random.default_rng([int(seed), 5])
    draw = lambda n: bytes(ACGTN[rng.integers(0, 5, size=int(n))].tobytes())
    docs = []
    for P in range(41):
        x, (c0, c1) = draw(P), XOR_PAIRS[P % 3]
        full = (P // 8 + 1) * 8 - P - 1                                        # symbols behind the difference up to the word's end
        docs += [x + c0 + draw(full + int(rng.integers(0, 4))), x + c1 + draw(full + 4 + int(rng.integers(0, 4)))]
    for P in range(25):
        x = draw(P)
        docs += [x + draw(1 + int(rng.integers(0, 12))), x]
    order = rng.permutation(len(docs))
    docs = [docs[i] for i in order]
    cut = len(docs) // 2
    reads, genomes = docs[:cut], docs[cut:]
    assert sum(len(d) + 1 for d in docs) <= 4100
    return reads, genomes


def word_compares_at_document_starts(reads, genomes):
    """What k_idx_lcp's compare loop meets on the rows of whole-document suffixes, where it starts from h = 0 (the position before is a
    terminator): -> (mismatch, ends); mismatch = set of (byte of the 8-byte word the first difference is in, lowest differing bit of that byte)
    over the rows where a word compare finds it, ends = set of (length of the shorter suffix) % 8 over the rows where the shorter suffix ends first."""
    docs = [bytes(d) for d in list(reads) + list(genomes)]
    BASE = 1 << 20
    sufs = sorted(([BASE + c for c in d[p:]] + [k], k, p) for k, d in enumerate(docs) for p in range(len(d) + 1))
    mismatch, ends = set(), set()
    for (_, kq, q), (_, kp, p) in zip(sufs, sufs[1:]):
        if p != 0:
            continue
        a, b = docs[kp], docs[kq][q:]
        lim = min(len(a), len(b))
        l = next((i for i in range(lim) if a[i] != b[i]), lim)
        if l == lim:
            ends.add(lim % 8)
        elif l // 8 * 8 + 8 <= lim:
            x = a[l] ^ b[l]
            mismatch.add((l % 8, (x & -x).bit_length() - 1))
    return mismatch, ends


def _closed_form(n_docs, L, term, full, arange, cat, repeat, u8, i32):
    """the one body of closed_form_runs / closed_form_runs_torch over an array module's full, arange, cat and repeat"""
    assert n_docs >= 2 and L >= 1
    A, Cc, m = ord("A"), ord("C"), n_docs - 1
    n = n_docs * (L + 1)
    ebwt = full(n, A, u8)
    ebwt[m] = Cc                                                               # before the last document's terminator
    ebwt[n_docs + (L - 1) * m:n_docs + L * m + 1] = term                       # the whole documents: block j = L and the first row behind it
    lcp = full(n, 0, i32)
    blocks = lcp[n_docs:n_docs + L * m].reshape(L, m)                          # (a view of lcp in both modules: the slice is contiguous)
    blocks[:] = arange(1, L + 1, 1)[:, None]
    blocks[:, 0] -= 1                                                          # against the block before (A^(j-1)), or a terminator row
    lcp[n_docs + L * m:] = arange(L - 1, -1, -1)
    da = cat([arange(0, n_docs, 1), repeat(arange(0, m, 1), L), full(L, m, i32)])
    return ebwt, lcp, da


def closed_form_runs(n_docs, L, term=0):
    """(ebwt, lcp, da) of the collection "documents 0 .. n_docs - 2 = 'A' * L, the last document = 'A' * (L - 1) + 'C'", L >= 1, written
    directly (n_docs >= 2: the row behind the blocks has a suffix A^L before it).  Rows: the n_docs terminators by document id; for
    j = 1 .. L the suffixes A^j of documents 0 .. n_docs - 2 by id (A^j$ sorts below every A^i C: the terminator, or an 'A' against the
    'C'); then the last document's A^(L-1) C, A^(L-2) C, ..., C."""
    e, l, d = _closed_form(n_docs, L, term, lambda n, v, t: np.full(n, v, t), lambda a, b, c: np.arange(a, b, c, dtype=np.int32),
                           np.concatenate, np.tile, np.uint8, np.int32)
    return e, l.view(np.uint32), d.view(np.uint32)


def closed_form_runs_torch(n_docs, L, term=0, device="cpu"):
    """closed_form_runs as torch tensors on `device` (uint8, int32, int32: build_index_dev's types), for sizes at which the host is slow"""
    import torch
    return _closed_form(n_docs, L, term, lambda n, v, t: torch.full((n,), v, dtype=t, device=device),
                        lambda a, b, c: torch.arange(a, b, c, dtype=torch.int32, device=device), torch.cat, lambda t, k: t.repeat(k),
                        torch.uint8, torch.int32)


def tied_after(reads, genomes, k):
    """how many suffixes are still in a group once the first k symbols are sorted: those with at least k symbols in front of their
    terminator (one whose terminator is inside the window is alone, by document id) whose first k symbols occur again in such a suffix.
    What index_info()["unresolved"][0] reports for k = k_syms."""
    from collections import Counter
    docs = [bytes(d) for d in list(reads) + list(genomes)]
    c = Counter(d[p:p + k] for d in docs for p in range(len(d) - k + 1))
    return sum(v for v in c.values() if v > 1)


def closed_form_documents(n_docs, L):
    """the collection of closed_form_runs as (reads, genomes)"""
    return [b"A" * L] * (n_docs - 1), [b"A" * (L - 1) + b"C"]


# FASTA as it comes: lower case, runs of N, IUPAC codes, CRLF, empty records, no final newline; r4's reverse complement is g3's first line
REAL_WORLD_READS = (b">r1 lower case and N runs\r\nacgtacgtnnnnnnnnnnACGTACGTNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNacgt\r\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\r\n"
                    b">r2 IUPAC\r\nACGTRYKMSWBDHVNacgtrykmswbdhvnU\r\nRYRYRYRYKMKMKMKMBDHVBDHVNNNN\r\n"
                    b">empty\r\n"
                    b">r3 mixed case twin of r1's start\r\nacgtacgtnnnnnnnnnnACGTACGTNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNacgA\r\n"
                    b">r4\r\nGATTACAGATTACAgattacaGATTACANNNNNGATTACA")                    # no final newline
REAL_WORLD_REFS = (b">g1\nACGTACGTNNNNNNNNNNACGTACGTNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNACGT\nGATTACAGATTACAGATTACAGATTACA\n"
                   b">g2 soft-masked\nacgtacgtacgtacgtGATTACAGATTACAnnnnnnnnnnRYKMSWBDHVN\n"
                   b">g_empty\n"
                   b">g3\nTGTAATCNNNNNTGTAATCtgtaatcTGTAATCTGTAATC\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN")


FUZZ_CASES, FUZZ_MAX_POSITIONS = 200, 3000


def fuzz_collection(seed, case):
    """one random collection of at most FUZZ_MAX_POSITIONS positions -> (reads, genomes, term, lcp_cap, description).  Drawn: the alphabet size
    from SIGMAS; document lengths from {0, 1, geometric, around k_syms * 2^r}; 0 .. 3 planted repeats; with probability 1/2 a document that holds
    every byte of the alphabet; duplicated documents with probability 1/2; the terminator byte; lcp_cap 0 or random."""
    rng = np.random.default_rng([int(seed), int(case)])
    sigma = int(rng.choice(SIGMAS))
    k = width_of(sigma)[1]
    a = alphabet(rng, sigma)
    draw = lambda n: bytearray(a[rng.integers(0, sigma, size=int(n))].tobytes())
    budget = int(rng.integers(1, FUZZ_MAX_POSITIONS + 1))
    mean = float(rng.choice([3, 30, 300]))
    docs, used = [], 0
    for _ in range(int(rng.integers(1, 60))):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            L = 0
        elif kind == 1:
            L = 1
        elif kind == 2:
            L = int(rng.geometric(1.0 / mean))
        else:
            L = max(0, (k << int(rng.integers(0, 4))) + int(rng.integers(-1, 2)))
        if used + L + 1 > budget:
            break
        docs.append(draw(L))
        used += L + 1
    if not docs:
        docs, used = [bytearray()], 1
    for _ in range(int(rng.integers(0, 4))):                                   # planted repeats: one string written into several documents
        rep = draw(int(rng.integers(2, 6 * k)))
        for _ in range(int(rng.integers(2, 6))):
            if not docs:
                break
            d = docs[int(rng.integers(0, len(docs)))]
            if len(d) == 0:
                continue
            o = int(rng.integers(0, len(d)))
            piece = rep[:len(d) - o]
            d[o:o + len(piece)] = piece
    if rng.random() < 0.5 and used + sigma + 1 <= FUZZ_MAX_POSITIONS:                      # every byte of the alphabet: the width is sigma's, not a narrower one
        docs.insert(int(rng.integers(0, len(docs) + 1)), bytearray(a.tobytes()))
        used += sigma + 1
    if docs and rng.random() < 0.5:                                            # identical documents: ties that only the document id breaks
        for _ in range(int(rng.integers(1, 5))):
            d = docs[int(rng.integers(0, len(docs)))]
            if used + len(d) + 1 > FUZZ_MAX_POSITIONS:
                break
            docs.insert(int(rng.integers(0, len(docs) + 1)), bytearray(d))
            used += len(d) + 1
    docs = [bytes(d) for d in docs]
    cut = int(rng.integers(0, len(docs) + 1))
    term = int(rng.integers(0, 256))
    lcp_cap = 0 if rng.random() < 0.5 else int(rng.integers(1, 2 * k + 3))
    assert used == sum(len(d) + 1 for d in docs) <= FUZZ_MAX_POSITIONS
    return docs[:cut], docs[cut:], term, lcp_cap, f"seed={seed} case={case} sigma<={sigma} docs={len(docs)} positions={used} term={term} lcp_cap={lcp_cap}"


def capped(want, cap):
    """the expected arrays under lcp_cap: min(lcp, cap), the other two unchanged; cap 0 = none"""
    return want if not cap else (want[0], np.minimum(want[1], np.uint32(cap)).astype(np.uint32), want[2])


def first_difference(got, want):
    """None if the three arrays are equal in type, shape and content, else a description of the first difference"""
    for name, g, w in zip(("ebwt", "lcp", "da"), got, want):
        if g.dtype != w.dtype or g.shape != w.shape:
            return f"{name}: {g.dtype}{g.shape} against {w.dtype}{w.shape}"
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            return f"{name} differs at {len(bad)} of {len(w)} positions, first {bad[:5]}: got {g[bad[:5]]}, want {w[bad[:5]]}"
    return None
