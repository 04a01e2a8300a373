"""Collections for the merge of reads into a prebuilt genome index (lime_merge_index; tests/test_merge_edges_gpu.py runs them on the
device) and an independent Python model of the merge (tests/test_merge_cases_cpu.py checks the model against lime_amd/builder.py without
a GPU: the decomposition itself -- ranks by text comparison, placement by i + j[i] / k + c[k], the lcp of two neighbours of one side
taken from that side's own array -- is proven before any kernel runs).  Everything comes from fixed seeds; builder.py stays the contract."""
import bisect

import numpy as np

from tests import index_cases as IC

SEED = 20267


def _docs(docs):
    return [d.encode() if isinstance(d, str) else bytes(d) for d in docs]


def side_suffixes(docs):
    """the suffixes of one side in its own sorted order -> list of (symbols in front of the terminator, document): bytes compare as unsigned
    bytes and a proper prefix sorts first (the terminator is below every symbol); equal symbols: by document id"""
    docs = _docs(docs)
    return sorted((d[p:], k) for k, d in enumerate(docs) for p in range(len(d) + 1))


def common(a, b):
    lim = min(len(a), len(b))
    return next((h for h in range(lim) if a[h] != b[h]), lim)


def model_merge(reads, genomes, term=0, lcp_cap=0):
    """(ebwt, lcp, da) of reads + genomes the way lime_merge_index_dev makes them, and what the tests want to know about the case:
    -> (arrays, facts); facts = {"j": ranks, "cross": the uncapped lcp values compared across the sides, "runs": runs of read suffixes}"""
    from lime_amd.builder import build_arrays
    reads, genomes = _docs(reads), _docs(genomes)
    er, lr, dr = build_arrays(reads, [], term)
    eg, lg, dg = build_arrays([], genomes, term)
    sr, sg = side_suffixes(reads), side_suffixes(genomes)
    assert [k for _, k in sr] == dr.tolist() and [k for _, k in sg] == dg.tolist()
    nr, ng = len(sr), len(sg)
    gsym = [s for s, _ in sg]
    # a genome suffix is below a read suffix if its symbols compare below (a first difference, or it ends where the read goes on); one that
    # ends together with the read is above it, because the read's document id is the lower one: the lower bound over the symbols
    j = [bisect.bisect_left(gsym, s) for s, _ in sr]
    assert all(a <= b for a, b in zip(j, j[1:]))
    c, i = [], 0
    for k in range(ng + 1):                                                    # c[k] = read suffixes with j <= k
        while i < nr and j[i] <= k:
            i += 1
        c.append(i)
    n = nr + ng
    ebwt, lcp, da = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    filled = np.zeros(n, bool)
    cross = []
    for i in range(nr):
        slot = i + j[i]
        assert not filled[slot]; filled[slot] = True
        ebwt[slot], da[slot] = er[i], dr[i]
        if slot == 0:
            lcp[slot] = 0
        elif i > 0 and j[i] == j[i - 1]:
            lcp[slot] = lr[i]
        else:
            cross.append(common(sr[i][0], sg[j[i] - 1][0])); lcp[slot] = cross[-1]
    for k in range(ng):
        before = c[k - 1] if k else 0
        slot = k + c[k]
        assert not filled[slot]; filled[slot] = True
        ebwt[slot], da[slot] = eg[k], len(reads) + dg[k]
        if slot == 0:
            lcp[slot] = 0
        elif c[k] == before:
            lcp[slot] = lg[k]
        else:
            cross.append(common(sr[c[k] - 1][0], sg[k][0])); lcp[slot] = cross[-1]
    assert filled.all()
    runs = sum(1 for i in range(nr) if i + 1 == nr or j[i] != j[i + 1])
    return IC.capped((ebwt, lcp, da), lcp_cap), {"j": j, "cross": cross, "runs": runs, "c": c}


# ---- 1: ties ----
TIES = ([b"ACGT", b"CGT", b"T", b"", b"ACGTACGT", b"ACGTACGTA", b"ACGTACGA"], [b"ACGTACGT", b"ACGT", b""])

# ---- 2: one symbol, every compare ends by length, at every remainder mod 8 ----
ONE_SYMBOL = ([b"A" * k for k in range(18)], [b"A" * m for m in (0, 1, 7, 8, 9, 16, 17, 33)])


# ---- 3: index_cases.lcp_word_collection as it is, and with the sides swapped ----
def word_collections():
    reads, genomes = IC.lcp_word_collection(SEED)
    return {"as_it_is": (reads, genomes), "swapped": (genomes, reads)}


# ---- 4: bytes 0x00 and 0xFF as symbols on both sides ----
def extreme_bytes():
    rng = np.random.default_rng([SEED, 4])
    a = np.array([0x00, 0xFF, 0x41], np.uint8)
    draw = lambda n: bytes(a[rng.integers(0, 3, size=int(n))].tobytes())
    s = draw(120)
    reads = [b"\x00", b"\xff", b"\x00\x00", b"\xff\xff", b"\x00\xff", s[5:40], s[50:59], s[60:76] + b"\x00", s[60:76] + b"\xff", b"", draw(30)]
    genomes = [s, b"\xff", b"\x00", b"", b"\x00" * 17, b"\xff" * 17, draw(60)]
    return reads, genomes


# ---- 5: degenerate sides ----
def degenerate():
    rng = np.random.default_rng([SEED, 5])
    acgt = lambda n: bytes(IC.ACGTN[rng.integers(0, 4, size=int(n))].tobytes())
    g = [acgt(200), acgt(90), b""]
    return {
        "no_reads": ([], g),
        "only_empty_reads": ([b"", b"", b""], g),
        "no_genomes": ([acgt(30) for _ in range(9)] + [b""], []),
        "one_genome_of_one_symbol": ([acgt(25) for _ in range(6)] + [b"C", b"", b"CC"], [b"C"]),
        "all_reads_below": ([b"A" * k for k in (1, 2, 9, 17)] + [b"AA+A", b"+A"], [b"C" + acgt(40).replace(b"A", b"C"), b"CCGT"]),          # A... against C...
        "all_reads_above": ([acgt(20).replace(b"A", b"T").replace(b"C", b"t").replace(b"G", b"T") for _ in range(8)] + [b"T" * 9],
                            [acgt(60).replace(b"T", b"G"), b"GGC"]),                                                                      # j = Ng
        "nothing": ([], []),
    }


# ---- 6: runs ----
RUN_COPIES = 300
RUN_FIRSTS = (319, 320, 321, 468, 469, 470)


def runs_collection(first):
    """300 copies of one read X (over C, G; its whole-document suffixes are one run of 300 read suffixes between two neighbouring genome
    suffixes), a genome over 0xF0 / 0xF1 whose 300+ suffixes no read falls between, and padding reads (b"A": two read suffixes in front of
    the run each, b"": one) so that the run's first read sits at index `first` of the reads' order.  The 300 terminator-only suffixes of the
    copies sort in front of everything, so no run of the copies can start below i = 300: RUN_FIRSTS puts the run's first read at
    5 * 64 - 1, 5 * 64, 5 * 64 + 1 (the edges of a wave) and its last read (first + 299) at 3 * 256 - 1, 3 * 256, 3 * 256 + 1 (the edges of
    a workgroup)."""
    rng = np.random.default_rng([SEED, 6])
    cg = np.frombuffer(b"CG", np.uint8)
    x = b"CCCCCGCCCCGCCCGCCGCG"                                                 # below every proper suffix of itself
    s = bytes(cg[rng.integers(0, 2, size=150)].tobytes())
    hi = bytes(np.array([0xF0, 0xF1], np.uint8)[rng.integers(0, 2, size=310)].tobytes())
    genomes = [s[:70] + x[:12] + b"T" + s[70:], hi]
    base = [x] * RUN_COPIES
    below = sum(1 for suf, _ in side_suffixes(base) if suf < x)
    assert below == RUN_COPIES                                                 # the copies' terminator-only suffixes, nothing else
    pad = first - below
    assert pad >= 0
    reads = [b"A"] * (pad // 2) + [b""] * (pad % 2) + base
    return reads, genomes


# ---- 7: views ----
def views_collection():
    """the last genome is shorter than eight symbols and a read is its extension; the last read is shorter than eight symbols and a genome
    is its extension: a word load past either text's end would read the bytes behind it, and 0x00 there against 0xFF changes the order"""
    rng = np.random.default_rng([SEED, 7])
    acgt = lambda n: bytes(IC.ACGTN[rng.integers(0, 4, size=int(n))].tobytes())
    s = acgt(300)
    genomes = [s, b"GATTACAGATTACA" + acgt(20), b"ACGTA"]
    reads = [s[10:60], s[100:131], b"ACGTACGTTG", b"ACGTAC", acgt(40), b"GATTACAGATTACA", b"GAT"]
    return reads, genomes


# ---- 8: caps ----
def caps_collection():
    """reads that share exactly 14 .. 18 symbols with a genome suffix and then differ with 'A' (below every genome symbol) or 'T' (above):
    the genome is over C, G"""
    rng = np.random.default_rng([SEED, 8])
    cg = np.frombuffer(b"CG", np.uint8)
    s = bytes(cg[rng.integers(0, 2, size=600)].tobytes())
    reads = []
    for n, k in enumerate(range(14, 19)):
        reads += [s[100 * n + 7:100 * n + 7 + k] + b"A", s[100 * n + 7:100 * n + 7 + k] + b"T" + s[:5]]
    return reads, [s, s[300:340]]


def pack(docs):
    """one side's documents -> (text uint8, doc_off uint64[n + 1]) the way api.pack_documents packs a collection"""
    docs = _docs(docs)
    off = np.zeros(len(docs) + 1, np.uint64)
    if docs:
        off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    text = np.frombuffer(b"".join(docs), np.uint8) if int(off[-1]) else np.zeros(1, np.uint8)
    return np.ascontiguousarray(text), off


# ---- the genome index file, from the layout documented in include/lime_hip.h ----
def gindex_file_bytes(n_docs, n_text, term=0, lcp_cap=0, doc_off=None, magic=b"LGIX", version=1, sizes=None):
    """a genome index file with zeroed sa / lcp / da / text / ebwt, written with numpy from the documented layout"""
    n = n_text + n_docs
    want = [(n_docs + 1) * 8, n * 4, n * 4, n * 4, n_text, n]
    sz = list(want if sizes is None else sizes)
    h = np.zeros(64, np.uint8)
    h[0:4] = np.frombuffer(magic, np.uint8)
    h[4:6] = np.frombuffer(np.array([version], "<u2").tobytes(), np.uint8)
    h[6] = term
    h[8:16] = np.frombuffer(np.array([n_docs, lcp_cap], "<u4").tobytes(), np.uint8)
    h[16:56] = np.frombuffer(np.array([n_text] + sz[:4], "<u8").tobytes(), np.uint8)
    h[56:64] = np.frombuffer(np.array(sz[4:], "<u4").tobytes(), np.uint8)
    up16 = lambda b: (b + 15) // 16 * 16
    body = np.zeros(sum(up16(b) for b in want), np.uint8)
    if doc_off is None:
        doc_off = np.linspace(0, n_text, n_docs + 1).astype("<u8")
    body[:(n_docs + 1) * 8] = np.frombuffer(np.asarray(doc_off, "<u8").tobytes(), np.uint8)
    return h.tobytes() + body.tobytes()
