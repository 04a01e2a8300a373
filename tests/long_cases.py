"""Collections for the long clusters' scorer, k_score_big (lime_kernels.hip), at the edges of its own arithmetic and data structure:
counts on the 255 / 256 border, pair scores that are multiples of 256, probe chains of its hash table that wrap past the last slot, a table
at the load it is sized for, more pair records than the exchange's list holds, and a table region that only long clusters write to.
tests/test_long_cases_cpu.py shows without a GPU that every generator has what it states, tests/test_long_edges_gpu.py runs them through
the three routes the long clusters' updates leave by.  Everything is seeded, pure numpy, alpha 16.

Every generator returns (lcp, da, ebwt, n_reads, n_refs, facts).  A cluster of L symbols is a position with lcp 0 followed by L - 1 positions
with lcp >= 16 (src/ClusterLCP.cpp:214-227: the run is opened at the position before the first lcp >= alpha)."""
import numpy as np

ALPHA = 16
HT_BITS = 17                                   # lime_kernels.h: HT_BITS, HT_SIZE, BIG_GRID, SMALL_MAX; lime_kernels.hip: MID_MAX; lime_pass.cpp: bigrec_cap
HT_SIZE = 1 << HT_BITS
HT_MULT = 2654435761
BIG_GRID = 32
SMALL_MAX, MID_MAX = 16, 64
BIGREC_CAP = 16 << 20
MAX_CLUSTER = 65536
A = ord("A")


def ht_hash(doc):
    """k_score_big's home slot of a document: (doc * 2654435761 mod 2^32) >> (32 - HT_BITS)"""
    return ((np.asarray(doc, dtype=np.uint64) * np.uint64(HT_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HT_BITS)


def probe(docs):
    """linear probing as k_score_big does it, in Python, documents inserted in the given order -> {doc: slot}, and whether any probe stepped
    from the last slot to slot 0.  (On the device the order within a cluster is whatever the lanes make it: the SET of slots a chain fills does
    not depend on it, who sits where does.)"""
    slot_of, taken, wrapped = {}, set(), False
    for d in docs:
        d = int(d)
        if d in slot_of:
            continue
        h = int(ht_hash(d))
        while h in taken:
            wrapped |= h == HT_SIZE - 1
            h = (h + 1) & (HT_SIZE - 1)
        taken.add(h)
        slot_of[d] = h
    return slot_of, wrapped


class _Builder:
    """positions appended cluster by cluster; between clusters the lcp is 0"""

    def __init__(self, rng):
        self.rng, self.lcp, self.da, self.eb, self.clusters = rng, [], [], [], []
        self.n = 0

    def cluster(self, da, eb=None, shuffle=True):
        da = np.asarray(da, dtype=np.uint32)
        eb = np.full(len(da), A, np.uint8) if eb is None else np.asarray(eb, dtype=np.uint8)
        if shuffle:
            o = self.rng.permutation(len(da))
            da, eb = da[o], eb[o]
        lcp = (ALPHA + self.rng.integers(0, 40, len(da))).astype(np.uint32)
        lcp[0] = int(self.rng.integers(0, ALPHA))
        if self.n == 0:
            lcp[0] = 0
        self.clusters.append((self.n, len(da)))
        self.lcp.append(lcp); self.da.append(da); self.eb.append(eb)
        self.n += len(da)

    def singles(self, da):
        """positions that belong to no cluster"""
        da = np.asarray(da, dtype=np.uint32)
        self.lcp.append(self.rng.integers(0, ALPHA, len(da)).astype(np.uint32) if self.n else np.zeros(len(da), np.uint32))
        self.da.append(da); self.eb.append(np.full(len(da), A, np.uint8))
        self.n += len(da)

    def arrays(self):
        lcp = np.concatenate(self.lcp).astype(np.uint32)
        lcp[0] = 0
        return lcp, np.concatenate(self.da).astype(np.uint32), np.concatenate(self.eb).astype(np.uint8)

    def cluster_list(self):
        return np.array(self.clusters, dtype=np.uint64).reshape(-1, 2)


def _from_counts(spec):
    """{doc: {symbol byte: count}} -> (da, ebwt) of one cluster, unshuffled"""
    da, eb = [], []
    for doc, syms in spec.items():
        for s, c in syms.items():
            da.append(np.full(c, doc, np.uint32)); eb.append(np.full(c, ord(s), np.uint8))
    return np.concatenate(da), np.concatenate(eb)


# ---- count_edges ------------------------------------------------------------------------------------------------------------------------
# 18 read and 18 genome "names" (indices 0 .. 17 on either side); a cluster is ({read name: {symbol: count}}, {genome name: {symbol: count}}).
# The first three hold one symbol only, so that per-document and per-symbol counts are the same thing and both builds see the borders:
COUNT_EDGES_NAMES = 18
_BASE = [
    # reads at 254 .. 257 against genomes at 254, 255, 256 (saturated: 255) and 300 (saturated): both orders; the read at 256 counts as 0
    ({0: {"A": 254}, 1: {"A": 255}, 2: {"A": 256}, 3: {"A": 257}}, {0: {"A": 254}, 1: {"A": 255}, 2: {"A": 256}, 3: {"A": 300}}),
    # reads at 511 (255), 512 (0), 513 (1); a genome far below the reads, one on the border, one beyond it
    ({0: {"A": 511}, 1: {"A": 512}, 2: {"A": 513}}, {1: {"A": 255}, 3: {"A": 3}, 0: {"A": 300}}),
    # a read at 256 against small genomes (scores nothing), a small read beside it
    ({3: {"A": 256}, 1: {"A": 2}}, {2: {"A": 254}, 3: {"A": 1}}),
]
# the clusters that need several symbols (EBWT=1).  Names 4 .. 13 occur in one cluster each, so a cell of theirs has one update:
_SPREAD = [
    # t = 128 + 128 = 256 for (read 4, genome 4): not zero for the kernel's `if (t)`, zero in the reference's unsigned char
    ({4: {"A": 128, "C": 128}, 5: {"A": 1}}, {4: {"A": 128, "C": 128}, 5: {"G": 5}, 6: {"A": 3}}),
    # t = 255 + 255 + 5 = 512 + 3 for (read 6, genome 7), through a saturated count; read 7 / genome 8: the borders symbol by symbol
    ({6: {"A": 255, "C": 255, "G": 5}, 7: {"A": 256, "C": 257, "G": 254, "T": 255}},
     {7: {"A": 255, "C": 300, "G": 5}, 8: {"A": 254, "C": 255, "G": 256, "T": 300}}),
    # per-symbol read counts 511 / 512 / 513 -> 255 + 0 + 1 = 256 again
    ({8: {"A": 511, "C": 512, "G": 513}, 9: {"T": 2}}, {9: {"A": 255, "C": 255, "G": 255}, 10: {"T": 7, "A": 4}}),
    # IUPAC symbols beside a saturated genome count: the cross-match's remainders (ClusterBWT_DA.cpp:146-177) start from 255 - count
    ({10: {"A": 100, "R": 3, "Y": 2, "N": 7, "G": 6}, 11: {"R": 260, "C": 9, "N": 1}},
     {11: {"A": 300, "R": 10, "N": 4}, 12: {"G": 256, "Y": 5, "C": 2, "N": 255}}),
    ({12: {"N": 257, "A": 2}, 13: {"Y": 255, "T": 1}}, {13: {"T": 300, "C": 254, "N": 3}, 14: {"A": 255, "G": 255, "R": 256}}),
]
# cells (read name, genome name) whose value can be written down from the counts above: {cell: (EBWT=0 build, EBWT=1 build)}.
# EBWT=0: t = min(read count mod 256, min(genome count, 255)); EBWT=1 without IUPAC symbols: the sum of that over the symbols, mod 256.
# Names 0 .. 3 meet in several clusters: their cells are the sums, mod 256.
COUNT_EDGES_BY_HAND_BASE = {                      # count_edges(False), and the EBWT=1 build of it (one symbol: the same numbers)
    # cluster 1: read 0 (254): 254, 254, 254, 254; read 1 (255): 254, 255, 255, 255; read 2 (0): nothing; read 3 (1): 1, 1, 1, 1
    # cluster 2: read 0 (255) x genomes 1, 3, 0 = 255, 3, 255; read 1 (0): nothing; read 2 (1): 1, 1, 1
    # cluster 3: read 3 (0): nothing; read 1 (2) x genomes 2, 3 = 2, 1
    (0, 0): (254 + 255) % 256, (0, 1): (254 + 255) % 256, (0, 2): 254, (0, 3): (254 + 3) % 256,
    (1, 0): 254, (1, 1): 255, (1, 2): (255 + 2) % 256, (1, 3): (255 + 1) % 256,
    (2, 0): 1, (2, 1): 1, (2, 2): 0, (2, 3): 1,
    (3, 0): 1, (3, 1): 1, (3, 2): 1, (3, 3): 1,
}
COUNT_EDGES_BY_HAND_SPREAD = {                    # count_edges(True): {cell: (EBWT=0, EBWT=1)}
    (4, 4): (0, 0),                               # 256 symbols each: 0 / t = 256
    (4, 5): (0, 0), (4, 6): (0, 3),               # read 4 counts 0 without symbols; A: min(128, 3)
    (5, 4): (1, 1), (5, 5): (1, 0), (5, 6): (1, 1),
    (6, 7): ((515 % 256), 3),                     # min(515 % 256 = 3, 255) = 3; 255 + 255 + 5 = 515 -> 3
    (6, 8): (3, (254 + 255 + 5) % 256),
    (7, 7): (min(1022 % 256, 255), 0 + 1 + 5 + 0),
    (7, 8): (min(1022 % 256, 255), (0 + 1 + 254 + 255) % 256),
    (8, 9): (0, 0),                               # 1536 % 256 = 0 / 255 + 0 + 1 = 256
    (8, 10): (0, 4), (9, 9): (2, 0), (9, 10): (2, 2),   # A: min(511 % 256, 4) keeps read 8's row in the lists
}
T256_CELLS = ((4, 4), (8, 9))                     # their only update is a t of 256
_IUPAC = b"ACGTRYSWKMBDHVN"


def count_edges(ebwt_on, n_reads=COUNT_EDGES_NAMES, n_refs=COUNT_EDGES_NAMES, seed=4101):
    """Clusters whose per-document occurrence counts sit on the borders of the reference's unsigned chars: reads at 254, 255, 256, 257, 511,
    512, 513 (they wrap), genomes at 254, 255, 256, 300 (they saturate), in both orders.  ebwt_on adds the clusters that spread such counts over
    symbols: per-symbol borders, two pairs with t = 256, one with t = 512 + 3, two clusters with IUPAC symbols beside saturated counts.  Between
    them short clusters of 2 .. 18 symbols over four further names, among them several of 15, 16, 17 and 18 (the list flow's SMALL_MAX border).
    n_reads / n_refs beyond 18 spread the 18 names evenly over a larger table (name k = document k * (n // 18)): the same counts on a table of
    several regions.  facts: clusters = [(start, length, {doc: {symbol index byte: count}})] in position order, read_of / genome_of = name ->
    document id / genome index."""
    assert n_reads >= COUNT_EDGES_NAMES and n_refs >= COUNT_EDGES_NAMES
    rng = np.random.default_rng(seed)
    rs, gs = n_reads // COUNT_EDGES_NAMES, n_refs // COUNT_EDGES_NAMES
    read_of = lambda k: k * rs
    genome_of = lambda k: k * gs
    b = _Builder(rng)
    specs = []

    def filler(length):
        # names 14 .. 17 (reads) and 15 .. 17 (genomes); at least one of each side
        docs = np.concatenate([[read_of(int(rng.integers(14, 18)))], [n_reads + genome_of(int(rng.integers(15, 18)))],
                               np.where(rng.random(length - 2) < 0.5, rs * rng.integers(14, 18, length - 2), n_reads + gs * rng.integers(15, 18, length - 2))])
        eb = rng.choice(np.frombuffer(_IUPAC if ebwt_on else b"A", np.uint8), length)
        b.cluster(docs, eb)

    def fillers(lengths):
        for L in lengths:
            filler(int(L))
            b.singles(rng.integers(0, n_reads + n_refs, int(rng.integers(0, 3))))

    fillers([15, 16, 17, 18, 2, 3])
    for reads, genomes in _BASE + (_SPREAD if ebwt_on else []):
        spec = {read_of(k): v for k, v in reads.items()}
        spec.update({n_reads + genome_of(k): v for k, v in genomes.items()})
        b.cluster(*_from_counts(spec))
        specs.append(spec)
        fillers(np.concatenate([[15, 16, 17, 18], rng.integers(2, 15, 12 if ebwt_on else 30)]))
    lcp, da, eb = b.arrays()
    facts = dict(clusters=b.cluster_list(), edge_specs=specs, read_of=read_of, genome_of=genome_of,
                 by_hand={**{c: (v, v) for c, v in COUNT_EDGES_BY_HAND_BASE.items()}, **(COUNT_EDGES_BY_HAND_SPREAD if ebwt_on else {})},
                 t256_cells=T256_CELLS if ebwt_on else ())
    return lcp, da, eb, n_reads, n_refs, facts


# ---- hash_chains ------------------------------------------------------------------------------------------------------------------------
def _side_with_a_document_in_the_chain(lo, hi):
    """the n in [lo, hi) closest to hi for which one of the 8 document ids n .. n + 7 has its home in the last three slots or in 0 .. 30"""
    for n in range(hi - 1, lo - 1, -1):
        h = ht_hash(np.arange(n, n + 8))
        if ((h >= HT_SIZE - 3) | (h <= 30)).any():
            return n
    raise AssertionError("no such size")


def hash_chains(crafted="reads", seed=4102):
    """k_score_big's open-addressing table where linear probing is at work.  Cluster A (about 300 symbols): every document of a range of about
    2^21 whose home is one of the last three slots (at least 40: their chain runs on over slot 0), 20 documents with homes in slots 0 .. 30 (which
    that chain pushes on), and the few documents of the other side, of which one has its home inside the chain as well.  crafted = "reads": a
    table of about 2^21 x 8, the crafted documents are reads; "genomes": 8 x 2^21.  Then 72 clusters of 65 .. 90 symbols (more than twice
    BIG_GRID: every workgroup of k_score_big takes several in turn, each after it has put its table back to empty), each drawn in another
    order from one pool of 200 colliding documents, so that a key or a counter left behind by one changes a score of the next."""
    rng = np.random.default_rng(seed)
    if crafted == "reads":
        n_reads = _side_with_a_document_in_the_chain((1 << 21) - (1 << 16), (1 << 21) + 1)
        n_refs, base, n_crafted = 8, 0, n_reads                          # crafted document id = base + k, k < n_crafted
        others = n_reads + np.arange(8)
    else:
        n_reads, n_refs, base, n_crafted = 8, 1 << 21, 8, 1 << 21        # (read 0 has its home in slot 0)
        others = np.arange(8)
    ids = base + np.arange(n_crafted, dtype=np.uint64)
    h = ht_hash(ids)
    tail = ids[h >= HT_SIZE - 3]
    near = ids[h <= 30]
    pushed = rng.choice(near, 20, replace=False)
    pool = np.concatenate([tail, rng.permutation(ids[h <= 12])])[:200]   # the 200 colliding documents: the tail's and homes 0 .. 12
    assert len(tail) >= 40 and len(pool) == 200
    b = _Builder(rng)
    # cluster A: every chain document 2 .. 5 times, the other side's 8 documents 3 .. 6 times
    docs_a = np.concatenate([tail, pushed])
    b.singles(rng.integers(0, n_reads + n_refs, 5))
    da_a = np.concatenate([np.repeat(docs_a, rng.integers(2, 6, len(docs_a))), np.repeat(others, rng.integers(3, 7, 8))])
    b.cluster(da_a, rng.choice(np.frombuffer(b"ACGTN", np.uint8), len(da_a)))
    cluster_a = b.clusters[-1]
    lens = []
    for _ in range(72):
        b.singles(rng.integers(0, n_reads + n_refs, int(rng.integers(1, 4))))
        L = int(rng.integers(65, 91))
        k_other = int(rng.integers(2, 9))
        take = rng.permutation(pool)[:int(rng.integers(30, 60))]
        docs = np.concatenate([rng.choice(others, k_other), rng.choice(take, L - k_other)])
        b.cluster(docs, rng.choice(np.frombuffer(b"ACGTRYN", np.uint8), L))
        lens.append(L)
    lcp, da, eb = b.arrays()
    facts = dict(clusters=b.cluster_list(), cluster_a=cluster_a, tail=tail, pushed=pushed, pool=pool, others=others, crafted=crafted)
    return lcp, da, eb, n_reads, n_refs, facts


# ---- full_load ---------------------------------------------------------------------------------------------------------------------------
def full_load(seed=4103):
    """One cluster of exactly 65 536 symbols (LIME_MAX_CLUSTER) with 65 536 distinct documents, 65 000 reads and 536 genomes once each: the
    load of 0.5 k_score_big's table is sized for.  34 840 000 pairs, every score 1 (all symbols 'C'), a table of 34.8 MB."""
    rng = np.random.default_rng(seed)
    n_reads, n_refs = 65000, 536
    b = _Builder(rng)
    b.singles([3, n_reads + 1])
    b.cluster(np.arange(MAX_CLUSTER), np.full(MAX_CLUSTER, ord("C"), np.uint8))
    b.singles([7])
    lcp, da, eb = b.arrays()
    return lcp, da, eb, n_reads, n_refs, dict(clusters=b.cluster_list(), pairs=n_reads * n_refs)


# ---- record_list_overflow -----------------------------------------------------------------------------------------------------------------
def record_list_overflow(seed=4104):
    """One cluster of 8 400 symbols, 4 200 reads and 4 200 genomes once each: 17 640 000 pair records, more than the 16 * 2^20 the exchange's
    list of long-cluster records holds before lime_get_stats regrows it.  All symbols 'A'.  Before and after it short clusters in groups of
    256 equal ones (1 536 + 1 280 symbols): ordinary update records for the repeated pass to make again, and every cell they touch receives
    256 * 1 = 0 modulo 256 -- so the table is 1 everywhere, in both builds."""
    rng = np.random.default_rng(seed)
    n_reads = n_refs = 4200
    g = lambda k: n_reads + k
    b = _Builder(rng)
    for _ in range(256):
        b.cluster([17, g(4000)], shuffle=False)
    for _ in range(256):
        b.cluster([2500, g(7), g(4199), 2500], shuffle=False)                   # read count 2 against genome counts 1: t = 1 twice
    n_short = 2 * 256
    b.singles([5, g(5)])
    b.cluster(np.arange(2 * n_reads))
    long_cluster = b.clusters[-1]
    b.singles([g(9)])
    for _ in range(256):
        b.cluster([4199, g(0), g(2100), g(2101), 0], shuffle=False)
    lcp, da, eb = b.arrays()
    return lcp, da, eb, n_reads, n_refs, dict(clusters=b.cluster_list(), long_cluster=long_cluster, pairs=n_reads * n_refs,
                                              short_updates=256 * (1 + 2 + 6))


# ---- lonely_region ------------------------------------------------------------------------------------------------------------------------
def lonely_region(seed=4105):
    """A table of 1000 x 300 bytes = 4.6 regions of 64 KB.  Every short cluster (2 .. 14 symbols) holds reads below 200 only: rows inside the
    first region.  One long cluster of 100 symbols holds reads from 900 on: rows inside the last region, which so receives long-cluster records
    and not one record from the scan; the regions between receive nothing."""
    rng = np.random.default_rng(seed)
    n_reads, n_refs = 1000, 300
    b = _Builder(rng)

    def shorts(k):
        for _ in range(k):
            L = int(rng.integers(2, 15))
            docs = np.concatenate([[int(rng.integers(0, 200))], [n_reads + int(rng.integers(0, n_refs))],
                                   np.where(rng.random(L - 2) < 0.5, rng.integers(0, 200, L - 2), n_reads + rng.integers(0, n_refs, L - 2))])
            b.cluster(docs, rng.choice(np.frombuffer(b"ACGT", np.uint8), L))
            b.singles(rng.integers(0, 200, int(rng.integers(0, 3))))
    shorts(300)
    docs = np.concatenate([rng.integers(900, n_reads, 45), n_reads + rng.integers(0, n_refs, 55)])
    b.cluster(docs, rng.choice(np.frombuffer(b"ACGT", np.uint8), 100))
    long_cluster = b.clusters[-1]
    b.singles([3])
    shorts(300)
    lcp, da, eb = b.arrays()
    return lcp, da, eb, n_reads, n_refs, dict(clusters=b.cluster_list(), long_cluster=long_cluster, region_bytes=1 << 16)


def small_max_border(seed=4106):
    """The list flow alone scores clusters of up to SMALL_MAX = 16 symbols in k_score_list and hands longer ones to k_score_big: clusters of
    15, 16, 17 and 18 symbols, forty of each, over count_edges' 18 + 18 documents with many repeats."""
    rng = np.random.default_rng(seed)
    n_reads = n_refs = COUNT_EDGES_NAMES
    b = _Builder(rng)
    for L in rng.permutation(np.repeat([15, 16, 17, 18], 40)):
        L = int(L)
        docs = np.concatenate([[int(rng.integers(0, 4))], [n_reads + int(rng.integers(0, 4))], rng.integers(0, 8, L - 2) % 4 + np.where(rng.random(L - 2) < 0.5, 0, n_reads)])
        b.cluster(docs, rng.choice(np.frombuffer(_IUPAC, np.uint8), L))
        b.singles(rng.integers(0, n_reads + n_refs, int(rng.integers(0, 3))))
    lcp, da, eb = b.arrays()
    return lcp, da, eb, n_reads, n_refs, dict(clusters=b.cluster_list())


def model_table(da, eb, clusters, n_reads, n_refs, ebwt_on, O=None):
    """The table from per-cluster counts, the plain way: per cluster np.unique counts per document (and symbol), read counts mod 256, genome
    counts saturated at 255; EBWT=0: t = min of the two; EBWT=1: O.pair_score(read counts[16], genome counts[16]) over O.sym_index's symbol classes (O = oracle.oracle_py:
    the restatement of ClusterBWT_DA.cpp:129-184 for ONE pair, which the goldens pin).  Small collections only."""
    sim = np.zeros((n_reads, n_refs), np.int64)
    for s, L in np.asarray(clusters, dtype=np.int64):
        d = da[s:s + L].astype(np.int64)
        if not ebwt_on:
            docs, cnt = np.unique(d, return_counts=True)
            for r, cr in zip(docs[docs < n_reads], cnt[docs < n_reads]):
                for g, cg in zip(docs[docs >= n_reads], cnt[docs >= n_reads]):
                    sim[r, g - n_reads] += min(int(cr) % 256, min(int(cg), 255))
        else:
            sym = np.array([O.sym_index(int(x)) for x in eb[s:s + L]], dtype=np.int64)
            docs = np.unique(d)
            counts = {int(k): np.bincount(sym[d == k], minlength=16) for k in docs}
            for r in docs[docs < n_reads]:
                cr = (counts[int(r)] % 256).astype(np.uint8)
                for g in docs[docs >= n_reads]:
                    cg = np.minimum(counts[int(g)], 255).astype(np.uint8)
                    sim[r, g - n_reads] += O.pair_score(cr, cg)
    return (sim % 256).astype(np.uint8)
