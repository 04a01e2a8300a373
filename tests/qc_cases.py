"""The per-position read statistics (include/lime_hip.h: lime_read_qc) as two numpy models, hand-made cases with their tables written out, and
a seeded generator of collections.  The models work on lists of bytes (reads, and quality strings or None) and give the flat tables of
LIME_QC_WORDS(n_pos) uint64 words: row[p][8] for p in 0 .. n_pos (A, C, G, T, other, qsum, q20, q30; row n_pos pools every later position),
len_hist[n_pos + 1], gc_hist[101], mq_hist[256].
  qc_loop    read by read, symbol by symbol: the rule as it is stated.
  qc_vector  the whole collection at once: position indices of all symbols, np.add.at / bincount on (position, class).
The two are compared with each other on everything the tests use."""
import numpy as np

from tests.adapter_cases import fasta_of, fastq_of      # noqa: F401  (the same helpers)
from tests.trim_cases import records                    # noqa: F401

SEED = 20317
FUZZ_CASES = 400
WORD = 64                                       # symbols a wave handles per step
READS_PER_TRIP = 2048 * 4                       # RD_BLOCKS workgroups of RD_WAVES reads (lime_reads.h): the grid cap
MAX_POS = 512
N_POS = (1, 2, 63, 64, 65, 100, 255, 256, 511, 512)
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 5000)
Q20, Q30 = 53, 63                               # the raw quality bytes of Phred 20 and 30
CLASS = np.full(256, 4, dtype=np.int64)         # A C G T are 0 1 2 3 after & 0xDF; everything else is "other" (4)
for _k, _b in enumerate(b"ACGT"):
    CLASS[_b] = CLASS[_b | 0x20] = _k
KEYS = ("rows", "len_hist", "gc_hist", "mq_hist")


def words(n_pos):
    return 9 * (n_pos + 1) + 101 + 256


def split(t, n_pos):
    n = n_pos + 1
    return {"rows": t[:8 * n].reshape(n, 8), "len_hist": t[8 * n:9 * n], "gc_hist": t[9 * n:9 * n + 101], "mq_hist": t[9 * n + 101:]}


def qc_loop(reads, quals, n_pos):
    t = np.zeros(words(n_pos), dtype=np.uint64)
    s = split(t, n_pos)
    for k, r in enumerate(reads):
        q = None if quals is None else quals[k]
        gc = acgt = qs = 0
        for p, b in enumerate(bytes(r)):
            row = s["rows"][min(p, n_pos)]
            c = int(CLASS[b])
            row[c] += 1
            acgt += c < 4
            gc += c in (1, 2)
            if q is not None:
                row[5] += q[p]
                row[6] += q[p] >= Q20
                row[7] += q[p] >= Q30
                qs += q[p]
        s["len_hist"][min(len(r), n_pos)] += 1
        if acgt:
            s["gc_hist"][100 * gc // acgt] += 1
        if q is not None and len(r):
            s["mq_hist"][qs // len(r)] += 1
    return t


def qc_vector(reads, quals, n_pos):
    t = np.zeros(words(n_pos), dtype=np.uint64)
    s = split(t, n_pos)
    text, off = records([bytes(r) for r in reads])
    off = off.astype(np.int64)
    L = np.diff(off)
    n = len(reads)
    s["len_hist"][:] = np.bincount(np.minimum(L, n_pos), minlength=n_pos + 1).astype(np.uint64)
    if not len(text):                           # (no read with L >= 1: the length histogram is all there is)
        return t
    read_of = np.repeat(np.arange(n), L)
    pos = np.minimum(np.arange(len(text)) - off[read_of], n_pos)
    cls = CLASS[text]
    np.add.at(s["rows"], (pos, cls), 1)
    acgt = np.bincount(read_of, weights=cls < 4, minlength=n).astype(np.int64)
    gc = np.bincount(read_of, weights=(cls == 1) | (cls == 2), minlength=n).astype(np.int64)
    has = acgt > 0
    s["gc_hist"][:] = np.bincount(100 * gc[has] // acgt[has], minlength=101).astype(np.uint64)
    if quals is not None:
        q = np.frombuffer(b"".join(bytes(x) for x in quals), dtype=np.uint8).astype(np.int64)
        assert len(q) == len(text)
        np.add.at(s["rows"][:, 5], pos, q.astype(np.uint64))
        np.add.at(s["rows"][:, 6], pos, (q >= Q20).astype(np.uint64))
        np.add.at(s["rows"][:, 7], pos, (q >= Q30).astype(np.uint64))
        qs = np.bincount(read_of, weights=q, minlength=n).astype(np.int64)      # (exact: sums far below 2^53)
        some = L > 0
        s["mq_hist"][:] = np.bincount(qs[some] // L[some], minlength=256).astype(np.uint64)
    return t


def model(reads, quals, n_pos):
    """both models, which must agree -> the flat tables"""
    a, b = qc_loop(reads, quals, n_pos), qc_vector(reads, quals, n_pos)
    assert np.array_equal(a, b)
    return a


def flat(reads, quals):
    """lists of bytes -> (text, qual or None, doc_off) as the library takes them"""
    text, off = records([bytes(r) for r in reads])
    q = None if quals is None else np.frombuffer(b"".join(bytes(x) for x in quals), dtype=np.uint8).copy()
    return text, q, off


def invariants(t, n_pos, reads, with_qual):
    s = split(t, n_pos)
    assert int(s["rows"][:, :5].sum()) == sum(len(r) for r in reads)
    assert int(s["len_hist"].sum()) == len(reads)
    assert int(s["gc_hist"].sum()) == sum(1 for r in reads if (CLASS[np.frombuffer(bytes(r), dtype=np.uint8)] < 4).any())
    assert int(s["mq_hist"].sum()) == (sum(1 for r in reads if len(r)) if with_qual else 0)
    if not with_qual:
        assert not s["rows"][:, 5:].any()


# ---- the report as a dictionary, keys in the stated order (lime_qc_report_write) ----
def section(t, n_pos, with_qual):
    s = split(t, n_pos)
    rows = s["rows"]
    d = {"reads": int(s["len_hist"].sum()), "empty": int(s["len_hist"][0]), "symbols": int(rows[:, :5].sum()), "gc": int(rows[:, 1].sum() + rows[:, 2].sum()),
         "bases": {k: [int(x) for x in rows[:, c]] for c, k in enumerate(("A", "C", "G", "T", "other"))},
         "length_hist": [int(x) for x in s["len_hist"]], "gc_hist": [int(x) for x in s["gc_hist"]]}
    if with_qual:
        d.update({"q20": int(rows[:, 6].sum()), "q30": int(rows[:, 7].sum()), "qual_sum": [int(x) for x in rows[:, 5]], "qual_ge20": [int(x) for x in rows[:, 6]],
                  "qual_ge30": [int(x) for x in rows[:, 7]], "mean_qual_hist": [int(x) for x in s["mq_hist"]]})
    return d


def report(names, formats, n_pos, before, after):
    """formats: "fasta" / "fastq" per file; before, after: flat tables per file"""
    return {"lime_qc_report": 1, "positions": n_pos,
            "files": [{"file": n, "format": f, "before": section(b, n_pos, f == "fastq"), "after": section(a, n_pos, False)}
                      for n, f, b, a in zip(names, formats, before, after)]}


def key_order(pairs):
    """json.load(..., object_pairs_hook=key_order): dictionaries that remember nothing but also refuse a key given twice"""
    d = dict(pairs)
    assert len(d) == len(pairs)
    return d


# ---- hand-made cases: (name, reads, quals or None, n_pos, expected {key: array}) ----
def _expect(n_pos, rows, len_hist, gc_hist, mq_hist):
    """sparse: rows {(p, counter): v}, the histograms {index: v}"""
    t = np.zeros(words(n_pos), dtype=np.uint64)
    s = split(t, n_pos)
    for (p, c), v in rows.items():
        s["rows"][p, c] = v
    for h, d in (("len_hist", len_hist), ("gc_hist", gc_hist), ("mq_hist", mq_hist)):
        for k, v in d.items():
            s[h][k] = v
    return t


def hand_cases():
    cases = []
    # one read ACGTN, qualities on the thresholds, every position its own row
    cases.append(("one read, five rows", [b"ACGTN"], [bytes([52, 53, 62, 63, 255])], 5,
                  _expect(5, {(0, 0): 1, (1, 1): 1, (2, 2): 1, (3, 3): 1, (4, 4): 1, (0, 5): 52, (1, 5): 53, (2, 5): 62, (3, 5): 63, (4, 5): 255,
                              (1, 6): 1, (2, 6): 1, (3, 6): 1, (4, 6): 1, (3, 7): 1, (4, 7): 1},
                          {5: 1}, {50: 1}, {(52 + 53 + 62 + 63 + 255) // 5: 1})))
    # the same read at n_pos = 2: positions 2, 3, 4 pooled
    cases.append(("one read, pooled behind 2", [b"ACGTN"], [bytes([52, 53, 62, 63, 255])], 2,
                  _expect(2, {(0, 0): 1, (1, 1): 1, (2, 2): 1, (2, 3): 1, (2, 4): 1, (0, 5): 52, (1, 5): 53, (2, 5): 62 + 63 + 255,
                              (1, 6): 1, (2, 6): 3, (2, 7): 2},
                          {2: 1}, {50: 1}, {97: 1})))
    # lower case is its base; without qualities the quality counters stay 0
    cases.append(("lower case, no qualities", [b"acgt", b"GGCC", b""], None, 4,
                  _expect(4, {(0, 0): 1, (1, 1): 1, (2, 2): 1, (3, 3): 1, (0, 2): 1, (1, 2): 1, (2, 1): 1, (3, 1): 1},
                          {4: 2, 0: 1}, {50: 1, 100: 1}, {})))
    # reads without a base: counted in len_hist and the rows, nowhere in gc_hist; byte 0 and byte 255 are "other"
    cases.append(("no base", [b"NNN", bytes([0, 255]), b"-"], [bytes([0, 0, 0]), bytes([33, 32]), bytes([255])], 3,
                  _expect(3, {(0, 4): 3, (1, 4): 2, (2, 4): 1, (0, 5): 33 + 255, (1, 5): 32, (0, 6): 1, (0, 7): 1},
                          {3: 1, 2: 1, 1: 1}, {}, {0: 1, 32: 1, 255: 1})))
    # gc next to a whole percent: 1 of 3 -> 33, 2 of 3 -> 66; N's do not count in acgt
    cases.append(("gc by integer division", [b"CAT", b"GCA", b"NGNAN"], None, 1,
                  _expect(1, {(0, 1): 1, (0, 2): 1, (0, 4): 1, (1, 0): 3, (1, 3): 1, (1, 1): 1, (1, 2): 1, (1, 4): 2},
                          {1: 3}, {33: 1, 66: 1, 50: 1}, {})))
    # only empty reads, and no read at all
    cases.append(("empty reads", [b"", b"", b""], [b"", b"", b""], 7, _expect(7, {}, {0: 3}, {}, {})))
    cases.append(("no read", [], None, 64, _expect(64, {}, {}, {}, {})))
    return cases


def threshold_cases():
    """(name, reads, quals or None): what sits on a threshold of the rule, for every n_pos"""
    out = []
    for q in (0, 32, 33, 52, 53, 62, 63, 254, 255):
        out.append((f"quality byte {q}", [b"A" * 70], [bytes([q]) * 70]))
    out.append(("quality bytes mixed on the thresholds", [b"ACGT" * 40], [bytes([52, 53, 62, 63] * 40)]))
    for gc, n in ((1, 3), (2, 3), (50, 100), (99, 100), (1, 100), (100, 100), (0, 7), (199, 200), (1, 101)):
        out.append((f"gc {gc} of {n}", [b"G" * gc + b"A" * (n - gc)], None))
        out.append((f"gc {gc} of {n} among N", [b"N" + b"c" * gc + b"N" * 5 + b"t" * (n - gc)], None))
    for n_pos in N_POS:
        for L in {max(n_pos - 1, 0), n_pos, n_pos + 1}:
            out.append((f"L = {L} next to n_pos {n_pos}", [b"T" * L, b"C" * L], [bytes([40]) * L, bytes([70]) * L]))
    out.append(("mean quality by integer division", [b"AAA", b"AAAA"], [bytes([40, 40, 41]), bytes([41, 41, 41, 40])]))
    return out


# ---- the seeded generator ----
ALPHABET = np.frombuffer(b"ACGTACGTACGTACGTacgtacgtNNRYKMnry-." + bytes([0, 255, 11, 64, 91]), dtype=np.uint8)


def fuzz_read(rng, L):
    u = rng.random()
    if u < 0.08:
        s = rng.choice(np.frombuffer(b"NRYKMn-." + bytes([0, 255]), dtype=np.uint8), size=L)      # no base at all
    elif u < 0.16:
        s = rng.choice(np.frombuffer(b"GCgc", dtype=np.uint8), size=L)
    else:
        s = rng.choice(ALPHABET, size=L)
    return s.astype(np.uint8).tobytes()


def fuzz_qual(rng, L):
    u = rng.random()
    if u < 0.2:
        q = rng.integers(0, 256, size=L)
    elif u < 0.4:
        q = rng.choice(np.array([0, 32, 33, 52, 53, 62, 63, 255]), size=L)
    else:
        q = rng.integers(33, 75, size=L)
    q[q == 10] = 9                              # (a FASTQ line holds any byte but LF and CR)
    q[q == 13] = 14
    return q.astype(np.uint8).tobytes()


def fuzz_collection(seed, case):
    """-> (reads, quals or None, n_pos)"""
    rng = np.random.default_rng([seed, case])
    n_pos = int(N_POS[case % len(N_POS)]) if case % 3 else int(rng.integers(1, MAX_POS + 1))
    n = int(rng.integers(0, 13))
    edges = [0, 1, n_pos - 1, n_pos, n_pos + 1, 63, 64, 65, 128, 2 * n_pos + 3]
    reads = []
    for _ in range(n):
        u = rng.random()
        L = int(rng.choice(edges)) if u < 0.4 else int(rng.integers(0, 200)) if u < 0.9 else int(rng.integers(200, 1400))
        reads.append(fuzz_read(rng, max(L, 0)))
    quals = None if case % 4 == 3 else [fuzz_qual(rng, len(r)) for r in reads]
    return reads, quals, n_pos


def fuzz_yield(seed=SEED, cases=FUZZ_CASES):
    """what the generator must produce for the comparison to show anything"""
    long_reads = no_base = empty = no_qual = in_word = 0
    for case in range(cases):
        reads, quals, n_pos = fuzz_collection(seed, case)
        no_qual += quals is None
        for r in reads:
            long_reads += len(r) >= n_pos
            empty += len(r) == 0
            no_base += len(r) > 0 and not (CLASS[np.frombuffer(r, dtype=np.uint8)] < 4).any()
            in_word += len(r) > n_pos and n_pos % 64 != 0
    return {"long": long_reads, "no_base": no_base, "empty": empty, "no_qual": no_qual, "pool_in_word": in_word}
