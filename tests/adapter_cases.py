"""The adapter trim's cases (include/lime_hip.h states the rule at lime_adapter_trim; lime_amd/csrc/lime_adapter_kernel.hip holds the kernel).
Two models of the rule: keep_loop, the loop over every start p, and keep_masks, the bit-mask form the kernel uses (the read as four
arbitrary-precision bit words, one per base, against the adapter's four masks).  Either takes one read and gives p*, the number of
symbols the read keeps.  trim_model cuts a whole collection.  The hand-made cases, a seeded generator and the planting function follow.
tests/test_adapter_cases_cpu.py holds the models against each other and against lime_adapter_trim without a GPU;
tests/test_adapter_edges_gpu.py holds the kernel against both."""
import numpy as np

from tests.trim_cases import bases, records      # (the same helpers)

SEED = 20314
FUZZ_CASES = 400
WORD = 64                                       # symbols a wave handles per step
READS_PER_TRIP = 2048 * 4                       # RD_BLOCKS workgroups of RD_WAVES reads (lime_reads.h): the grid cap
LONG = 70_001
ADAPTER_LENGTHS = (1, 2, 31, 32, 33, 63, 64)
TRUSEQ_R1 = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
TRUSEQ_R2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
COMP = bytes.maketrans(b"ACGT", b"CATG")        # a base to a different base


def fold(b):
    return bytes(x & 0xDF for x in bytes(b))


# ---- the rule, twice ----
def keep_loop(s, a, O, E):
    """the loop form: the smallest p in [0, L) with k = min(M, L - p) >= O and at most (k * E) // 100 of the k places unequal; L without one"""
    s, a = fold(s), fold(a)
    L, M = len(s), len(a)
    for p in range(L):
        k = min(M, L - p)
        if k < O:
            break                                # (k only falls from here on)
        allow, mm = (k * E) // 100, 0
        for j in range(k):
            if s[p + j] != a[j]:
                mm += 1
                if mm > allow:
                    break
        else:
            return p
    return L


def keep_masks(s, a, O, E):
    """the bit-mask form: R_b = the read's places that hold base b as one long integer (no bit at or behind L), A_b the adapter's; the places
    that agree at start p are the set bits of (R_b >> p) & A_b summed over b, which counts the k overlapping places alone"""
    s, a = fold(s), fold(a)
    L, M = len(s), len(a)
    R = [sum(1 << i for i in range(L) if s[i] == b) for b in b"ACGT"]
    A = [sum(1 << j for j in range(M) if a[j] == b) for b in b"ACGT"]
    for p in range(L):
        k = min(M, L - p)
        same = sum(bin((R[b] >> p) & A[b]).count("1") for b in range(4))
        if k >= O and k - same <= (k * E) // 100:
            return p
    return L


def trim_model(reads, adapter, O, E, keep=keep_loop):
    """list of bytes -> (trimmed reads, info as lime_trim_info_t counts it)"""
    out = [bytes(r[:keep(r, adapter, O, E)]) for r in reads]
    return out, {"n_reads": len(reads), "n_changed": sum(len(t) != len(r) for t, r in zip(out, reads)),
                 "n_empty": sum(len(r) != 0 and len(t) == 0 for t, r in zip(out, reads)), "symbols_in": sum(len(r) for r in reads),
                 "symbols_out": sum(len(t) for t in out)}


# ---- planting ----
def with_errors(rng, a, n_err):
    """the adapter with n_err of its symbols changed to another base, at seeded places"""
    a = bytearray(a)
    for j in rng.choice(len(a), size=min(n_err, len(a)), replace=False) if n_err else []:
        a[j] = a[j:j + 1].translate(COMP)[0]
    return bytes(a)


def plant(rng, read, insert_len, adapter, n_err=0):
    """read-through: the read's insert cut at insert_len, then the adapter (n_err symbols of it changed) and filler bases, up to the read's
    original length.  An insert at least as long as the read leaves it as it is"""
    L = len(read)
    if insert_len >= L:
        return bytes(read)
    tail = with_errors(rng, adapter, n_err) + bases(rng, L)
    return (bytes(read[:insert_len]) + tail)[:L]


def far_from(rng, L, adapter, O, E):
    """L random bases that the rule leaves alone (redrawn where a chance hit shows)"""
    for _ in range(1000):
        s = bases(rng, L)
        if keep_loop(s, adapter, O, E) == L:
            return s
    raise AssertionError("no hit-free read found")


def hand_cases():
    """-> {name: (reads, adapter, O, E)}; what each expects is written out in tests/test_adapter_cases_cpu.py"""
    rng = np.random.default_rng([SEED, 1])
    a = TRUSEQ_R1[:20]
    c = {}
    body = far_from(rng, 130, a, 3, 0)
    # the adapter at every start of a read of 130 symbols: windows across the 63/64 and 127/128 word edges, partial overlaps at the end
    c["every start of 130"] = ([(body[:p] + a + bases(rng, 130))[:130] for p in range(130)], a, 3, 0)
    c["a full hit in the last word"] = ([body[:110] + a], a, 3, 0)
    last3 = far_from(rng, 97, a, 3, 0)
    c["a partial hit of exactly O"] = ([last3 + a[:3]], a, 3, 0)
    c["a partial hit of O - 1"] = ([last3 + a[:2]], a, 3, 0)
    # two hits: the leftmost wins
    c["two hits in one word"] = ([body[:10] + a + body[10:15] + a + body[:20]], a, 3, 0)
    c["two hits in different words"] = ([body[:40] + a + body[40:70] + a + body[:20]], a, 3, 0)
    # in front, at place 35, the adapter's first 5 symbols and then other bases: inside the read the overlap there is the whole adapter, so 5
    # right symbols of 20 are no hit; the whole adapter follows at place 70, in the next word
    c["a later full hit behind an earlier partial non-hit"] = ([body[:30] + a[:10].translate(COMP)[:5] + a[:5] + body[30:60] + a], a, 3, 0)
    c["a hit at 0"] = ([a + body[:50], a, a[:5]], a, 3, 0)
    c["every read empty"] = ([b""] * 5, a, 3, 10)
    c["lower case"] = ([(body[:33] + a + body[:9]).lower(), body[:70] + a.lower()], a.lower(), 3, 0)
    c["N inside the occurrence"] = ([body[:50] + a[:7] + b"N" + a[8:], body[:50] + a[:7] + b"N" + a[8:12] + b"N" + a[13:]], a, 3, 5)
    c["a read of only N"] = ([b"N" * 100, b"n" * 64, b"N"], a, 1, 50)
    c["other bytes"] = ([body[:20] + bytes([0, 255, 0x41 | 0x80, ord("R"), ord("-")]) + a], a, 3, 0)
    return c


def threshold_cases():
    """mismatch counts of exactly (k * E) // 100 and one more, at E of 0, 10 and 50: the occurrence at place 70 of a read, whole (k = M = 30)
    and cut by the read's end at every k at which one symbol more moves k * E across a multiple of 100 (and the k next to them)
    -> {name: (read, adapter, O, E, k, n_err)}; place 70 is a hit exactly when n_err <= (k * E) // 100"""
    rng = np.random.default_rng([SEED, 2])
    a = TRUSEQ_R1[:30]
    c = {}
    for E in (0, 10, 50):
        edges = {k for k in range(4, 31) if (k * E) // 100 != ((k - 1) * E) // 100}
        for k in sorted(edges | {k - 1 for k in edges} | {3, 30}):
            allow = (k * E) // 100
            for n_err in (allow, allow + 1):
                body = far_from(rng, 70, a, 3, E)
                c[f"E {E} k {k} errors {n_err}"] = (body + with_errors(rng, a[:k], n_err) + (bases(rng, 25) if k == 30 else b""), a, 3, E, k, n_err)
    return c


def hits_at(s, a, O, E, p):
    """is start p a hit? (the rule's clause for one p, written out once more)"""
    s, a = fold(s), fold(a)
    k = min(len(a), len(s) - p)
    return k >= O and sum(s[p + j] != a[j] for j in range(k)) <= (k * E) // 100


# ---- seeded collections ----
def fuzz_collection(seed, case):
    """-> (reads, adapter, O, E): 0 .. 40 reads of 0 .. 300 symbols (every 50th case one of some thousands), an adapter of 1 .. 64, about two
    thirds of the reads with the adapter planted with 8 % errors, some lower case, some N"""
    rng = np.random.default_rng([seed, 3, case])
    M = int(rng.integers(1, 65)) if case % 4 else int(rng.choice(ADAPTER_LENGTHS))
    adapter = bases(rng, M)
    O = int(rng.integers(1, M + 1)) if case % 3 == 0 else min(M, int(rng.integers(1, 6)))
    E = int(rng.choice([0, 5, 10, 20, 33, 50])) if case % 5 else int(rng.integers(0, 51))
    n = int(rng.integers(0, 41))
    lens = [int(rng.integers(0, 301)) for _ in range(n)]
    if case % 50 == 49:
        lens.append(int(rng.integers(3000, 9000)))
    reads = []
    for L in lens:
        r = bases(rng, L)
        if L and rng.random() < 0.67:
            r = plant(rng, r, int(rng.integers(0, L)), adapter, int(rng.binomial(M, 0.08)))
        u = rng.random()
        if u < 0.1:
            r = r.lower()
        elif u < 0.25 and L:
            b = bytearray(r)
            for j in rng.choice(L, size=min(L, 3), replace=False):
                b[j] = ord("N")
            r = bytes(b)
        reads.append(r)
    if case % 7 == 3:
        adapter = adapter.lower()
    return reads, adapter, O, E


def fasta_of(reads):
    return b"".join(b">r%d\n" % k + bytes(r) + b"\n" for k, r in enumerate(reads))


def fastq_of(reads, quals=None, eol=b"\n"):
    quals = quals or [b"I" * len(r) for r in reads]
    return b"".join(b"@r%d" % k + eol + bytes(r) + eol + b"+" + eol + bytes(q) + eol for k, (r, q) in enumerate(zip(reads, quals)))
