"""The quality trim's cases (include/lime_hip.h states the rule at lime_quality_trim; lime_amd/csrc/lime_fqtrim_kernel.hip holds the kernels).
Two models of the rule: bounds_loop, the walk from either end, and bounds_closed, the closed form over the suffix / prefix sums in numpy.
Either takes one read's quality bytes and gives (lo, hi).  trim_model cuts a whole collection.  The hand-made quality patterns, the seeded
generators and a FASTQ writer that takes qualities follow.  tests/test_trim_cases_cpu.py holds the models against each other and against
lime_quality_trim without a GPU; tests/test_trim_edges_gpu.py holds the kernels against both."""
import numpy as np

SEED = 20313
FUZZ_CASES = 400
STEP = 256                                      # symbols a row of 16 lanes handles per step (TR_STEP); a lane holds 16
READS_PER_TRIP = 1536 * 16                      # TR_BLOCKS workgroups of TR_READS reads: the grid cap
LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097)
LONG = 70_001
RUNS = (1, 15, 16, 17, 63, 64, 65)
CUTOFFS = (0, 1, 20, 93)


# ---- the rule, twice ----
def bounds_loop(b, q5, q3):
    """the loop form: walk from the end, add q - q3, stop at the first sum above 0, keep the index of the strictly lowest sum; the 5' end alike"""
    q = [int(x) - 33 for x in bytes(b)]
    L = len(q)
    lo, hi = 0, L
    if q3:
        s = low = 0
        for i in range(L - 1, -1, -1):
            s += q[i] - q3
            if s > 0:
                break
            if s < low:
                low, hi = s, i
    if q5:
        s = high = 0
        for i in range(L):
            s += q5 - q[i]
            if s < 0:
                break
            if s > high:
                high, lo = s, i + 1
    return lo, hi


def bounds_closed(b, q5, q3):
    """the closed form: S(i) the suffix sums of q - q3, B the largest i with S(i) > 0, hi the largest argmin of S over (B, L) if that minimum
    is below 0; P(i) the prefix sums of q5 - q, E the smallest i with P(i) < 0, lo = 1 + the smallest argmax of P over [0, E) if above 0"""
    q = np.frombuffer(bytes(b), dtype=np.uint8).astype(np.int64) - 33
    L = len(q)
    lo, hi = 0, L
    if q3 and L:
        S = np.cumsum((q - q3)[::-1])[::-1]
        pos = np.nonzero(S > 0)[0]
        B = int(pos[-1]) if len(pos) else -1
        if B + 1 < L:
            tail = S[B + 1:]
            m = int(tail.min())
            if m < 0:
                hi = B + 1 + int(np.nonzero(tail == m)[0][-1])
    if q5 and L:
        P = np.cumsum(q5 - q)
        neg = np.nonzero(P < 0)[0]
        E = int(neg[0]) if len(neg) else L
        if E > 0:
            head = P[:E]
            M = int(head.max())
            if M > 0:
                lo = 1 + int(np.nonzero(head == M)[0][0])
    return lo, hi


def trim_model(reads, quals, q5, q3, bounds=bounds_closed):
    """lists of bytes -> (trimmed reads, info as lime_trim_info_t counts it)"""
    out, changed, emptied = [], 0, 0
    for r, b in zip(reads, quals):
        assert len(r) == len(b)
        lo, hi = bounds(b, q5, q3)
        t = bytes(r[lo:hi]) if lo < hi else b""
        changed += len(t) != len(r)
        emptied += len(r) != 0 and len(t) == 0
        out.append(t)
    return out, {"n_reads": len(reads), "n_changed": changed, "n_empty": emptied, "symbols_in": sum(len(r) for r in reads), "symbols_out": sum(len(t) for t in out)}


def records(docs):
    """list of bytes -> (text, doc_off)"""
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    if docs:
        off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), off


def fastq_of(reads, quals, eol=b"\n"):
    """four-line FASTQ of the reads with their quality strings"""
    return b"".join(b"@r%d" % k + eol + bytes(r) + eol + b"+" + eol + bytes(q) + eol for k, (r, q) in enumerate(zip(reads, quals)))


def bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def Q(v):
    """a quality value -> its Phred+33 byte"""
    return v + 33


# ---- hand-made quality patterns for one read of L symbols ----
def from_walk(vals, L, fill):
    """quality values in 3' walk order (the last symbol first), padded further in with `fill` -> the read's quality bytes"""
    vals = (list(vals) + [fill] * L)[:L]
    return bytes(Q(v) for v in reversed(vals))


def patterns(L, cut=20):
    """-> {name: quality bytes}, built around the cutoff `cut` (1 .. 78) so that each stresses one clause of the rule; a pattern named
    '... (5')' is the mirror image of its 3' form"""
    assert 1 <= cut <= 78
    good, low = cut + 15, max(cut - 15, 0)
    p = {}
    p["all above"] = bytes([Q(good)]) * L
    p["all below: both cuts take everything and cross"] = bytes([Q(low)]) * L
    p["all equal: sums of 0 cut nothing"] = bytes([Q(cut)]) * L
    p["bytes 33"] = bytes([33]) * L
    p["bytes 126"] = bytes([126]) * L
    for k in RUNS:
        if k <= L:
            p[f"low tail of {k}"] = from_walk([low] * k, L, good)
            p[f"low head of {k} (5')"] = p[f"low tail of {k}"][::-1]
            if 2 * k <= L:
                p[f"low head and tail of {k}"] = bytes([Q(low)]) * k + bytes([Q(good)]) * (L - 2 * k) + bytes([Q(low)]) * k
    if L >= 4:
        # the sums -1, 0, -1: two equal minima, the first one met stays: the larger index at 3', the smaller at 5'
        p["two equal minima"] = from_walk([cut - 1, cut + 1, cut - 1], L, good)
        p["two equal minima (5')"] = p["two equal minima"][::-1]
        p["equal values behind the minimum"] = from_walk([cut - 1, cut, cut, cut], L, good)
        p["equal values behind the minimum (5')"] = p["equal values behind the minimum"][::-1]
    # the early stop: the walk's sum is -1 from its first value, 0-valued symbols keep it there, value number d makes it +1 and stops the
    # walk; the low stretch further in must NOT be cut.  d - 1, the stopping index, on, one before and one behind every lane, row and step edge
    for d in sorted({1, 2, 15, 16, 17, 18, 31, 32, 33, 34, STEP - 1, STEP, STEP + 1, STEP + 2, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1, 2 * STEP + 2}):
        if d + 5 <= L:
            walk = [cut + 1] if d == 1 else [cut - 1] + [cut] * (d - 2) + [cut + 2]
            p[f"early stop on value {d}"] = from_walk(walk + [0] * 4, L, good)
            p[f"early stop on value {d} (5')"] = p[f"early stop on value {d}"][::-1]
    # a minimum deep in the read, behind sums that never turn positive: the cut reaches across steps
    for d in (17, STEP + 1, 3 * STEP + 5):
        if d + 2 <= L:
            p[f"a cut of {d}"] = from_walk([cut] * (d - 1) + [low], L, good)
            p[f"a cut of {d} (5')"] = p[f"a cut of {d}"][::-1]
    if L >= 3:
        h = L // 2                                                          # one good symbol in low ones: the 5' cut ends behind it, the 3' cut in front
        p["a 5' cut and a 3' cut that cross"] = bytes([Q(low)]) * h + bytes([Q(cut + 1)]) + bytes([Q(low)]) * (L - h - 1)
    assert all(len(v) == L for v in p.values())
    return p


def fuzz_read(rng, L):
    """one read's qualities: a mix of plateaus, tie-heavy alphabets and noise"""
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return rng.integers(33, 127, size=L, dtype=np.uint8).tobytes()
    if kind == 1:                                                           # tie-heavy: three values around 20
        return np.array([Q(19), Q(20), Q(21)], np.uint8)[rng.integers(0, 3, size=L)].tobytes()
    if kind == 2:                                                           # two values, long runs
        a = np.zeros(L, np.uint8)
        at, v = 0, int(rng.integers(0, 2))
        while at < L:
            k = int(rng.integers(1, 40))
            a[at:at + k] = Q(35) if v else Q(5)
            at += k; v ^= 1
        return a.tobytes()
    if kind == 3:
        return sample_quals(rng, L)
    return np.array([33, 34, 126, Q(20)], np.uint8)[rng.integers(0, 4, size=L)].tobytes()


def fuzz_collection(seed, case):
    """-> (reads, quals, q5, q3): 0 .. 40 reads of 0 .. 39 symbols, every 10th case with reads of up to 700, every 50th one read of some thousands"""
    rng = np.random.default_rng([seed, 3, case])
    n = int(rng.integers(0, 41))
    top = 40 if case % 10 != 9 else 700
    lens = [int(rng.integers(0, top)) for _ in range(n)]
    if case % 50 == 49:
        lens.append(int(rng.integers(3000, 9000)))
    quals = [fuzz_read(rng, L) for L in lens]
    reads = [bases(rng, L) for L in lens]
    cut = lambda: int(rng.choice([0, 1, 2, 10, 20, 21, 30, 40, 93]))
    return reads, quals, cut(), cut()


# ---- a sequencer-like generator: the middle 30 .. 40, low tails and heads ----
def sample_quals(rng, L):
    q = rng.integers(30, 41, size=L)
    u = rng.random()
    if u < 0.05:
        q[:] = rng.integers(2, 15, size=L)                                  # low throughout
    elif u < 0.10:
        keep = rng.choice(L, size=min(5, L), replace=False) if L else []
        low = rng.integers(2, 15, size=L)
        low[keep] = q[keep]
        q = low                                                             # low on all but 5 symbols
    elif u < 0.65:
        k = min(L, int(rng.integers(1, 61)))
        q[L - k:] = rng.integers(2, 15, size=k)                             # a low tail
        if rng.random() < 1 / 3:
            h = min(L, int(rng.integers(1, 9)))
            q[:h] = rng.integers(2, 15, size=h)                             # and a low head
    return (q + 33).astype(np.uint8).tobytes()


def sample_quals_for(reads, seed=7):
    rng = np.random.default_rng([SEED, 4, seed])
    return [sample_quals(rng, len(r)) for r in reads]
