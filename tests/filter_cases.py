"""The read filter's cases (include/lime_hip.h states the rule at lime_read_filter; lime_amd/csrc/lime_filter_kernel.hip holds the kernel).
Two models of the rule: keep_loop, the loops over every tail length and every symbol, and keep_words, the word form the kernel uses (the
read as 64-symbol words of class masks, the tail walked from the last word down with the carried misses and the early exit, the N's and the
equal neighbours by set bits).  Either takes one read and the parameters and gives (n, facts): what the read keeps and what was counted.
filter_model filters a whole collection.  The hand-made cases, a planting function and a seeded generator follow.
tests/test_filter_cases_cpu.py holds the models against each other and against lime_read_filter without a GPU;
tests/test_filter_edges_gpu.py holds the kernel against both."""
import numpy as np

from tests.adapter_cases import fasta_of, fastq_of      # (the same helpers)
from tests.trim_cases import bases, records

SEED = 20315
FUZZ_CASES = 400
WORD = 64                                       # symbols a wave handles per step
READS_PER_TRIP = 2048 * 4                       # RD_BLOCKS workgroups of RD_WAVES reads (lime_reads.h): the grid cap
LONG = 70_001
OFF = None                                      # max_n without a limit (LIME_FILTER_OFF)
A_, C_, G_, T_ = 1, 2, 4, 8                     # polyx_mask bits
MISS_RATES = (0.0, 0.05, 0.12, 0.125, 0.20)
INFO_KEYS = ("n_reads", "n_polyx", "n_capped", "n_short", "n_many_n", "n_low_complexity", "symbols_in", "symbols_out")
TRAP = b"G" * 500 + b"ACTACTACT" + b"G" * 55    # nine misses stop a first-run scan at t = 55; the rule cuts all 564: 8 * 9 <= 564


def params(polyx=0, polyx_min=10, max_len=0, min_len=0, max_n=OFF, min_complexity=0):
    """the parameters as api.read_filter and Context.docs_filter take them by keyword"""
    return {"polyx": polyx, "polyx_min": polyx_min, "max_len": max_len, "min_len": min_len, "max_n": max_n, "min_complexity": min_complexity}


def classes(s):
    """per symbol 0 .. 3 for A C G T (either case), 4 for every other byte"""
    return [b"ACGT".find(bytes([x & 0xDF])) % 5 for x in bytes(s)]    # (find gives -1 for other: -1 % 5 == 4)


# ---- the rule, twice ----
def tail_loop(c, mask, T):
    """t*: the largest t >= T at which the tail begins with X and holds at most t // 8 symbols that are not X, over the X of the mask"""
    L, best = len(c), 0
    for X in range(4):
        if not mask >> X & 1:
            continue
        mm = 0
        for t in range(1, L + 1):
            if c[L - t] != X:
                mm += 1
            elif t >= T and 8 * mm <= t and t > best:
                best = t
    return best


def keep_loop(s, p):
    """the loop form -> (n, facts): n the symbols kept (0 for an emptied read), facts the set of info fields the read is counted under"""
    c = classes(s)
    L = len(c)
    facts = set()
    if not L:
        return 0, facts
    t = tail_loop(c, p["polyx"], p["polyx_min"]) if p["polyx"] else 0
    if t:
        facts.add("n_polyx")
    n = L - t
    if p["max_len"] and n > p["max_len"]:
        n = p["max_len"]
        facts.add("n_capped")
    if n < p["min_len"]:
        return 0, facts | {"n_short"}
    if p["max_n"] is not None and sum(x == 4 for x in c[:n]) > p["max_n"]:
        return 0, facts | {"n_many_n"}
    d = sum(c[j] != c[j + 1] for j in range(n - 1))
    if n >= 2 and 100 * d < p["min_complexity"] * (n - 1):
        return 0, facts | {"n_low_complexity"}
    return n, facts


M64 = (1 << 64) - 1


def _low(k):
    return M64 if k >= 64 else (1 << k) - 1


def _words(c):
    """-> per 64-symbol word [R_A, R_C, R_G, R_T, valid]"""
    out = []
    for w in range((len(c) + 63) // 64):
        part = c[w * 64:w * 64 + 64]
        out.append([sum(1 << j for j, x in enumerate(part) if x == b) for b in range(4)] + [_low(len(part))])
    return out


def tail_words(W, L, mask, T):
    """the kernel's walk: from the last word down; bit j's misses are those at and above it in the word plus the carry; the word's lowest
    admissible bit is its longest tail; X leaves at the first word boundary with 8 * carry > L"""
    carry = [0, 0, 0, 0]
    live = mask
    best = L
    for w in range(len(W) - 1, -1, -1):
        if not live:
            break
        adm = 0
        for X in range(4):
            if not live >> X & 1:
                continue
            miss = ~W[w][X] & W[w][4]
            for j in range(64):
                if W[w][X] >> j & 1:
                    t = L - (w * 64 + j)
                    mm = bin(miss >> j).count("1") + carry[X]
                    if t >= T and 8 * mm <= t:
                        adm |= 1 << j
            carry[X] += bin(miss).count("1")
            if 8 * carry[X] > L:
                live &= ~(1 << X)
        if adm:
            best = w * 64 + (adm & -adm).bit_length() - 1
    return L - best


def keep_words(s, p):
    """the word form, in the kernel's order of work -> (n, facts) as keep_loop"""
    c = classes(s)
    L = len(c)
    facts = set()
    if not L:
        return 0, facts
    W = _words(c)
    n = L
    if p["polyx"]:
        t = tail_words(W, L, p["polyx"], p["polyx_min"])
        if t:
            facts.add("n_polyx")
        n -= t
    if p["max_len"] and n > p["max_len"]:
        n = p["max_len"]
        facts.add("n_capped")
    if n < p["min_len"]:
        return 0, facts | {"n_short"}
    if n and (p["max_n"] is not None or p["min_complexity"]):
        other = equal = 0
        for w in range((n + 63) // 64):
            cur = W[w][:4] + [~(W[w][0] | W[w][1] | W[w][2] | W[w][3]) & M64]
            nx = W[w + 1] if w + 1 < len(W) else [0, 0, 0, 0, 0]
            nxt = nx[:4] + [~(nx[0] | nx[1] | nx[2] | nx[3]) & M64]
            below = n - w * 64
            other += bin(cur[4] & _low(below)).count("1")
            eq = 0
            for b in range(5):
                eq |= cur[b] & ((cur[b] >> 1) | ((nxt[b] << 63) & M64))
            equal += bin(eq & _low(below - 1)).count("1")
        if p["max_n"] is not None and other > p["max_n"]:
            return 0, facts | {"n_many_n"}
        if n >= 2 and 100 * (n - 1 - equal) < p["min_complexity"] * (n - 1):
            return 0, facts | {"n_low_complexity"}
    return n, facts


def filter_model(reads, p, keep=keep_loop):
    """list of bytes -> (filtered reads, info as lime_filter_info_t counts it)"""
    info = {k: 0 for k in INFO_KEYS}
    out = []
    for r in reads:
        n, facts = keep(r, p)
        out.append(bytes(r[:n]))
        for f in facts:
            info[f] += 1
    info["n_reads"] = len(reads)
    info["symbols_in"] = sum(len(r) for r in reads)
    info["symbols_out"] = sum(len(t) for t in out)
    return out, info


# ---- planting ----
OTHERS = {ord("A"): b"CGT", ord("C"): b"AGT", ord("G"): b"ACT", ord("T"): b"ACG"}


def tail_of(rng, X, t, misses, first_is_x=True):
    """t symbols of base X (a byte such as b"G") with `misses` of them other bases at seeded places; the first one stays X if asked"""
    b = bytearray(X * t)
    places = np.arange(1 if first_is_x else 0, t)
    for j in rng.choice(places, size=min(misses, len(places)), replace=False) if misses else []:
        b[j] = OTHERS[X[0]][int(rng.integers(0, 3))]
    return bytes(b)


def plant(rng, read, t, X=b"G", rate=0.0):
    """the read's last t symbols replaced by a poly-X tail in which each symbol but the first misses with probability `rate`"""
    t = min(t, len(read))
    if not t:
        return bytes(read)
    miss = rng.random(t) < rate
    miss[0] = False
    tail = bytearray(X * t)
    for j in np.nonzero(miss)[0]:
        tail[j] = OTHERS[X[0]][int(rng.integers(0, 3))]
    return bytes(read[:len(read) - t]) + bytes(tail)


def no_tail(rng, L, X=b"G"):
    """L random bases none of which is one of X (one or more bases): whatever follows them, a tail of such a base ends in front of them or
    pays for every one of them"""
    rest = bytes(x for x in b"ACGT" if x not in X)
    return bytes(rest[int(k)] for k in rng.integers(0, len(rest), size=L))


def hand_cases():
    """-> {name: (reads, params)}; what each expects is written out in tests/test_filter_cases_cpu.py"""
    rng = np.random.default_rng([SEED, 1])
    body = no_tail(rng, 130)
    c = {}
    c["the trap"] = ([TRAP], params(G_))
    c["a clean tail"] = ([body[:100] + b"G" * 30, body[:100] + b"G" * 9, body[:100] + b"G" * 10], params(G_))
    c["a tail of another base is left"] = ([body[:100] + b"A" * 30], params(G_))
    ct = no_tail(rng, 90, b"AG")
    c["every base of the mask on its own"] = ([ct + b"A" * 20 + b"G" * 20, ct + b"AG" * 20, ct + b"G" * 20 + b"A" * 3], params(A_ | G_))
    c["the longest, not the first run"] = ([body[:60] + b"G" * 30 + b"AC" + b"G" * 10, body[:60] + b"G" * 12 + b"ACT" + b"G" * 10], params(G_))
    c["lower case"] = ([(body[:50] + b"G" * 20).lower(), body[:50] + b"g" * 20], params(G_))
    c["N in the tail is a miss"] = ([body[:50] + b"GGGGGGGGNGGGGGGG", body[:50] + b"GGGGNNGGGGGG"], params(G_))
    c["the whole read is the tail"] = ([b"G" * 64, b"g" * 65, b"G" * 10, b"G" * 9], params(G_))
    c["the cap"] = ([body[:100], body[:101], body[:99], body[:90] + b"G" * 40], params(G_, max_len=100))
    c["short"] = ([body[:30], body[:29], body[:20] + b"G" * 40, b""], params(G_, min_len=30))
    c["many N"] = ([b"ACGTNNACGT", b"ACGTNNNACGT", b"ACNNGT" + b"G" * 20 + b"NN", b"acgtnnnacgt", b"AC-R.GT"], params(G_, max_n=2))
    c["low complexity"] = ([b"A" * 50, b"AC" * 25, b"AAAC" * 25, b"N" * 40, b"ACGTTGCA" * 5 + b"A" * 60, b"A", b"AC", b"AA"], params(min_complexity=30))
    c["the first reason alone"] = ([b"A" * 20, b"N" * 20, b"N" * 40, b"A" * 40], params(min_len=30, max_n=5, min_complexity=30))
    c["every read empty"] = ([b""] * 5, params(G_, min_len=10, max_n=0, min_complexity=50))
    c["other bytes"] = ([body[:20] + bytes([0, 255, 0x47 | 0x80, ord("R"), ord("-")]) + b"G" * 30], params(G_, max_n=4))
    return c


def threshold_cases():
    """tails of t = 8k - 1, 8k, 8k + 1 symbols with k - 1, k, k + 1 misses at the end of a read of 200 whose other symbols are not X (G): the
    misses in the tail's last word, in its first word, or on both sides of a word boundary of the read; and the same with the tail's first
    symbol one of the misses, so that a shorter tail wins -> [(read, t, misses, first_is_x)].  Meant for T = 5"""
    rng = np.random.default_rng([SEED, 2])
    out = []
    for k in (1, 2, 8, 9, 16):
        for t in (8 * k - 1, 8 * k, 8 * k + 1):
            for m in (k - 1, k, k + 1):
                for where in ("last word", "first word", "word boundary", "first symbol"):
                    start = 200 - t
                    if where == "last word":
                        places = [t - 1 - 2 * i for i in range(m)]                      # from the read's end inwards, every second symbol
                    elif where == "first word":
                        places = [1 + 2 * i for i in range(m)]                          # behind the tail's first symbol
                    elif where == "word boundary":
                        edge = 128 if start < 127 else 192                              # bit 0 of a word, then bit 63 of the one in front, ...
                        places = [edge - start + (i // 2 if i % 2 == 0 else -1 - i // 2) for i in range(m)]
                    else:
                        places = [0] + [2 + 2 * i for i in range(m - 1)] if m else [-1]
                    lowest = 0 if where == "first symbol" else 1
                    if any(not lowest <= q < t for q in places) or len(set(places)) != m:
                        continue
                    tail = bytearray(b"G" * t)
                    for q in places:
                        tail[q] = ord("A")
                    out.append((no_tail(rng, start) + bytes(tail), t, m, where != "first symbol"))
    return out


# ---- seeded collections ----
def fuzz_read(rng, L):
    u = rng.random()
    if u < 0.45:                                  # a G-rich (sometimes A, C or T) tail at one of the miss rates around the rule's one in eight
        X = b"G" if rng.random() < 0.7 else bytes([b"ACT"[int(rng.integers(0, 3))]])
        r = plant(rng, bases(rng, L), int(rng.integers(0, L + 1)), X, MISS_RATES[int(rng.integers(0, len(MISS_RATES)))])
    elif u < 0.55:                                # homopolymer
        r = bytes([b"ACGT"[int(rng.integers(0, 4))]]) * L
    elif u < 0.65:                                # dinucleotide
        r = (bases(rng, 2) * (L // 2 + 1))[:L]
    else:
        r = bases(rng, L)
    if L and rng.random() < 0.3:                  # N runs
        b = bytearray(r)
        for _ in range(int(rng.integers(1, 4))):
            at, k = int(rng.integers(0, L)), int(rng.integers(1, 9))
            b[at:at + k] = b"N" * len(b[at:at + k])
        r = bytes(b)
    if rng.random() < 0.1:
        r = r.lower()
    return r


def fuzz_collection(seed, case):
    """-> (reads, params): 0 .. 30 reads of 0 .. 300 symbols (every 50th case one of some thousands), each parameter off in some cases"""
    rng = np.random.default_rng([seed, 3, case])
    n = int(rng.integers(0, 31))
    lens = [int(rng.integers(0, 301)) for _ in range(n)]
    if case % 50 == 49:
        lens.append(int(rng.integers(3000, 9000)))
    reads = [fuzz_read(rng, L) for L in lens]
    p = params(polyx=int(rng.choice([0, G_, G_, G_ | A_, 15, T_, C_])), polyx_min=int(rng.choice([1, 5, 10, 10, 20, 64, 255])),
               max_len=int(rng.choice([0, 0, 50, 100, 150, 255])), min_len=int(rng.choice([0, 0, 1, 20, 30, 100])),
               max_n=[OFF, OFF, 0, 1, 5, 20][int(rng.integers(0, 6))], min_complexity=int(rng.choice([0, 0, 1, 30, 50, 100])))
    if not (p["polyx"] or p["max_len"] or p["min_len"] or p["max_n"] is not None or p["min_complexity"]):
        p["polyx"] = G_                           # (nothing asked is a refusal)
    return reads, p
