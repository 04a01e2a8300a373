"""The overlap cut's cases (include/lime_hip.h states the rule at lime_pair_overlap_trim; lime_amd/csrc/lime_overlap_kernel.hip holds the kernel).
Two models of the rule: insert_loop, the loop over the places of every candidate I as the rule is written, and insert_masks, a closed form on
Python integers used as bit masks, one per class: mate 1 as it is, mate 2 as its reverse complement, a candidate as a shift of one against
the other.  Either takes the two mates of a pair and gives I*, or 0.  cut_model cuts two whole collections.  The planting function, the
hand-made cases, the threshold cases, the trap and a seeded generator follow.
tests/test_overlap_cases_cpu.py holds the models against each other and against lime_pair_overlap_trim without a GPU;
tests/test_overlap_edges_gpu.py holds the kernel against all three."""
import numpy as np

from tests.adapter_cases import COMP, TRUSEQ_R1, TRUSEQ_R2, fasta_of, fastq_of   # noqa: F401  (the same helpers)
from tests.trim_cases import bases, records                                       # noqa: F401

SEED = 20316
FUZZ_CASES = 400
WORD = 64                                       # candidates a wave handles per step, symbols per word
PAIRS_PER_TRIP = 2048 * 4                       # RD_BLOCKS workgroups of RD_WAVES pairs (lime_reads.h): the grid cap
KEPT = 512                                      # OV_CAP * 64: the symbols of a mate whose words stay in LDS; beyond, they are made again
LENGTHS = lambda O: sorted({0, 1, O - 1, O, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1000})      # noqa: E731
INFO_KEYS = ("n_pairs", "n_overlap", "n_cut", "symbols_in", "symbols_out")
RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
CLASS = np.full(256, 4, dtype=np.int8)          # A C G T are 0 1 2 3 after & 0xDF; everything else has no class (4)
for _k, _c in enumerate(b"ACGT"):
    CLASS[_c] = CLASS[_c | 0x20] = _k


def revcomp(s):
    return bytes(s).translate(RC)[::-1]


# ---- the rule, twice ----
def places(La, Lb, I):
    """-> (first place, one behind the last): the j in [max(0, I - Lb), min(La, I))"""
    return max(0, I - Lb), min(La, I)


def insert_loop(a, b, O, E):
    """the rule as written: the largest I in [O, La + Lb - O] with n(I) >= O and mis(I) <= (n(I) * E) // 100; place j agrees when a[j] has a
    class and it is the complement of b[I - 1 - j]'s.  0 without one"""
    ca, cb = CLASS[np.frombuffer(bytes(a), dtype=np.uint8)], CLASS[np.frombuffer(bytes(b), dtype=np.uint8)]
    La, Lb = len(ca), len(cb)
    for I in range(La + Lb - O, O - 1, -1):
        j0, j1 = places(La, Lb, I)
        n = j1 - j0
        if n < O:
            continue
        x = ca[j0:j1]
        y = cb[I - 1 - j1 + 1:I - 1 - j0 + 1][::-1]          # b[I - 1 - j] for j = j0 .. j1 - 1
        same = int(np.count_nonzero((x < 4) & (y == 3 - x)))
        if n - same <= (n * E) // 100:
            return I
    return 0


def _masks(s, comp=False):
    """one integer per class: bit i set where s[i] is of that class (comp: of the complement's class)"""
    c = CLASS[np.frombuffer(bytes(s), dtype=np.uint8)]
    out = []
    for k in range(4):
        bits = np.packbits(c == (3 - k if comp else k), bitorder="little").tobytes()
        out.append(int.from_bytes(bits, "little"))
    return out


def insert_masks(a, b, O, E):
    """the closed form: A_c = mate 1's places of class c as one long integer, B_c = those of mate 2's reverse complement.  Place j of candidate
    I lies opposite place j + d of the reverse complement, d = Lb - I; the agreeing places are the set bits of A_c & (B_c >> d) (of
    (A_c >> -d) & B_c for d < 0) summed over c, and n(I) is arithmetic"""
    La, Lb = len(a), len(b)
    A, B = _masks(a), _masks(bytes(b)[::-1], comp=True)
    for I in range(La + Lb - O, O - 1, -1):
        n = min(La, I) - max(0, I - Lb)
        d = Lb - I
        same = sum(bin(A[c] & (B[c] >> d) if d >= 0 else (A[c] >> -d) & B[c]).count("1") for c in range(4))
        if n >= O and n - same <= (n * E) // 100:
            return I
    return 0


def mis_at(a, b, I):
    """(n(I), mis(I)): the rule's clause for one I, written out once more, on bytes"""
    A, B = bytes(x & 0xDF for x in bytes(a)), bytes(x & 0xDF for x in bytes(b))
    j0, j1 = places(len(A), len(B), I)
    pair = {65: 84, 67: 71, 71: 67, 84: 65}
    return max(j1 - j0, 0), sum(1 for j in range(j0, j1) if pair.get(A[j]) != B[I - 1 - j])


def cut_model(r1, r2, O, E, insert=insert_loop):
    """two lists of bytes -> (cut mates 1, cut mates 2, inserts, info as lime_overlap_info_t counts it)"""
    ins = [insert(a, b, O, E) for a, b in zip(r1, r2)]
    o1 = [bytes(a[:min(len(a), I)]) if I else bytes(a) for a, I in zip(r1, ins)]
    o2 = [bytes(b[:min(len(b), I)]) if I else bytes(b) for b, I in zip(r2, ins)]
    info = {"n_pairs": len(r1), "n_overlap": sum(I != 0 for I in ins),
            "n_cut": sum(len(x) != len(a) or len(y) != len(b) for x, a, y, b in zip(o1, r1, o2, r2)),
            "symbols_in": sum(map(len, r1)) + sum(map(len, r2)), "symbols_out": sum(map(len, o1)) + sum(map(len, o2))}
    return o1, o2, ins, info


# ---- planting ----
def spoil(rng, s, n_err, lo=0, hi=None):
    """s with n_err of its symbols in [lo, hi) changed to another base, at seeded places"""
    s = bytearray(s)
    hi = len(s) if hi is None else hi
    n_err = min(n_err, max(hi - lo, 0))
    for j in (rng.choice(hi - lo, size=n_err, replace=False) + lo if n_err else []):
        s[j] = s[j:j + 1].upper().translate(COMP)[0]
    return bytes(s)


def plant(rng, read, I, adapter1=TRUSEQ_R1, adapter2=TRUSEQ_R2, n_err=0, La=None, Lb=None):
    """a pair sequenced from the fragment that is the first I symbols of `read` (random bases behind it where it is shorter): mate 1 reads the
    fragment, mate 2 its reverse complement, each runs into its adapter and then filler where the fragment ends inside it, and holds La (Lb)
    symbols, by default len(read).  n_err symbols of mate 1 inside the fragment are changed: n_err mismatches at insert I"""
    La = len(read) if La is None else La
    Lb = len(read) if Lb is None else Lb
    frag = (bytes(read) + bases(rng, max(I - len(read), 0)))[:I]
    a = (frag + adapter1 + bases(rng, La))[:La]
    b = (revcomp(frag) + adapter2 + bases(rng, Lb))[:Lb]
    j0, j1 = places(La, Lb, I)
    return spoil(rng, a, n_err, j0, max(j1, j0)), b


def unrelated(rng, La, Lb, O, E):
    """two random mates that the rule leaves alone (redrawn where a chance overlap shows)"""
    for _ in range(1000):
        a, b = bases(rng, La), bases(rng, Lb)
        if insert_masks(a, b, O, E) == 0:
            return a, b
    raise AssertionError("no pair without an overlap found")


def hand_cases():
    """-> {name: (mates 1, mates 2, O, E)}; what each expects is written out in tests/test_overlap_cases_cpu.py"""
    rng = np.random.default_rng([SEED, 1])
    c = {}
    body = bases(rng, 400)
    # every insert on a 130 / 100 pair, one below the lowest candidate to one above the highest
    pairs = [plant(rng, body, I, La=130, Lb=100) for I in range(29, 130 + 100 - 30 + 2)]
    c["every insert of 130 / 100"] = ([p[0] for p in pairs], [p[1] for p in pairs], 30, 0)
    # 100 / 100, O = 30: the candidates run from 170 down; a step holds 64 of them (170 .. 107, 106 .. 43, 42 .. 30), and the kernel's own steps,
    # cut at multiples of 64 of the shift Lb - I, hold 170 .. 165, 164 .. 101, 100 .. 37, 36 .. 30
    at = (170, 165, 164, 107, 106, 101, 100, 43, 42, 37, 36, 30)
    pairs = [plant(rng, body, I, La=100, Lb=100) for I in at]
    c["first, last and 64th candidate of the steps"] = ([p[0] for p in pairs], [p[1] for p in pairs], 30, 0)
    a, b = plant(rng, body, 80, La=100, Lb=100)
    an, bn = a[:40] + b"N" + a[41:], b[:39] + b"N" + b[40:]      # place 40 of mate 1 lies opposite b[80 - 1 - 40]
    c["N opposite N"] = ([an, a, b"N" * 100], [bn, b, b"N" * 100], 30, 0)
    c["lower case"] = ([a.lower(), a, a.lower()], [b, b.lower(), b.lower()], 30, 0)
    c["other bytes"] = ([a[:10] + bytes([0, 255, 0x41 | 0x80, ord("R"), ord("-")]) + a[15:]], [b], 30, 10)
    c["an empty mate"] = ([b"", a, b"", b"A"], [b, b"", b"", b"T"], 1, 0)
    c["every pair empty"] = ([b""] * 5, [b""] * 5, 30, 10)
    c["mates shorter than O"] = ([a[:29], a[:29], a[:30], a], [revcomp(a[:29]), b, revcomp(a[:30]), revcomp(a)[:29]], 30, 0)
    c["periodic reads"] = ([b"AC" * 50, b"A" * 100, b"AC" * 50, b"A" * 70], [b"GT" * 50, b"T" * 100, b"GT" * 40, b"T" * 100], 30, 10)
    pairs = [plant(rng, body, I, La=100, Lb=100) for I in (100, 101, 150, 170, 171)]
    c["an ordinary overlap cuts nothing"] = ([p[0] for p in pairs], [p[1] for p in pairs], 30, 0)
    c["O of 1"] = ([b"A", b"A", b"ACG"], [b"T", b"A", b"N"], 1, 0)
    return c


THRESHOLD_N = (30, 64, 65, 130)


def threshold_cases():
    """mismatch counts of exactly (n * E) // 100 and one more at n = 30, 64, 65 and 130 places: a read-through pair with insert n in mates
    of n + 25 symbols -> {name: (a, b, O, E, n, n_err)}; I = n is admissible exactly when n_err <= (n * E) // 100"""
    rng = np.random.default_rng([SEED, 2])
    c = {}
    for E in (0, 10, 50):
        for n in THRESHOLD_N:
            allow = (n * E) // 100
            for n_err in (allow, allow + 1):
                a, b = plant(rng, bases(rng, n + 25), n, n_err=n_err)
                c[f"E {E} n {n} errors {n_err}"] = (a, b, 30, E, n, n_err)
    return c


def trap(n_err):
    """-> (a, b, O, E, smaller, larger): mates of 100 symbols at which the smaller insert 60 has no mismatch and the larger insert 150 (50
    places, 5 allowed at 10 percent) has n_err of them, all at places that the smaller insert does not hold"""
    rng = np.random.default_rng([SEED, 3])
    frag = bases(rng, 60)
    a, b = bytearray(frag + bases(rng, 40)), bytearray(revcomp(frag) + bases(rng, 40))
    for j in range(90, 100):                     # opposite b[59 .. 50], which the fragment fixes
        a[j] = bytes(b[149 - j:150 - j]).translate(RC)[0]
    for j in range(50, 90):                      # opposite b[99 .. 60], which is free
        b[149 - j] = bytes(a[j:j + 1]).translate(RC)[0]
    a = spoil(rng, bytes(a), n_err, 60, 90)
    return a, bytes(b), 30, 10, 60, 150


# ---- seeded collections ----
def fuzz_collection(seed, case):
    """-> (mates 1, mates 2, O, E): 0 .. 12 pairs of mates of 0 .. 300 symbols, equal or unequal; inserts from below O to above La + Lb, 0 .. 12 %
    of the places wrong, some N's, some lower case, empty mates, the periodic reads (AC)* and A*; every 50th case a pair of some thousands"""
    rng = np.random.default_rng([seed, 4, case])
    O = int(rng.choice([1, 8, 20, 30, 31])) if case % 3 else 30
    E = int(rng.choice([0, 5, 10, 12, 20, 50])) if case % 5 else int(rng.integers(0, 51))
    r1, r2 = [], []
    for _ in range(int(rng.integers(0, 13))):
        La = int(rng.integers(40, 161)) if rng.random() < 0.8 else int(rng.integers(0, 301))
        Lb = La if rng.random() < 0.5 else (int(rng.integers(40, 161)) if rng.random() < 0.8 else int(rng.integers(0, 301)))
        u = rng.random()
        if u < 0.52:                             # read-through: a cut where the insert is a candidate
            I = int(rng.integers(max(O - 5, 0), max(min(La, Lb), O) + 1))
        elif u < 0.72:                           # a long fragment: an overlap without a cut, up to above La + Lb (no overlap)
            I = int(rng.integers(max(La, Lb), La + Lb + 10))
        else:
            I = None
        if I is None:
            a, b = bases(rng, La), bases(rng, Lb)
        else:
            n = max(places(La, Lb, I)[1] - places(La, Lb, I)[0], 0)
            a, b = plant(rng, bases(rng, I), I, n_err=int(rng.binomial(n, rng.choice([0.0, 0.02, 0.06, 0.12]))), La=La, Lb=Lb)
        v = rng.random()
        if v < 0.06:
            a, b = (b"AC" * 150)[:La], (b"GT" * 150)[:Lb]
        elif v < 0.10:
            a, b = b"A" * La, b"T" * Lb
        elif v < 0.18:
            a = a.lower()
        elif v < 0.30 and La:
            x = bytearray(a)
            for j in rng.choice(La, size=min(La, 3), replace=False):
                x[j] = ord("N")
            a = bytes(x)
        r1.append(a); r2.append(b)
    if case % 50 == 49:
        I = int(rng.integers(600, 1500))
        a, b = plant(rng, bases(rng, I), I, n_err=int(rng.integers(0, 20)), La=int(rng.integers(1500, 3000)), Lb=int(rng.integers(1500, 3000)))
        r1.append(a); r2.append(b)
    return r1, r2, O, E


def fuzz_yield(seed=SEED, cases=FUZZ_CASES, insert=insert_masks):
    """the generator's yield over its cases, asserted so that no test on it is vacuous: at least a quarter of the pairs are cut, at least a
    tenth have an overlap without a cut, at least a tenth have none -> (pairs, cut, overlap without a cut, none)"""
    pairs = cut = whole = none = 0
    for case in range(cases):
        r1, r2, O, E = fuzz_collection(seed, case)
        for a, b in zip(r1, r2):
            I = insert(a, b, O, E)
            pairs += 1
            cut += bool(I) and I < max(len(a), len(b))
            whole += bool(I) and I >= max(len(a), len(b))
            none += not I
    assert 4 * cut >= pairs and 10 * whole >= pairs and 10 * none >= pairs, (pairs, cut, whole, none)
    return pairs, cut, whole, none
