"""Collections for the read-assignment step at the widths and edges of k_classify (lime_classify_kernel.hip), and a model of the decision
that is independent of decide() (lime_classify.cpp) and of the kernel.  No GPU; tests/test_classify_cases_cpu.py checks the model against
the reference's bytes and lime_classify_mem, tests/test_classify_edges_gpu.py runs the same collections through lime_classify_lists_dev,
tests/golden/make_golden_classify.py makes the wide goldens from near_tie_tables / tolerance_tables / beta0_tables.

The model is written from DESIGN.md section 9 f5 and the header of lime_classify.cpp: sets and dicts, every value an np.float32 looked up
in the writer's table (count / norm; its "%.5f" rounding for the text build), every sum and difference an np.float32 operation.

A collection is a dict: sims (list of 2 or 4 uint8 tables, reads x genomes), norm, beta, n_targ, tax (the lineage file's bytes), name."""
import numpy as np

TOL32 = np.float32(0.02)
N_HIGHER = 6
HEADER = "Accession_number;Species_TaxID;Genus_TaxID;Family_TaxID;Order_TaxID;Class_TaxID;Phylum_TaxID"


# ---- lists -------------------------------------------------------------------------------------------------------------------------
def lists_of(sim, norm, beta):
    """clusterChoose of one table: row maxima, row offsets of the passing rows' non-zero cells, (idRef, count) pairs"""
    sim = np.asarray(sim, dtype=np.uint8)
    mx = sim.max(axis=1) if sim.shape[1] else np.zeros(sim.shape[0], np.uint8)
    passing = mx.astype(np.float32) / np.float32(norm) > np.float32(beta)
    nz = (sim > 0) & passing[:, None]
    off = np.zeros(sim.shape[0] + 1, dtype=np.uint64)
    off[1:] = np.cumsum(nz.sum(axis=1))
    r, g = np.nonzero(nz)
    return mx, off, np.stack([g.astype(np.uint32), sim[r, g].astype(np.uint32)], axis=1)


def collection_lists(col):
    return [lists_of(s, col["norm"], col["beta"]) for s in col["sims"]]


# ---- the model ---------------------------------------------------------------------------------------------------------------------
class Tax:
    """a lineage file at one rank: taxon of every genome at the rank (rank 0: the genome itself), and with `higher` the genome's taxon at
    every rank from the chosen one up (0: the field is empty)"""

    def __init__(self, tax_bytes, rank, higher, n_targ):
        rows = [l.split(";") for l in tax_bytes.decode().split("\n")[1:-1]]       # header off; a last line without newline is not taken
        self.rank, self.higher = int(rank), bool(higher)
        self.at_rank = list(range(len(rows))) if rank == 0 else [int(f[rank]) for f in rows if f[rank] != ""]
        assert len(self.at_rank) == n_targ, "one taxon per genome at the chosen rank"
        self.up = {q: [int(f[q + 1]) if f[q + 1] != "" else 0 for f in rows[:n_targ]] for q in range(N_HIGHER)} if higher else {}


def value_tables(norm, beta, binary):
    """(value of a cell, value of a record's top) by count: the writers' count / norm in float32, seen through "%.5f" by the text build;
    a row whose maximum does not pass beta has no record (top 0)"""
    vals, tops = [], []
    for k in range(256):
        v = np.float32(k) / np.float32(norm)
        seen = v if binary else np.float32(float("%.5f" % float(v)))
        vals.append(seen)
        tops.append(seen if v > np.float32(beta) else np.float32(0))
    return vals, tops


class Report(dict):
    __getattr__ = dict.__getitem__


def _decide(rows, tops, n_targ, tax, F, tol):
    """one read.  rows: per list {genome: value}; tops: per list the record's top (0: none); F: the float type of every operation"""
    n = len(rows)
    zero = F(0)
    rep = Report(type="U", taxon=0, sim=np.float32(0), rule=0, T=sum(len(r) for r in rows), longest_row=0, every_genome=False, h_rank=None)
    held = [i for i in range(n) if tops[i] != 0]
    if not held:
        return rep
    best = max(F(tops[i]) for i in held)
    near = [i for i in held if F(best - F(tops[i])) < tol]
    cand = sorted({g for i in near for g, v in rows[i].items() if F(F(tops[i]) - F(v)) < tol})
    if len({tax.at_rank[g] for g in cand}) == 1:
        rep.update(type="C", taxon=tax.at_rank[cand[0]], sim=np.float32(best), rule=1)
        return rep
    # from here on the other lists' rows are looked into
    lens = [len(r) for r in rows]
    rep["longest_row"] = max([lens[j] for j in range(n) if any(lens[i] for i in range(n) if i != j)], default=0)
    strands = ((0, 3), (1, 2)) if n == 4 else ((0,), (1,))

    def strand_sum(g, k):
        s = zero
        for i in strands[k]:
            s = F(s + F(rows[i].get(g, zero)))
        return s

    top2 = [max([strand_sum(g, k) for g in cand], default=zero) for k in (0, 1)]
    win = 0 if top2[0] > F(top2[1] + tol) else 1 if top2[1] > F(top2[0] + tol) else None
    if win is not None:
        taxa = {tax.at_rank[g] for g in cand if strand_sum(g, win) == top2[win]}
        if len(taxa) == 1:
            rep.update(type="C", taxon=taxa.pop(), sim=np.float32(top2[win]), rule=2)
            return rep
    rep["rule"] = 3
    union = set().union(*[set(r) for r in rows])
    sums = {g: (strand_sum(g, 0), strand_sum(g, 1)) for g in union}
    hi = [max([s[k] for s in sums.values()], default=zero) for k in (0, 1)]
    which = (0,) if hi[0] > hi[1] else (1,) if hi[0] < hi[1] else (0, 1)
    h = hi[which[0]]
    chosen = {g for g, s in sums.items() if any(F(h - s[k]) < tol for k in which)}
    if F(h - zero) < tol:                                   # a genome in no list has sums 0: within tol of h as well
        rep["every_genome"] = True
        rep["longest_row"] = max(lens)
        chosen |= set(range(n_targ)) - union
    taxa = {tax.at_rank[g] for g in chosen}
    if len(taxa) == 1:
        rep.update(type="C", taxon=taxa.pop(), sim=np.float32(h))
        return rep
    if chosen and tax.higher and tax.rank >= 1:
        for q in range(tax.rank - 1, N_HIGHER):
            ups = {tax.up[q][g] for g in chosen}
            if len(ups) == 1 and 0 not in ups:
                rep.update(type="H", taxon=ups.pop(), sim=np.float32(h), h_rank=q)
                return rep
    rep["type"] = "A"
    return rep


def model_decide(lists, norms, betas, n_targ, taxonomy, binary, *, wide=False):
    """The decision of every read, from the lists (row_max, row_off, pairs) of the 2 or 4 inputs.  taxonomy: a Tax.  Returns one Report per
    read: type, taxon, sim, rule, T (elements in all rows), longest_row (the longest row another list's element is looked up in),
    every_genome (rule 3 selected the genomes in no list too), h_rank (the higher rank, 0 = species .. 5 = phylum, that gave an H).
    wide=True does every add and compare in float64 on the same table values: only to count the reads that depend on float32."""
    F = np.float64 if wide else np.float32
    tol = F(0.02)
    tabs = [value_tables(nm, bt, binary) for nm, bt in zip(norms, betas)]
    n_reads = len(lists[0][0])
    out, memo = [], {}
    offs = [np.asarray(l[1]).astype(np.int64) for l in lists]
    for r in range(n_reads):
        key, rows, tops = [], [], []
        for i, (mx, _, pairs) in enumerate(lists):
            p = np.asarray(pairs[offs[i][r]:offs[i][r + 1]]).reshape(-1, 2)
            key.append((int(mx[r]), p.tobytes()))
            tops.append(tabs[i][1][int(mx[r])])
            row = {}
            for g, k in p:
                row.setdefault(int(g), tabs[i][0][int(k) & 0xFF])
            rows.append(row)
        key = tuple(key)
        if key not in memo:
            memo[key] = _decide(rows, tops, n_targ, taxonomy, F, tol)
        out.append(memo[key])
    return out


def classification_bytes(reports):
    """the classification file of a list of Reports (maxSim as an ostream prints a float: %g)"""
    lines = ["C/U/A/H,IdSeqRead,TaxID,maxSim"]
    for r, v in enumerate(reports):
        lines.append(f"{v.type},{r},NA,0" if v.type in "UA" else f"{v.type},{r},{v.taxon},{'%g' % float(v.sim)}")
    return ("\n".join(lines) + "\n").encode()


def verdict_fields(reports):
    """(type, taxon, sim, rule) arrays as lime_verdict_t holds them"""
    return (np.array([ord(v.type) for v in reports], np.uint8), np.array([v.taxon for v in reports], np.uint32),
            np.array([v.sim for v in reports], np.float32), np.array([v.rule for v in reports], np.uint8))


# ---- taxonomies --------------------------------------------------------------------------------------------------------------------
def tree_taxonomy(n_targ, rng=None, holes=0.0, widths=(2, 4, 8, 16, 32, 64)):
    """genomes in a tree: `widths` consecutive genomes share species, genus, family, order, class, phylum.  holes: share of empty fields at
    family, class and phylum (never at species, genus or order: the ranks the goldens are made at keep one taxon per genome)"""
    lines = [HEADER]
    for g in range(n_targ):
        f = [f"ACC_{g:04d}.1"] + [str(1000 * (q + 1) + g // w) for q, w in enumerate(widths)]
        for q in (3, 5, 6):
            if rng is not None and rng.random() < holes:
                f[q] = ""
        lines.append(";".join(f))
    return ("\n".join(lines) + "\n").encode()


def taxonomy_of(fields):
    """lineage file from per-genome 6-tuples of taxa ('' for a hole)"""
    return ("\n".join([HEADER] + [";".join([f"ACC_{g:04d}.1"] + [str(x) for x in f]) for g, f in enumerate(fields)]) + "\n").encode()


# ---- generators --------------------------------------------------------------------------------------------------------------------
def _strand(i, n_files):
    return (0 if i in (0, 3) else 1) if n_files == 4 else i


# distance from the read's genome to a relative -> the lowest rank of tree_taxonomy the two share
_DIST = (1, 2, 3, 5, 6, 9, 12, 17, 24, 33, 48, 65, 90)
T_TARGETS = (63, 64, 65, 127, 128, 129, 257, 300)


def _unit_tables(n_files, n_reads, n_targ, rng, norm, unit, t_targets=T_TARGETS, p_none=0.06, lo_frac=0.3):
    """Reads with many near-ties.  A read has a genome with count `top` on strand 0, a few relatives (at tree distances that share only
    the species, the genus, ... or nothing) within 0, 1 or 2 * unit of it, a dense background of low counts, and a strand 1 that is weaker,
    equal, or `unit`s apart around the tolerance.  The first len(t_targets) reads get exactly that many elements over their lists."""
    sims = [np.zeros((n_reads, n_targ), np.uint8) for _ in range(n_files)]
    hi = min(norm, 250)
    for r in range(n_reads):
        fixed = r < len(t_targets)
        if not fixed and rng.random() < p_none:
            continue
        g = int(rng.integers(0, n_targ))
        top = int(rng.integers(max(int(lo_frac * norm), 8 * unit + 2), hi - 4 * unit))
        row = {g: top}
        spread = int(rng.integers(0, len(_DIST) + 1))
        for _ in range(int(rng.integers(0 if not fixed else 1, 5))):
            d = int(_DIST[int(rng.integers(0, max(1, spread)))]) * (1 if rng.random() < 0.5 else -1)
            row[(g + d) % n_targ] = top - unit * int(rng.integers(0, 3))
        row[g] = top
        want = t_targets[r] // n_files if fixed else int(rng.choice((0, 3, 10, 40, 70, n_targ - 8), p=(0.1, 0.1, 0.1, 0.25, 0.3, 0.15)))
        want = min(want, n_targ)
        free = [x for x in rng.permutation(n_targ) if int(x) not in row]
        for x in free[:max(0, want - len(row))]:
            row[int(x)] = int(rng.integers(1, max(2, top - 6 * unit)))
        mode = rng.choice(("weak", "equal", "near", "mixed"), p=(0.3, 0.2, 0.3, 0.2))
        shift = {"weak": None, "equal": 0, "near": unit * int(rng.integers(-2, 3)), "mixed": None}[mode]
        gone = int(rng.integers(0, n_files)) if (not fixed and rng.random() < 0.15) else -1
        for i in range(n_files):
            if i == gone:
                continue
            for x, c in row.items():
                c2 = c
                if _strand(i, n_files) == 1:
                    if mode == "weak":
                        c2 = c // 3
                    elif mode == "mixed":
                        c2 = c + unit * int(rng.integers(-1, 2)) if rng.random() < 0.6 else c // 3
                    else:
                        c2 = c + shift
                if rng.random() < 0.35:
                    c2 += unit * int(rng.integers(-1, 2))
                sims[i][r, x] = min(max(c2, 1), 255)
        if fixed:                                            # exactly t_targets[r] elements: low cells added to / taken from the last list
            last = sims[-1][r]
            have = sum(int((s[r] > 0).sum()) for s in sims)
            zeros = [x for x in np.nonzero(last == 0)[0]]
            lows = [x for x in np.nonzero(last > 0)[0] if int(x) not in (g,)]
            while have < t_targets[r] and zeros:
                last[zeros.pop()] = 1
                have += 1
            while have > t_targets[r] and lows:
                last[lows.pop()] = 0
                have -= 1
    return sims


def near_tie_tables(n_files, n_reads, n_targ, seed, norm=85, beta=0.05, holes=0.08):
    rng = np.random.default_rng(seed)
    tax = tree_taxonomy(n_targ, rng, holes)
    sims = _unit_tables(n_files, n_reads, n_targ, rng, norm, 1)
    return dict(sims=sims, norm=norm, beta=beta, n_targ=n_targ, tax=tax, name=f"near_tie{n_files}x{n_targ}")


def tolerance_tables(n_files, n_reads, n_targ, seed, norm):
    """norm 50: counts one unit apart, norm 100: two units apart; float32(k / norm) - float32((k - unit) / norm) is below float32(0.02) for
    about half of the k and not below it for the rest, so best - top, top - v, t0 > t1 + TOL, h - s all sit on the tolerance; reads of a
    single count `unit` have h == float32(0.02) itself (h < TOL is false in float32, true in double)"""
    assert norm in (50, 100)
    unit = norm // 50
    rng = np.random.default_rng(seed)
    tax = tree_taxonomy(n_targ, rng, 0.05)
    sims = _unit_tables(n_files, n_reads, n_targ, rng, norm, unit, t_targets=(63, 64, 65, 129), lo_frac=0.1)
    n_h, n_two = n_reads // 5, n_reads // 3
    for r in range(n_reads - n_h, n_reads):                 # h on the tolerance: a few cells of `unit` (and one below it for norm 100)
        for i, s in enumerate(sims):
            s[r] = 0
            if rng.random() < 0.8:
                for x in rng.integers(0, n_targ, size=int(rng.integers(1, 4))):
                    s[r, int(x)] = unit if rng.random() < 0.7 else max(1, unit - 1)
    for r in range(n_reads - n_h - n_two, n_reads - n_h):   # two genomes of different taxa `unit` apart at every count, strands 0 or `unit` apart
        a = int(rng.integers(0, n_targ))
        b = (a + int(rng.choice((2, 4, 8, 33)))) % n_targ
        k = int(rng.integers(2 * unit, norm // 2 + 1))
        for i, s in enumerate(sims):
            s[r] = 0
            d = unit * int(rng.integers(0, 2)) if _strand(i, n_files) == 1 else 0
            s[r, a] = k - d
            s[r, b] = max(k - d - unit * int(rng.integers(0, 2)), 1)
    return dict(sims=sims, norm=norm, beta=0.0, n_targ=n_targ, tax=tax, name=f"tol{norm}_{n_files}")


def beta0_tables(n_files, n_reads, n_targ, seed, norm=85):
    """beta 0: every non-empty row has a record.  A third of the reads hold only counts of 1 (h = 1 / norm < TOL: rule 3 selects every genome)"""
    rng = np.random.default_rng(seed)
    tax = tree_taxonomy(n_targ, rng, 0.05, widths=(2, 4, 8, 16, 64, 256))
    sims = _unit_tables(n_files, n_reads, n_targ, rng, norm, 1, t_targets=(65, 129))
    for r in range(2, n_reads, 3):
        for s in sims:
            s[r] = 0
            if rng.random() < 0.85:
                xs = rng.integers(0, n_targ, size=int(rng.choice((1, 2, 5, 70))))
                s[r, xs] = 1
    return dict(sims=sims, norm=norm, beta=0.0, n_targ=n_targ, tax=tax, name=f"beta0_{n_files}x{n_targ}")


# placement_cases: what must be present, by label
FIND_ROWS = (1, 2, 3, 63, 64, 65, 200)
FIND_POSITIONS = ("first", "last", "absent_below", "absent_above", "absent_between")
LAST_ELEMENT_T = (64, 65, 128, 129)                          # the deciding element is element 63, 64, 127, 128
PLACEMENTS = ([f"last_element_rule{k}_T{t}" for k in (1, 3) for t in LAST_ELEMENT_T]
              + [f"find_row{L}_{p}" for L in FIND_ROWS for p in FIND_POSITIONS if not (L == 1 and p == "absent_between")]
              + [f"only_list{i}_of{n}" for n in (2, 4) for i in range(n)]
              + [f"lists{i}{j}_of{n}" for n in (2, 4) for i in range(n) for j in range(i + 1, n)]
              + [f"later_only_of{n}" for n in (2, 4)] + [f"earlier_too_of{n}" for n in (2, 4)] + [f"shared_hole_of{n}" for n in (2, 4)])
HOLE_PAIR = (100, 105)                                       # placement_cases: no family for either; species and genus differ, the order is shared


def placement_cases(n_files):
    """Hand-built reads (norm 85, beta 0, a tree taxonomy over 420 genomes); labels[r] names what read r places.  The find_row* and
    last_element_rule3 reads need the strand sums of a paired-end read and come with n_files == 4 only; PLACEMENTS is the union."""
    n_targ, norm = 420, 85
    reads, labels = [], []

    def add(label, *rows):
        rows = list(rows) + [{}] * (n_files - len(rows))
        reads.append(rows[:n_files])
        labels.append(label)

    last = n_files - 1
    for t in LAST_ELEMENT_T:
        # rule 1: the only candidate is the last element of the last list (the best top; everything else is far below it)
        n0 = t // 2
        low0 = {2 * x: 1 + x % 5 for x in range(n0)}
        low1 = {2 * x + 1: 1 + x % 7 for x in range(t - n0 - 1)}
        low1[n_targ - 1] = 60
        add(f"last_element_rule1_T{t}", *([low0] + [{}] * (last - 1) + [low1]))
        if n_files == 4:
            # rule 3: lists 1 and 2 hold a (60) and b (60) of different phyla, b the read's last element; strand 1 wins rule 2 with a tie,
            # rule 3 selects a and b: A.  Without b: C.
            fill = {2 * x: 1 + x % 5 for x in range(t - 2)}
            row = dict(fill)
            row[301] = 60
            row[n_targ - 1] = 60
            add(f"last_element_rule3_T{t}", {}, {}, row, {})
    if n_files == 4:
        # find_in: q (60 in list 0, next to q2 = 60 of another taxon) is looked up in list 3's row of L low counts.  Found (3): strand 0's
        # sums are 60 + 3 against 60, rule 2 gives q's taxon; absent: a tie, rule 3, A.
        for L in FIND_ROWS:
            ids = [10 + 2 * x for x in range(L)]
            for pos in FIND_POSITIONS:
                if L == 1 and pos == "absent_between":
                    continue
                q = {"first": ids[0], "last": ids[-1], "absent_below": ids[0] - 3, "absent_above": ids[-1] + 3,
                     "absent_between": ids[L // 2 - 1] + 1 if L > 1 else 0}[pos]
                row3 = {x: 1 + (x // 2) % 4 for x in ids}
                if pos in ("first", "last"):
                    row3[q] = 3
                add(f"find_row{L}_{pos}", {q: 60, n_targ - 1: 60}, {}, {}, row3)
    # reads in one list only and in every pair of lists; near-ties so that the list an element belongs to matters (strand, top, own value)
    rng = np.random.default_rng(77 + n_files)
    for subset in [(i,) for i in range(n_files)] + [(i, j) for i in range(n_files) for j in range(i + 1, n_files)]:
        label = (f"only_list{subset[0]}_of{n_files}" if len(subset) == 1 else f"lists{subset[0]}{subset[1]}_of{n_files}")
        for _ in range(6):
            a = int(rng.integers(0, n_targ - 40))
            rows = [{} for _ in range(n_files)]
            for i in subset:
                for d in (0, 1, 2, 5, 17, 33):
                    if rng.random() < 0.7:
                        rows[i][a + d] = int(40 + rng.integers(0, 4))
                rows[i][a] = int(40 + rng.integers(0, 4))
            add(label, *rows)
    # a genome in a later list only / in an earlier list too, on rule 3's path (two genomes of different taxa tie on both strands)
    a, b = 100, 200
    add(f"later_only_of{n_files}", {a: 50}, {a: 50, b: 50})
    add(f"earlier_too_of{n_files}", {a: 50, b: 50}, {a: 50, b: 50})
    # two genomes that tie, both without a family (taxon 0 at that rank is no agreement): H at the order
    add(f"shared_hole_of{n_files}", {g: 50 for g in HOLE_PAIR}, {g: 50 for g in HOLE_PAIR})
    sims = [np.zeros((len(reads), n_targ), np.uint8) for _ in range(n_files)]
    for r, rows in enumerate(reads):
        for i, row in enumerate(rows):
            for g, c in row.items():
                sims[i][r, g] = c
    lines = tree_taxonomy(n_targ).decode().split("\n")
    for g in HOLE_PAIR:
        f = lines[1 + g].split(";")
        f[3] = ""
        lines[1 + g] = ";".join(f)
    return dict(sims=sims, norm=norm, beta=0.0, n_targ=n_targ, tax="\n".join(lines).encode(), name=f"placement{n_files}", labels=labels)


EVERY_GENOME_N = (1, 63, 64, 65, 129, 1000)
EVERY_GENOME_TAX = ("one", "two", "higher", "last")


def every_genome_cases(n_targ, kind, n_files=2, norm=64):
    """beta 0 and 1 / norm < TOL: a read that holds only counts of 1, two of them of different taxa, fails rules 1 and 2 and makes rule 3
    select every genome.  kind: "one" all genomes of one taxon (rule 1 decides: rule 3 cannot end in C here, its selection holds rule 1's
    candidates); "two" even and odd genomes differ at every rank (A); "higher" they differ in the species only (H at the genus);
    "last" as "higher", but the last genome differs from all others at every rank (A; H for a walk that stops before it)"""
    assert norm >= 64
    fields = []
    for g in range(n_targ):
        odd = g % 2
        f = {"one": (11, 21, 31, 41, 51, 61), "two": tuple(10 * q + 11 + odd for q in range(6))}.get(kind, (11 + odd, 21, 31, 41, 51, 61))
        if kind == "last" and g == n_targ - 1 and g > 0:
            f = (13, 23, 33, 43, 53, 63)
        fields.append(f)
    tax = taxonomy_of(fields)
    rng = np.random.default_rng(1000 * n_targ + len(kind))
    n_reads = 10
    sims = [np.zeros((n_reads, n_targ), np.uint8) for _ in range(n_files)]
    for r in range(n_reads):
        for i, s in enumerate(sims):
            if r == 0 and i > 0:
                continue                                     # read 0: one cell in list 0, nothing else
            xs = rng.integers(0, n_targ, size=int(rng.integers(1, 4)))
            s[r, xs] = 1 if r < 7 else rng.integers(1, 4, size=len(xs))      # reads 7..9: counts up to 3 (h may reach TOL)
        if 1 <= r < 7 and n_targ > 1:                        # an even and an odd genome in list 0; never the last genome
            a = int(rng.integers(0, max(1, (n_targ - 1) // 2)))
            sims[0][r, n_targ - 1] = 0
            sims[0][r, 2 * a] = 1
            sims[0][r, min(2 * a + 1, max(n_targ - 2, 1))] = 1
    return dict(sims=sims, norm=norm, beta=0.0, n_targ=n_targ, tax=tax, name=f"every_genome{n_targ}_{kind}")


def shifted_lineage_case(n_files=2):
    """A lineage file with one line more than genomes and an empty species on line 2: at the species rank the empty field is skipped, so
    at_rank is the species of lines 0, 1, 3, 4, 5, 6 while the higher ranks stay by line.  Genomes 3 and 4 then differ at the rank and
    share the species of their own lines: the only way the chosen rank itself (index rank - 1 of the higher ranks) decides an H.
    Not a golden: the reference's HIGHER build writes past its table for a line beyond numGenomes."""
    sp = (11, 12, "", 14, 14, 15, 16)
    tax = taxonomy_of([(x, 21 + k, 31, 41, 51, 61) for k, x in enumerate(sp)])
    sims = [np.zeros((3, 6), np.uint8) for _ in range(n_files)]
    for s in sims:
        s[0, 3] = s[0, 4] = 50                               # H at the species of lines 3 and 4
        s[1, 0] = s[1, 1] = 50                               # A below the family, H there
        s[2, 4] = s[2, 5] = 50
    return dict(sims=sims, norm=85, beta=0.0, n_targ=6, tax=tax, name="shifted_lineage")


STRIDE_READS = 16384 + 5                                     # launch_classify: at most 4096 workgroups of 4 waves, the rest by grid stride


def stride_case(n_files=2):
    """3 genomes of three species, two genera; reads 0..4 and 16384..16388 have rows of their own, the rest repeat a pattern of 7"""
    n_targ, norm = 3, 85
    tax = taxonomy_of([(11, 21, 31, 41, 51, 61), (12, 21, 31, 41, 51, 61), (13, 22, 31, 41, 51, 61)])
    rng = np.random.default_rng(5)
    pattern = rng.integers(0, 60, size=(7, n_files, n_targ))
    sims = [np.ascontiguousarray(pattern[np.arange(STRIDE_READS) % 7, i, :]).astype(np.uint8) for i in range(n_files)]
    own = rng.integers(30, 36, size=(10, n_files, n_targ))  # near-ties: distinct, non-trivial
    own[:, :, 2] += np.arange(10)[:, None]
    for k, r in enumerate(list(range(5)) + list(range(16384, 16389))):
        for i in range(n_files):
            sims[i][r] = own[k, i]
    return dict(sims=sims, norm=norm, beta=0.1, n_targ=n_targ, tax=tax, name="stride")


def fuzz_collection(seed):
    """-> (collection, rank, higher, binary): at most 64 reads and 300 genomes, 2 or 4 lists, drawn from the generators above"""
    rng = np.random.default_rng(100003 * seed + 17)
    n_files = int(rng.choice((2, 4)))
    n_reads = int(rng.integers(1, 65))
    n_targ = int(rng.choice((1, 2, 7, 63, 64, 65, 130, 300)))
    kind = int(rng.integers(0, 4))
    if kind == 0 or n_targ < 40:
        norm = int(rng.choice((10, 50, 64, 85, 100)))
        beta = float(rng.choice((0.0, 0.1, 0.25)))
        sims = [np.where(rng.random((n_reads, n_targ)) < rng.choice((0.02, 0.3, 0.9)), rng.integers(0, min(norm, 255), (n_reads, n_targ)), 0).astype(np.uint8)
                for _ in range(n_files)]
        col = dict(sims=sims, norm=norm, beta=beta, n_targ=n_targ, tax=tree_taxonomy(n_targ, rng, 0.1), name=f"fuzz{seed}")
    elif kind == 1:
        col = near_tie_tables(n_files, n_reads, n_targ, seed, norm=int(rng.choice((60, 85))), beta=float(rng.choice((0.0, 0.05, 0.25))))
    elif kind == 2:
        col = tolerance_tables(n_files, max(n_reads, 16), n_targ, seed, int(rng.choice((50, 100))))
    else:
        col = beta0_tables(n_files, n_reads, n_targ, seed, norm=int(rng.choice((64, 85))))
    higher = int(rng.integers(0, 2))
    rows = [l.split(";") for l in col["tax"].decode().split("\n")[1:-1]]
    full = [q for q in range(1, 7) if all(f[q] != "" for f in rows)]         # a hole at the chosen rank would leave fewer taxa than genomes
    rank = int(rng.choice(full if higher else [0] + full))
    col["name"] = f"fuzz{seed}:{col['name']}"
    return col, rank, higher, int(rng.integers(0, 2))


# ---- what the two test modules share -----------------------------------------------------------------------------------------------
COMBOS = tuple((b, h, r) for b in (1, 0) for h, r in ((0, 0), (0, 1), (1, 1), (1, 2), (1, 4)))       # (binary, higher, rank)
NEW_GOLDENS = ("wide_single", "wide_paired", "tol50", "tol100_single", "beta0_wide")


def same_verdicts(reports, v):
    """None, or what differs between the model's Reports and an array of lime_verdict_t (every field; pad zero)"""
    ty, tx, sm, ru = verdict_fields(reports)
    if len(v) != len(reports):
        return f"{len(v)} verdicts for {len(reports)} reads"
    for name, want in (("type", ty), ("taxon", tx), ("sim", sm), ("rule", ru)):
        bad = np.nonzero(v[name] != want)[0]
        if len(bad):
            r = int(bad[0])
            return f"{name} of read {r}: {v[name][r]!r}, model {want[r]!r} ({dict(reports[r])})"
    if v["pad"].any():
        return "pad bytes not zero"
    return None
