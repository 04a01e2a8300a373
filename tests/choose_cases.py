"""Chosen tables for clusterChoose on the device, along its two routes, and a numpy model of what it must return.

With the table: k_choose + k_gather_pairs (lime_kernels.hip) under lime_choose_dev / lime_choose_pairs_dev / lime_choose_lists_dev -- a case is a
sparse table plus the (norm, beta) to test it with.  Without the table: k_region_rows, k_bigrec_count / k_bigrec_scatter and k_apply_tiles<WIDE, 1>
then <WIDE, 2> (lime_apply.hip) under lime_fused_choose_dev -- a case is a sparse table, and arrays_of() makes the (lcp, da, ebwt) whose table is
exactly that one, so that every cell, its sum and where its updates come from (the scan or a long cluster) are chosen, not drawn.
tests/test_choose_cases_cpu.py shows without a GPU that the model is right, that the oracle's table of every hand-made collection is the chosen
one, and that every case holds the edge it is named for; tests/test_choose_edges_gpu.py runs them.  Everything is seeded, pure numpy.

A table is described sparsely -- Cells: (read, genome, sum[, long]) entries, several to one cell allowed; their sums count modulo 256 and a cell
whose sum is 0 modulo 256 is absent from the table."""
import numpy as np

# lime_amd/csrc/lime_apply.hip, lime_kernels.hip
REGION_SHIFT = 16
REGION = 1 << REGION_SHIFT            # k_apply_tiles builds 64 KB of the table per workgroup pass
FIN_SEGS = 258                        # row segments per region up to which MODE 1 looks at the region from LDS words per segment
QW = 768                              # first adds a wave can queue per region
NWV = 8                               # waves of a k_apply_tiles workgroup
SMALL_REFS = 16                       # below: a wave per segment whatever the segments' number
CHOOSE_SWEEP, GATHER_SWEEP = 1024, 256          # bytes of a row a wave covers per sweep: k_choose (64 x 16), k_gather_pairs (64 x 4)
CHOOSE_CAP, GATHER_CAP = 65536 * 4, 16384 * 4   # rows the largest grids of launch_choose / launch_gather_pairs take at once
MAX_K = 32                            # copies of a read in one short cluster of arrays_of()
MID_MAX = 64                          # clusters beyond this many symbols are k_score_big's: their updates arrive as 64-bit records
WIN, HALO = 1024, 16                  # lime_kernels.h: positions a wave of the scan owns per window, and its read-ahead behind them
ALPHA = 16
BASE = ord("C")


class Cells:
    """a sparse table: entry i adds v[i] to cell (r[i], g[i]); long[i]: through ONE cluster of more than MID_MAX symbols (v <= 255)"""

    def __init__(self, r=(), g=(), v=(), long=None):
        self.r = np.asarray(r, dtype=np.int64).reshape(-1)
        self.g = np.asarray(g, dtype=np.int64).reshape(-1)
        self.v = np.asarray(v, dtype=np.int64).reshape(-1)
        self.long = np.zeros(len(self.r), dtype=bool) if long is None else np.asarray(long, dtype=bool).reshape(-1)
        assert len(self.r) == len(self.g) == len(self.v) == len(self.long)
        assert len(self.v) == 0 or (self.v.min() >= 1 and (self.v[self.long] <= 255).all())

    @staticmethod
    def of(items):
        items = list(items)
        return Cells([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [len(i) > 3 and bool(i[3]) for i in items])

    @staticmethod
    def at(lin, v, n_refs, long=None):
        lin = np.asarray(lin, dtype=np.int64).reshape(-1)
        return Cells(lin // n_refs, lin % n_refs, np.broadcast_to(np.asarray(v, dtype=np.int64), lin.shape), long)

    def __add__(self, o):
        return Cells(np.concatenate([self.r, o.r]), np.concatenate([self.g, o.g]), np.concatenate([self.v, o.v]), np.concatenate([self.long, o.long]))

    def __len__(self):
        return len(self.r)

    def lin(self, n_refs):
        return self.r * n_refs + self.g


def _entries(x, n_refs):
    """any description of a table -> (cell as r * n_refs + g, value added), unsorted, unsummed"""
    if isinstance(x, Cells):
        return x.lin(n_refs), x.v
    if isinstance(x, dict):
        k = np.array(list(x.keys()), dtype=np.int64).reshape(-1, 2)
        return k[:, 0] * n_refs + k[:, 1], np.array(list(x.values()), dtype=np.int64)
    if isinstance(x, np.ndarray) and x.ndim == 2:
        lin = np.flatnonzero(x)
        return lin.astype(np.int64), x.reshape(-1)[lin].astype(np.int64)
    r, g, v = x
    return np.asarray(r, dtype=np.int64) * n_refs + np.asarray(g, dtype=np.int64), np.asarray(v, dtype=np.int64)


def table_of(x, n_reads, n_refs):
    """-> (cells ascending, their values 1 .. 255): the table's non-zero cells"""
    lin, v = _entries(x, n_refs)
    assert len(lin) == 0 or (lin.min() >= 0 and lin.max() < n_reads * n_refs)
    if not len(lin):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    u, inv = np.unique(lin, return_inverse=True)
    s = np.bincount(inv.reshape(-1), weights=v.astype(np.float64)).astype(np.int64) & 255            # (sums far below 2^53)
    return u[s != 0], s[s != 0]


def choose_model(x, n_reads, n_refs, norm, beta):
    """clusterChoose (ClusterBWT_DA.cpp:385-423) -> (row_max u8[n_reads], row_nnz u32[n_reads], row_off u64[n_reads + 1], pairs u32[n, 2]): the rows'
    maxima and non-zero counts, and for the rows with float(max) / norm > beta, in the reference's types (:404-406), their (idRef, sim) in ascending idRef"""
    lin, val = table_of(x, n_reads, n_refs)
    row = lin // n_refs
    mx = np.zeros(n_reads, dtype=np.uint8)
    np.maximum.at(mx, row, val.astype(np.uint8))
    nnz = np.bincount(row, minlength=n_reads).astype(np.uint32)
    ok = (mx.astype(np.float32) / np.float32(norm)) > np.float32(beta)
    off = np.zeros(n_reads + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.where(ok, nnz, 0).astype(np.uint64))
    keep = ok[row]
    pairs = np.stack([lin[keep] - row[keep] * n_refs, val[keep]], axis=1).astype(np.uint32)
    return mx, nnz, off, pairs


def choose_naive(dense, norm, beta):
    """the same, row by row over a dense table"""
    mx, nnz, off, pairs = [], [], [0], []
    for row in dense.tolist():
        m = max(row) if row else 0
        nz = [(j, x) for j, x in enumerate(row) if x]
        mx.append(m); nnz.append(len(nz))
        if np.float32(m) / np.float32(norm) > np.float32(beta):
            pairs += nz
        off.append(len(pairs))
    return (np.array(mx, np.uint8), np.array(nnz, np.uint32), np.array(off, np.uint64), np.array(pairs, np.uint32).reshape(-1, 2))


def dense_of(x, n_reads, n_refs):
    lin, val = table_of(x, n_reads, n_refs)
    t = np.zeros(n_reads * n_refs, dtype=np.uint8)
    t[lin] = val
    return t.reshape(n_reads, n_refs)


# ---- the collection whose table is the chosen one --------------------------------------------------------------------------------------
def clusters_of(cells):
    """-> (read, genome, copies of the read, copies of the genome) per cluster: an entry that is not long as clusters of k <= MAX_K + k, a
    long one as ONE cluster of v reads and enough genomes for more than MID_MAX symbols.  Each adds min(reads, genomes) to its cell."""
    sh = np.flatnonzero(~cells.long)
    v = cells.v[sh]
    ncl = (v + MAX_K - 1) // MAX_K
    idx = np.repeat(sh, ncl)
    j = np.arange(len(idx)) - np.repeat(np.cumsum(ncl) - ncl, ncl)
    k = np.minimum(MAX_K, np.repeat(v, ncl) - MAX_K * j)
    lo = np.flatnonzero(cells.long)
    vl = cells.v[lo]
    gl = np.where(vl % 2 == 0, np.maximum(vl, MID_MAX + 1 - vl), 2 * vl + MID_MAX + 1)     # 40 + 40; 101 + 267 (genome counts saturate at 255 >= v)
    return (np.concatenate([cells.r[idx], cells.r[lo]]), np.concatenate([cells.g[idx], cells.g[lo]]),
            np.concatenate([k, vl]), np.concatenate([k, gl]))


def crosses(start, size):
    """the scan takes the arrays in windows of WIN positions with a read-ahead of HALO: a cluster that begins in a window and does not close inside
    that window's read-ahead is scored like a long one, whatever its size -- its update arrives as a 64-bit record (k_resolve_open)"""
    return start + size >= (start // WIN + 1) * WIN + HALO


def _starts(size, fit):
    """where every cluster begins: one behind the other with one lone genome between them; fit: further lone genomes in front of a cluster that would
    not close inside its window's read-ahead, so that it begins with the next window"""
    L = size + 1
    start = 1 + np.cumsum(L) - L
    if not fit or not len(L):
        return start
    assert (size <= WIN).all()                                    # (from a window's first position every cluster closes in time)
    i0, shift, n = 0, 0, len(L)
    while i0 < n:                                                 # a step per window: the next WIN clusters reach beyond it
        j = min(n, i0 + WIN)
        start[i0:j] += shift
        hit = np.flatnonzero(crosses(start[i0:j], size[i0:j]))
        if not len(hit):
            i0 = j
            continue
        h = i0 + int(hit[0])
        start[h:j] -= shift                                       # (not placed yet)
        shift += int((start[h] + shift) // WIN + 1) * WIN - int(start[h] + shift)
        i0 = h
    return start


def arrays_of(cells, n_reads, n_refs, alpha=ALPHA, ebwt=None, seed=None, fit=True):
    """-> (lcp u32, da u32, ebwt u8 | None).  A cluster: its copies of the read, then its copies of genome n_reads + g; lcp 0 at its first position,
    alpha on the others; one lone genome with lcp 0 in front of everything and behind every cluster.  ebwt: None, or the byte every position holds
    (one repeated base: the pair score is min(reads, genomes) as without ebwt).  seed: the clusters in a seeded random order, so that a region's
    records spread over tiles and waves.  fit: no cluster lies across the end of a scan window's read-ahead (crosses()), so that only the long ones
    arrive as 64-bit records; without it about one cluster in WIN / its size does."""
    cr, cg, kr, kg = clusters_of(cells)
    assert len(cr) == 0 or (cr.min() >= 0 and cr.max() < n_reads and cg.min() >= 0 and cg.max() < n_refs)
    if seed is not None:
        o = np.random.default_rng(seed).permutation(len(cr))
        cr, cg, kr, kg = cr[o], cg[o], kr[o], kg[o]
    size = kr + kg
    start = _starts(size, fit)
    n = int(start[-1] + size[-1]) + 1 if len(size) else 1
    da = np.full(n, n_reads, dtype=np.int64)                      # lone genomes everywhere ...
    lcp = np.zeros(n, dtype=np.uint32)
    cl = np.repeat(np.arange(len(size)), size)                    # ... but in the clusters
    j = np.arange(len(cl)) - np.repeat(np.cumsum(size) - size, size)
    pos = start[cl] + j
    da[pos] = np.where(j < kr[cl], cr[cl], n_reads + cg[cl])
    lcp[pos] = np.where(j == 0, 0, alpha)
    if len(size):
        da[start + size] = n_reads + (cg + 1) % n_refs            # (the lone genome behind a cluster is another one than the cluster's)
    return lcp, da.astype(np.uint32), None if ebwt is None else np.full(n, ebwt, dtype=np.uint8)


def n_clusters_of(cells):
    return len(clusters_of(cells)[0])


def n_big_of(cells, seed=None, fit=True):
    """-> (clusters of arrays_of(cells, ..., seed=seed, fit=fit) whose updates arrive as 64-bit records -- lime_stats_t.n_big --, those of them that are
    not long: fit leaves none)"""
    _, _, kr, kg = clusters_of(cells)
    if seed is not None:
        o = np.random.default_rng(seed).permutation(len(kr))
        kr, kg = kr[o], kg[o]
    size = kr + kg
    cross = crosses(_starts(size, fit), size)
    return int((cross | (size > MID_MAX)).sum()), int((cross & (size <= MID_MAX)).sum())


# ---- k_region_rows and the looks of k_apply_tiles<., 1> --------------------------------------------------------------------------------
def sim_bytes(n_reads, n_refs):
    return (n_reads * n_refs + 15) & ~15


def region_rows(n_reads, n_refs):
    """k_region_rows in numpy -> (r0, o0, nseg, len) per 64 KB region: first row, offset of the region's first byte in it, row segments, bytes
    of the region inside the table"""
    tb = n_reads * n_refs
    rb = np.arange((sim_bytes(n_reads, n_refs) + REGION - 1) >> REGION_SHIFT, dtype=np.int64) << REGION_SHIFT
    ln = np.minimum(tb - rb, REGION)
    assert (ln > 0).all()
    r0, r1 = rb // n_refs, (rb + ln - 1) // n_refs
    return r0, rb - r0 * n_refs, r1 - r0 + 1, ln


def region_facts(cells, n_reads, n_refs):
    """per region, from the cells alone: distinct cells the scan's records add to (each is queued once as a first add), whether one of their sums
    passes 255 (the region is rebuilt with the exact adds), whether a long cluster's record falls into it, and whether a cell stands at exactly 255
    where an add of 0 could meet it (k_apply_tiles: a record slot outside the run adds 0 to the word its 16 bits name and raises the flag all the
    same; slots beyond a row's end name cell 0) -- only then is the look of a region without a wrap not decided by its own cells"""
    nreg = len(region_rows(n_reads, n_refs)[0])
    lin = cells.lin(n_refs)
    u, inv = np.unique(lin[~cells.long], return_inverse=True)
    s = np.bincount(inv.reshape(-1), weights=cells.v[~cells.long].astype(np.float64)).astype(np.int64) if len(u) else np.zeros(0, np.int64)
    reg = u >> REGION_SHIFT
    first = np.bincount(reg, minlength=nreg)
    wrap = np.bincount(reg[s >= 256], minlength=nreg) > 0
    big = np.bincount(lin[cells.long] >> REGION_SHIFT, minlength=nreg) > 0
    offs = np.bincount(u & (REGION - 1), minlength=REGION)
    at255 = u[s == 255]
    risky = np.bincount((at255 >> REGION_SHIFT)[((at255 & (REGION - 1)) == 0) | (offs[at255 & (REGION - 1)] > 1)], minlength=nreg) > 0
    return first, wrap, big, risky


def looks(cells, n_reads, n_refs):
    """which of MODE 1's three looks every region gets: "walk" (the waves' queues of first adds), "rows" (fin_region_rows, piece by piece), "segs"
    (fin_region<1>, a wave per segment); None where the cells do not decide it (769 .. 6144 cells: it depends on how they fall to the waves).
    For the arrays of arrays_of(..., fit=True) only: without fit, clusters of any size arrive as 64-bit records (crosses()), and a region that gets
    one is looked at piece by piece like one with a long cluster's cell."""
    _, _, nseg, _ = region_rows(n_reads, n_refs)
    first, wrap, big, risky = region_facts(cells, n_reads, n_refs)
    out = []
    for k in range(len(nseg)):
        if nseg[k] > FIN_SEGS or n_refs < SMALL_REFS:
            out.append("segs")
        elif wrap[k] or big[k] or first[k] > NWV * QW:
            out.append("rows")
        elif first[k] <= QW and not risky[k]:
            out.append("walk")
        else:
            out.append(None)
    return out


def seg_edges(n_reads, n_refs, region):
    """the table cells at the first and the last byte of every row segment of a region"""
    r0, o0, nseg, ln = (int(a[region]) for a in region_rows(n_reads, n_refs))
    j = np.arange(nseg, dtype=np.int64)
    s = np.maximum(j * n_refs - o0, 0)
    e = np.minimum((j + 1) * n_refs - o0, ln)
    return np.unique(np.concatenate([s, e - 1])) + (region << REGION_SHIFT)


def _vals(n, lo=1, span=200, step=7):
    return lo + (np.arange(n, dtype=np.int64) * step) % span


# ---- cases for the route with the table --------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _table(name, n_reads, n_refs, cells, tests, **facts):
    return Case(name=name, n_reads=n_reads, n_refs=n_refs, cells=cells, tests=list(tests), facts=facts)


SHARED_REFS = [1, 2, 3, 5, 15, 16, 17, 31, 33, 47]
# F: a row full of 255; a / z: the only cell, a 1, at the row's first / last byte; E: an empty row; R: a row of seeded values, zeros among them
SHARED_ROWS = "FaFzFEFEEFaazzFFRERaRzRFEaEzEF" + "RRRRRRRRRR"


def shared_group(n_refs):
    """rows shorter than, as long as and a little longer than a 16-byte group: the first and the last group of a row are the same one, or neighbours"""
    rng = np.random.default_rng(1000 + n_refs)
    t = np.zeros((len(SHARED_ROWS), n_refs), dtype=np.uint8)
    for r, k in enumerate(SHARED_ROWS):
        if k == "F":
            t[r] = 255
        elif k == "a":
            t[r, 0] = 1
        elif k == "z":
            t[r, -1] = 1
        elif k == "R":
            t[r] = rng.integers(0, 256, n_refs) * (rng.random(n_refs) < 0.5)
    return _table(f"shared_group_{n_refs}", len(SHARED_ROWS), n_refs, t, [(85, 0.0), (85, 0.02), (85, -1.0)], rows=SHARED_ROWS)


def one_bit():
    """rows whose only cell has ONE bit set, every bit at every byte position of a word: k_choose's fold of a byte's bits must see each"""
    n_refs = 12
    cells = Cells.of((4 * b + p, 4 + p, 1 << b) for b in range(8) for p in range(4))
    return _table("one_bit", 32, n_refs, cells, [(85, 0.0), (1, 100.0)])


SWEEP_REFS = list(range(253, 261)) + [511, 513, 1008, 1023, 1024, 1025, 1040, 2049]


def sweep_edges(n_refs):
    """rows of more than one sweep of a wave: the only cell of a row at the last byte of a sweep, then at the first byte of the next (the sweeps
    start at the row's first 16-byte group in k_choose and at its first word in k_gather_pairs), and rows with every cell set"""
    items, r, on = [], 1, {CHOOSE_SWEEP: 0, GATHER_SWEEP: 0}
    for sweep, unit in ((CHOOSE_SWEEP, 16), (GATHER_SWEEP, 4)):
        for s in range(1, n_refs // sweep + 2):
            for side in (-1, 0):
                b0 = r * n_refs
                col = b0 // unit * unit + sweep * s + side - b0
                if 0 <= col < n_refs:
                    items.append((r, col, 3 + (r % 250)))
                    on[sweep] += 1
                    r += 1
    n_reads = r + 2
    full = np.random.default_rng(n_refs).integers(1, 256, (2, n_refs))
    cells = Cells.of(items) + Cells(np.repeat([0, r], n_refs), np.tile(np.arange(n_refs), 2), full.reshape(-1))        # (row r + 1 is empty)
    return _table(f"sweep_edges_{n_refs}", n_reads, n_refs, cells, [(85, 0.0), (85, 0.5)], on_edge=on, full_rows=[0, r])


GRID_SHAPES = [(CHOOSE_CAP + 5, 3), (GATHER_CAP + 3, 5)]


def grid_stride(n_reads, n_refs):
    """more rows than the largest grid takes at once: marked rows (they pass) at 0, on both sides of either cap and last; rows that fail next to
    them and every 997th row"""
    marked = sorted({0, n_reads - 1} | {c + d for c in (CHOOSE_CAP, GATHER_CAP) for d in (-1, 0, 1) if c + d < n_reads})
    fail = sorted(({m + d for m in marked for d in (-2, 2)} | set(range(500, n_reads, 997))) - set(marked))
    fail = [f for f in fail if 0 <= f < n_reads]
    cells = Cells.of([(m, (i + k) % n_refs, 100 + 10 * i + k) for i, m in enumerate(marked) for k in range(1 + i % n_refs)] +
                     [(f, f % n_refs, 1) for f in fail])
    return _table(f"grid_stride_{n_reads}x{n_refs}", n_reads, n_refs, cells, [(85, 0.02)], marked=marked, failing=fail)


def padding(n_reads):
    """17-byte rows: the table ends at n_reads modulo 16 bytes behind a 16-byte border.  The bytes up to lime_sim_bytes() are filled with 0xFF
    by the test (include/lime_hip.h asks only that they exist)"""
    n_refs = 17
    cells = Cells.of([(n_reads - 1, n_refs - 1, 9), (n_reads - 1, 0, 200), (0, 0, 7), (n_reads // 2, 5, 1)])
    return _table(f"padding_{n_reads}", n_reads, n_refs, cells, [(85, 0.0)])


BIG_SHAPE = (70001, 65537)            # 4.59 GB; row 65535 starts at byte 2^32 - 1


def beyond_4g():
    """r * n_refs beyond 2^32: cells in the rows below, across and above byte 2^32, in the last row and the last cell.  Sparse model only."""
    n_reads, n_refs = BIG_SHAPE
    items = []
    for i, r in enumerate([0, 65533, 65535, 65534, 65536, 65537, 70000, 69999]):
        for k, g in enumerate([0, 1, 2, 4095, 32768, 65535, 65536][i % 2:]):
            items.append((r, g, 2 + (13 * i + 5 * k) % 250))
    items += [(65532, 7, 1), (65538, 65536, 1), (3, 3, 1)]                  # rows that fail
    return _table("beyond_4g", n_reads, n_refs, Cells.of(items), [(85, 0.02)])


BETA_TRIPLES = [(4, 0.25, 1), (100, 0.02, 2), (85, 0.2, 17)]


def beta_edges():
    """rows whose maximum is m - 1, m, m + 1 for every (norm, beta, m) with float(m) / norm == beta exactly: m fails, m + 1 passes; beta -1: every
    row passes and empty rows list nothing; beta 0: rows of maximum 0 fail; beta 3: no row passes"""
    rows = sorted({m + d for _, _, m in BETA_TRIPLES for d in (-1, 0, 1)} | {0, 255})
    cells = Cells.of([(i, (3 * i) % 7, m) for i, m in enumerate(rows) if m] + [(i, (3 * i + 2) % 7, 1) for i, m in enumerate(rows) if m > 1])
    return _table("beta_edges", len(rows), 7, cells, [(n, b) for n, b, _ in BETA_TRIPLES] + [(85, -1.0), (85, 0.0), (85, 3.0)], maxima=rows)


def no_reads():
    return _table("no_reads", 0, 5, Cells(), [(85, 0.0), (85, -1.0)])


def all_zero():
    return _table("all_zero", 37, 19, Cells(), [(85, -1.0), (85, 0.0)])


FUZZ_TABLES = 200


def fuzz_table(i):
    """a small seeded table whose shape is drawn from the sets above"""
    rng = np.random.default_rng(50_000 + i)
    n_refs = int(rng.choice(SHARED_REFS + SWEEP_REFS))
    n_reads = int(rng.choice([1, 2, 3, 7, 40, 65]))
    dens = float(rng.choice([0.0, 0.01, 0.1, 0.5, 1.0]))
    t = (rng.integers(1, 256, (n_reads, n_refs)) * (rng.random((n_reads, n_refs)) < dens)).astype(np.uint8)
    t[rng.random(n_reads) < 0.2] = 0
    norm, beta, _ = BETA_TRIPLES[i % 3]
    return _table(f"fuzz_{i}", n_reads, n_refs, t, [(norm, beta), (85, float(rng.choice([-1.0, 0.0, 0.5])))])


TABLE_CASES = {
    **{f"shared_group_{n}": (lambda n=n: shared_group(n)) for n in SHARED_REFS},
    "one_bit": one_bit,
    **{f"sweep_edges_{n}": (lambda n=n: sweep_edges(n)) for n in SWEEP_REFS},
    **{f"grid_stride_{a}x{b}": (lambda a=a, b=b: grid_stride(a, b)) for a, b in GRID_SHAPES},
    **{f"padding_{n}": (lambda n=n: padding(n)) for n in range(3, 19)},
    "beta_edges": beta_edges, "no_reads": no_reads, "all_zero": all_zero, "beyond_4g": beyond_4g,
}


# ---- cases for the route without the table ---------------------------------------------------------------------------------------------
def _free(name, n_reads, n_refs, cells, levels="1,1", tests=((85, 0.02),), seed=7, **facts):
    return Case(name=name, n_reads=n_reads, n_refs=n_refs, cells=cells, levels=levels, tests=list(tests), seed=seed, facts=facts)


def _edge_cells(n_reads, n_refs, region, **kw):
    lin = seg_edges(n_reads, n_refs, region)
    return Cells.at(lin, _vals(len(lin), **kw), n_refs)


def _long_in(n_reads, n_refs, region, v=40, off=12345):
    """a long cluster's cell inside a region (the region is then looked at piece by piece, or a wave per segment)"""
    ln = int(region_rows(n_reads, n_refs)[3][region])
    return Cells.at([(region << REGION_SHIFT) + off % ln], v, n_refs, [True])


SEGS_REFS = [253, 254, 255, 256, 257, 512]


def segs_258_259(n_refs):
    """FIN_SEGS on both sides: 65535 = 257 x 255, so EVERY whole region of a 255-wide table has exactly 258 row segments, the most the LDS looks
    take; 254-wide tables have 259 or 260 (a wave per segment), 253-wide ones 260 or 261, 256- and 257-wide ones 256.  Cells at the first and
    last byte of every segment of region 1, a few in the other regions; region 2 is looked at piece by piece (a long cluster's cell)."""
    n_reads = 3 * REGION // n_refs + 10
    cells = _edge_cells(n_reads, n_refs, 1) + _edge_cells(n_reads, n_refs, 2, span=90) + _long_in(n_reads, n_refs, 2) + \
        Cells.of([(0, 0, 5), (3, n_refs - 1, 77), (n_reads - 1, n_refs - 1, 9)])
    return _free(f"segs_258_259_{n_refs}", n_reads, n_refs, cells)


SHORT_TAIL = [(n, t) for n in (16, 17, 100, 255) for t in (1, 3, 258)] + [(83, 258)]        # (83: the segment estimate is one too low at byte 83)


def small_refs_short_tail(n_refs, tail_segs):
    """16 <= n_refs < 256: only a short last region has few enough segments for the LDS looks -- 1, 3 and 258 of them.  (255-wide: every whole
    region has 258 and no shorter one can, so that table ends with a whole region: 65536 rows, 255 regions)"""
    n_reads = REGION // n_refs + 1
    while int(region_rows(n_reads, n_refs)[2][-1]) != tail_segs or len(region_rows(n_reads, n_refs)[2]) < 2:
        n_reads += 1
        if n_reads >= 4 * REGION // n_refs:
            n_reads = REGION
            assert int(region_rows(n_reads, n_refs)[2][-1]) == tail_segs
    last = len(region_rows(n_reads, n_refs)[0]) - 1
    cells = _edge_cells(n_reads, n_refs, last) + Cells.of([(0, 0, 5), (1, n_refs - 1, 200), (2, 1, 1)])
    return _free(f"small_refs_short_tail_{n_refs}_{tail_segs}", n_reads, n_refs, cells, tail=last)


def tiny_refs(n_refs):
    """n_refs < 16: always a wave per segment, thousands of segments per region"""
    n_reads = 2 * REGION // n_refs + 77
    rng = np.random.default_rng(n_refs)
    lin = np.unique(np.concatenate([rng.integers(0, n_reads * n_refs, 500), [0, REGION - 1, REGION, 2 * REGION - 1, 2 * REGION, n_reads * n_refs - 1]]))
    return _free(f"tiny_refs_{n_refs}", n_reads, n_refs, Cells.at(lin, _vals(len(lin), span=250), n_refs))


def _dense_region(n_reads, n_refs, region, n, seed, avoid=()):
    """n distinct cells of a region, values 1 .. 3"""
    ln = int(region_rows(n_reads, n_refs)[3][region])
    pool = np.setdiff1d(np.arange(ln), np.asarray(list(avoid), dtype=np.int64) - (region << REGION_SHIFT))
    off = np.random.default_rng(seed).choice(pool, n, replace=False)
    return Cells.at(np.sort(off) + (region << REGION_SHIFT), 1 + np.arange(n) % 3, n_refs)


def _border_pairs(n_refs, region, k):
    """the last cell of row r and the first of row r + 1 inside ONE 16-byte piece, 255 | 1, and 1 | 255 at the next such border; rows well inside
    the region, other rows (and so other offsets in the region) for every k"""
    r = ((region << REGION_SHIFT) + n_refs - 1) // n_refs + 5 + 11 * k
    out = []
    for a, b in ((255, 1), (1, 255)):
        while ((r + 1) * n_refs) % 16 == 0:
            r += 1
        out += [(r, n_refs - 1, a), (r + 1, 0, b)]
        r += 3
    return Cells.of(out)


def border_in_piece():
    """a row border inside a 16-byte piece with different values on either side: region 0 gets the walk over the queues, regions 1 .. 3 are forced to
    fin_region_rows by a wrapping cell elsewhere in the region, by a long cluster's cell, by 6145 cells"""
    n_reads, n_refs = 900, 300
    pairs = [_border_pairs(n_refs, k, k) for k in range(4)]
    cells = pairs[0] + pairs[1] + Cells.of([(230, 17, 256 + 44)]) + pairs[2] + _long_in(n_reads, n_refs, 2) + \
        pairs[3] + _dense_region(n_reads, n_refs, 3, NWV * QW + 1 - 4, 5, avoid=pairs[3].lin(n_refs)) + Cells.of([(n_reads - 1, 7, 3)])
    return _free("border_in_piece", n_reads, n_refs, cells, tests=[(85, 0.02), (85, -1.0)], pairs=pairs)


ESTIMATE_REFS = [255, 257, 300, 1027, 65535, 65537]
ESTIMATE_LOW = [307, 425]             # widths at which the estimate is one too low at the first byte of dozens of rows (at the six above it is right everywhere)


def seg_estimate(n_refs, forced):
    """the segment of a byte by one multiplication with float(1 / n_refs), corrected by one: cells at the first and last byte of every segment of
    the region whose first byte lies deepest in its row and of region 0 (offset 0); forced: both regions looked at piece by piece (a long
    cluster's cell each), else by the walk over the queues"""
    n_reads = max(6, 8 * REGION // n_refs + 3)
    o0 = region_rows(n_reads, n_refs)[1]
    deep = int(np.argmax(o0))
    cells = _edge_cells(n_reads, n_refs, 0) + _edge_cells(n_reads, n_refs, deep, span=120) + Cells.of([(n_reads - 1, n_refs - 1, 2)])
    if forced:
        cells = cells + _long_in(n_reads, n_refs, 0) + _long_in(n_reads, n_refs, deep, v=101)
    return _free(f"seg_estimate_{n_refs}_{'rows' if forced else 'walk'}", n_reads, n_refs, cells, deep=deep, forced=forced)


ESTIMATE_WIDE = [(1 << 25) - 4]


def seg_estimate_wide(n_refs):
    """the one kind of width at which the estimate is one too HIGH: 2^25 - 4 -- the last byte of row 0, x = 2^25 - 5, becomes float 2^25 - 4, which is
    float(n_refs), and the product 1.0.  (Below 2^24 bytes per row float(x) is exact and the estimate is right or one too low.)  Two rows of 512
    regions each; cells on both sides of the border between the rows and at the table's ends."""
    cells = Cells.of([(0, 0, 3), (0, n_refs - 2, 6), (0, n_refs - 1, 200), (1, 0, 100), (1, 1, 7), (1, n_refs - 1, 5)])
    return _free(f"seg_estimate_wide_{n_refs}", 2, n_refs, cells, levels="1,2", tests=[(85, 0.02), (200, 0.6)])


def queue_overflow():
    """region 1: 6145 distinct cells -- eight waves share them, so one queues more than 768; region 2: exactly 768 cells -- no queue can overflow"""
    n_reads, n_refs = 700, 300
    cells = _dense_region(n_reads, n_refs, 1, NWV * QW + 1, 1) + _dense_region(n_reads, n_refs, 2, QW, 2) + Cells.of([(0, 0, 9), (n_reads - 1, 299, 8)])
    return _free("queue_overflow", n_reads, n_refs, cells, tests=[(85, 0.02), (85, 0.03)])


def wraps():
    """cells whose sums are 255, 256 and 257 in one region; a row whose only cell sums to 256: its maximum is 0, it fails at beta 0 and passes at
    beta -1 with an empty list; region 2 has a lone cell of 512"""
    n_reads, n_refs = 600, 400
    cells = Cells.of([(10, 5, 255), (11, 6, 256), (12, 7, 257), (11, 9, 3), (20, 399, 256), (21, 0, 1), (400, 100, 512), (401, 3, 2), (599, 399, 255)])
    return _free("wraps", n_reads, n_refs, cells, tests=[(85, -1.0), (85, 0.0), (85, 0.02)], lone_256_row=20)


def big_records():
    """a long cluster's cell in a region nothing else writes (2), one in a region with cells from the scan (1), the same cell from both sources
    -- 216 + 40 = 256: absent -- and 10 + 40 (region 0); region 3 has cells from the scan only"""
    n_reads, n_refs = 1000, 300
    cells = Cells.of([(500, 10, 40, True), (250, 7, 101, True), (251, 8, 3), (252, 299, 200),
                      (5, 5, 216), (5, 5, 40, True), (6, 6, 10), (6, 6, 40, True), (7, 0, 1), (700, 1, 6), (999, 299, 3)])
    return _free("big_records", n_reads, n_refs, cells, tests=[(85, 0.02), (85, -1.0), (85, 0.0)])


LONG_REFS = [65536, 65537, 131072, 200000, 196613]


def long_rows(n_refs):
    """rows of one to four regions.  Row 0: cells only in its first region; 1: only in its last; 2: only in a middle one (rows of three regions
    and more); 3: empty; 4: passes, cells in its first and last region, the regions between hold nothing; 5: fails (a 1); 6: passes because of ONE
    cell in its last region and has 1s in its first; 7: fails; 8: passes; 9, 10: fail (at every width a region between them has no passing row); 11: passes.  (norm 85, beta 0.02: a maximum of 1 fails)"""
    n_reads = 12
    first = lambda r: (r * n_refs) >> REGION_SHIFT
    last = lambda r: ((r + 1) * n_refs - 1) >> REGION_SHIFT
    in_reg = lambda r, k, d: max(r * n_refs, k << REGION_SHIFT) + d - r * n_refs          # a genome of row r inside region k
    items = [(0, in_reg(0, first(0), d), 50 + d) for d in (0, 1, 17)]
    tail = 2 * n_refs - (last(1) << REGION_SHIFT)                                         # bytes of row 1 in its last region
    items += [(1, n_refs - 1 - d, 60 + d) for d in (0, 1, 300) if d < tail]
    mid = (first(2) + last(2)) // 2
    items += [(2, in_reg(2, mid, d), 70 + d) for d in (3, 4, 200)]
    items += [(4, 0, 9), (4, 2, 8), (4, n_refs - 1, 7), (4, n_refs - 3, 6)]
    items += [(5, n_refs // 2, 1)]
    items += [(6, 0, 1), (6, 5, 1), (6, 6, 1), (6, n_refs - 1, 90)]
    items += [(7, 1, 1), (7, n_refs - 2, 1)]
    items += [(8, 0, 2), (8, n_refs - 1, 255)]
    items += [(9, 3, 1), (10, n_refs - 4, 1), (11, 7, 33)]
    return _free(f"long_rows_{n_refs}", n_reads, n_refs, Cells.of(items), levels="1,2", tests=[(85, 0.02), (85, 0.0), (85, -1.0)], mid=mid)


MANY_SHAPE = (460_000, 300)
MANY_SHAPE_SEGS = (1_380_000, 100)    # the same bytes in rows of 100: 656 or 657 segments per region, a wave per segment everywhere


def many_regions(segs=False):
    """2106 regions: more than twice any launch of k_apply_tiles (at most 1050 resident workgroups are assumed; the source says 512), so every
    workgroup walks several and what it carries from a region to its next -- the all-zero LDS copy, the zeroed segment words, the queue overflow
    flag of either parity, the prefetched region rows -- meets every kind of neighbour.  A region's kind is drawn (seeded): empty, a few cells, a
    wrap or a long cluster's cell with equal chances, and about one region in sixteen holds 6145 cells.  (Kinds that repeat every 4 or 16 regions
    would show a workgroup of a grid of 512 ONE kind.)  Regions 0, 511, 512, 513, 1023, 1024 and the last hold a cell in any case.
    segs: the same in rows of 100 bytes -- fin_region<1> looks at every region and leaves its LDS copy as it is: the next region must clear it."""
    n_reads, n_refs = MANY_SHAPE_SEGS if segs else MANY_SHAPE
    nreg = len(region_rows(n_reads, n_refs)[0])
    rng = np.random.default_rng(98 if segs else 99)
    parts = []
    kind = rng.integers(0, 4, nreg)
    kind[rng.random(nreg) < 1 / 16] = 4
    k = np.arange(nreg)
    lens = region_rows(n_reads, n_refs)[3]
    pick = lambda regs, n: ((np.repeat(regs, n).astype(np.int64) << REGION_SHIFT) + rng.integers(0, int(lens.min()), len(regs) * n))
    few = k[kind == 1]
    lin = np.unique(pick(few, 5))
    parts.append(Cells.at(lin, _vals(len(lin)), n_refs))
    wr = k[kind == 2]
    lin = np.unique(pick(wr, 1))
    parts.append(Cells.at(lin, 256 + 2 + np.arange(len(lin)) % 50, n_refs))
    lin = np.unique(pick(wr, 3))
    parts.append(Cells.at(lin, 1 + np.arange(len(lin)) % 9, n_refs))
    lg = k[kind == 3]
    lin = np.unique(pick(lg, 1))
    parts.append(Cells.at(lin, 40 + 2 * (np.arange(len(lin)) % 30), n_refs, np.ones(len(lin), bool)))
    lin = np.unique(pick(lg, 2))
    parts.append(Cells.at(lin, 2 + np.arange(len(lin)) % 5, n_refs))
    for r in k[kind == 4]:
        off = rng.choice(int(lens[r]), NWV * QW + 1, replace=False)
        parts.append(Cells.at(np.sort(off) + (int(r) << REGION_SHIFT), 1 + np.arange(len(off)) % 3, n_refs))
    always = [0, 511, 512, 513, 1023, 1024, nreg - 1]
    parts.append(Cells.at([(r << REGION_SHIFT) + 1000 + r for r in always], 3, n_refs))
    cells = parts[0]
    for p in parts[1:]:
        cells = cells + p
    return _free("many_regions_segs" if segs else "many_regions", n_reads, n_refs, cells, levels="2,3", tests=[(85, 0.03)], seed=3, always=always, kind=kind)


def table_end():
    """the table ends inside a region and inside a 16-byte piece; its last cell is set"""
    n_reads, n_refs = 129, 1027
    cells = Cells.of([(128, 1026, 77), (128, 1025, 1), (128, 0, 3), (127, 1026, 5), (63, 837, 8), (64, 0, 200), (0, 0, 1)])
    return _free("table_end", n_reads, n_refs, cells, tests=[(85, 0.02), (85, 0.0)])


FUZZ_FREE = 20


def fuzz_free(i):
    """a seeded sparse table of 2 .. 40 regions, its shape drawn from the sets above"""
    rng = np.random.default_rng(70_000 + i)
    n_refs = int(rng.choice(SEGS_REFS + ESTIMATE_REFS + LONG_REFS[:2] + [1, 15, 16, 17, 100, 200000]))
    nreg = int(rng.integers(2, 41))
    n_reads = max(2, (nreg * REGION - int(rng.integers(0, REGION - 1))) // n_refs)
    if sim_bytes(n_reads, n_refs) <= REGION:
        n_reads = REGION // n_refs + 2
    total = n_reads * n_refs
    lin = np.unique(rng.integers(0, total, int(rng.choice([20, 300, 3000]))))
    v = np.where(rng.random(len(lin)) < 0.02, 256 + rng.integers(0, 3, len(lin)), rng.integers(1, 256, len(lin)))
    cells = Cells.at(lin, v, n_refs)
    lin2 = np.unique(rng.integers(0, total, 6))
    cells = cells + Cells.at(lin2, rng.integers(33, 256, len(lin2)), n_refs, np.ones(len(lin2), bool))
    return _free(f"fuzz_free_{i}", n_reads, n_refs, cells, levels=["1,1", "1,2", "2,3"][i % 3] if nreg > 3 else "1,1",
                 tests=[(85, float(rng.choice([-1.0, 0.0, 0.02, 0.5])))], seed=i)


FREE_CASES = {
    **{f"segs_258_259_{n}": (lambda n=n: segs_258_259(n)) for n in SEGS_REFS},
    **{f"small_refs_short_tail_{n}_{t}": (lambda n=n, t=t: small_refs_short_tail(n, t)) for n, t in SHORT_TAIL},
    **{f"tiny_refs_{n}": (lambda n=n: tiny_refs(n)) for n in (1, 3, 15)},
    "border_in_piece": border_in_piece,
    **{f"seg_estimate_{n}_{'rows' if f else 'walk'}": (lambda n=n, f=f: seg_estimate(n, f)) for n in ESTIMATE_REFS + ESTIMATE_LOW for f in (False, True)},
    **{f"seg_estimate_wide_{n}": (lambda n=n: seg_estimate_wide(n)) for n in ESTIMATE_WIDE},
    "queue_overflow": queue_overflow, "wraps": wraps, "big_records": big_records,
    **{f"long_rows_{n}": (lambda n=n: long_rows(n)) for n in LONG_REFS},
    "many_regions": many_regions, "many_regions_segs": (lambda: many_regions(True)), "table_end": table_end,
    **{f"fuzz_free_{i}": (lambda i=i: fuzz_free(i)) for i in range(FUZZ_FREE)},
}
GROUPED = ["border_in_piece", "queue_overflow"] + [f"long_rows_{n}" for n in LONG_REFS]      # the cases that also run with LIME_APPLY_GROUP 1 .. 6


def make(name):
    case = (TABLE_CASES.get(name) or FREE_CASES[name])()
    assert case.name == name
    if isinstance(case.cells, np.ndarray):
        case.cells.setflags(write=False)
    else:
        for a in (case.cells.r, case.cells.g, case.cells.v, case.cells.long):
            a.setflags(write=False)
    return case
