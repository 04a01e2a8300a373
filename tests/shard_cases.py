"""What the tests of the genome-shard path share (test_shard_cases_cpu.py, test_listcat_edges_gpu.py, test_sample_shards_gpu.py): numpy
models of clusterChoose on a whole score table and of the concatenation of its column shards' lists (lime_lists_concat_dev's rule), and
the seeded sparse tables, cuts and hand-made rows both are tried on.  No GPU and no library call here."""
import numpy as np

SEED = 20311
NORM, BETA = 85, 0.25                                # readLen 100, alpha 16: 21 / 85 fails the test and 22 / 85 passes it
ROW_LENGTHS = (0, 1, 63, 64, 65, 200)                # pairs in a row, across the parts


def passes(mx, norm, beta):
    """clusterChoose's test in the reference's types (ClusterBWT_DA.cpp:404-406): float(max) / norm > beta"""
    return np.float32(mx) / np.float32(norm) > np.float32(beta)


def choose(table, norm, beta):
    """clusterChoose of a whole table -> (row_max u8[n], row_off u64[n + 1], pairs u32[k, 2] = (idRef, sim), ascending idRef in a row)"""
    table = np.asarray(table, dtype=np.uint8)
    n_reads = table.shape[0]
    row_max = table.max(axis=1).astype(np.uint8) if table.shape[1] else np.zeros(n_reads, np.uint8)
    keep = passes(row_max, norm, beta)
    rows, cols = np.nonzero(table * keep[:, None])
    pairs = np.stack([cols.astype(np.uint32), table[rows, cols].astype(np.uint32)], axis=1).reshape(-1, 2)
    row_off = np.zeros(n_reads + 1, dtype=np.uint64)
    np.cumsum(np.bincount(rows, minlength=n_reads), out=row_off[1:])
    return row_max, row_off, pairs


def concat(parts, id_base, norm, beta):
    """the rule of lime_lists_concat_dev on host copies: parts = [(row_max, row_off, pairs)], each made with a beta every non-zero row
    passes.  The maximum over the parts decides; a passing row is its parts' rows one after the other with id_base added"""
    n_reads = len(parts[0][0])
    row_max = np.zeros(n_reads, dtype=np.uint8)
    for mx, _, _ in parts:
        row_max = np.maximum(row_max, mx)
    keep = passes(row_max, norm, beta)
    out, row_off = [], np.zeros(n_reads + 1, dtype=np.uint64)
    for r in range(n_reads):
        n = 0
        if keep[r]:
            for (_, off, pairs), base in zip(parts, id_base):
                p = np.array(pairs[int(off[r]):int(off[r + 1])], dtype=np.uint64).reshape(-1, 2)
                p[:, 0] += np.uint64(base)
                out.append(p)
                n += len(p)
        row_off[r + 1] = row_off[r] + np.uint64(n)
    pairs = (np.concatenate(out) if out else np.zeros((0, 2), np.uint64)).astype(np.uint32).reshape(-1, 2)
    return row_max, row_off, pairs


def same_lists(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)) and np.asarray(a[2]).shape == np.asarray(b[2]).shape


def cuts(n_refs, n_parts, rng):
    """n_parts + 1 ascending column cuts of 0 .. n_refs, every part with at least one column"""
    assert 1 <= n_parts <= n_refs
    inner = np.sort(rng.choice(np.arange(1, n_refs), size=n_parts - 1, replace=False)) if n_parts > 1 else np.zeros(0, np.int64)
    return [0] + [int(x) for x in inner] + [n_refs]


def sparse_table(n_reads, n_refs, rng, density=0.05, top=60):
    """a seeded sparse u8 table: most cells 0, values 1 .. top (both sides of the 21 / 22 threshold of NORM, BETA), some rows all zero"""
    t = (rng.integers(1, top + 1, size=(n_reads, n_refs)) * (rng.random((n_reads, n_refs)) < density)).astype(np.uint8)
    if n_reads > 3:
        t[rng.integers(0, n_reads, size=max(1, n_reads // 8))] = 0
    return t


def handmade(col_cuts):
    """rows that pin the rule on the parts col_cuts gives (at least 3 parts of at least 2 columns): -> (table, what each row is)"""
    assert len(col_cuts) >= 4 and all(b - a >= 2 for a, b in zip(col_cuts, col_cuts[1:]))
    n_refs, first, mid, last = col_cuts[-1], col_cuts[0], col_cuts[1], col_cuts[-2]
    rows, names = [], []

    def row(name, cells):
        r = np.zeros(n_refs, dtype=np.uint8)
        for c, v in cells.items():
            r[c] = v
        rows.append(r); names.append(name)
    row("maximum in the first part", {first: 40, mid: 3, last: 5})
    row("maximum in a middle part", {first: 3, mid + 1: 40, last: 5})
    row("maximum in the last part", {first: 3, mid: 5, n_refs - 1: 40})
    row("passes only through another part's maximum", {first: 1, first + 1: 2, mid: 22})      # the first part's own maximum, 2, would fail
    row("21 in every part: fails", {first: 21, mid: 21, last: 21})
    row("21 and 22: passes, the 21s listed too", {first: 21, mid: 22, last: 21})
    row("22 alone in the last part", {n_refs - 1: 22})
    row("empty in some parts", {mid: 30})
    row("empty in all parts", {})
    row("255", {first: 255, n_refs - 1: 255})
    return np.stack(rows), names


def rows_of_lengths(n_refs, rng, lengths=ROW_LENGTHS):
    """one passing row per length in `lengths` (as many non-zero cells, spread over the columns; n_refs >= max(lengths))"""
    t = np.zeros((len(lengths), n_refs), dtype=np.uint8)
    for r, n in enumerate(lengths):
        cols = rng.choice(n_refs, size=n, replace=False)
        t[r, cols] = rng.integers(30, 200, size=n)
    return t


def split(table, col_cuts):
    """the column shards of a table"""
    return [np.ascontiguousarray(table[:, a:b]) for a, b in zip(col_cuts, col_cuts[1:])]
