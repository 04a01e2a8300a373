"""tests/choose_cases.py without a GPU: the sparse model against a row-by-row loop over a dense table, the collections arrays_of() makes against the
oracle (their table is the chosen one, without ebwt and with one repeated base), and every named case against the edge it is named for, so that
tests/test_choose_edges_gpu.py cannot lose one quietly when a generator changes.  A case that does not hold its edge fails here."""
import functools

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import choose_cases as CC

R = CC.REGION


@functools.lru_cache(maxsize=4)
def _case(name):
    return CC.make(name)


def _same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 4


# ---- the model -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CC.TABLE_CASES if not n.startswith("grid_stride") and n != "beyond_4g"])
def test_model_equals_a_loop_over_the_rows(name):
    c = _case(name)
    dense = CC.dense_of(c.cells, c.n_reads, c.n_refs)
    for norm, beta in c.tests:
        assert _same(CC.choose_model(c.cells, c.n_reads, c.n_refs, norm, beta), CC.choose_naive(dense, norm, beta)), (norm, beta)


def test_model_equals_a_loop_over_the_rows_fuzz():
    for i in range(CC.FUZZ_TABLES):
        c = CC.fuzz_table(i)
        for norm, beta in c.tests:
            assert _same(CC.choose_model(c.cells, c.n_reads, c.n_refs, norm, beta), CC.choose_naive(c.cells, norm, beta)), i


# (the three tables of 67 and 138 MB are left to the sparse model: as Python lists they take gigabytes)
@pytest.mark.parametrize("name", [n for n in CC.FREE_CASES if not n.startswith("many_regions") and not n.startswith("seg_estimate_wide")])
def test_model_equals_a_loop_over_the_rows_sparse_cases(name):
    c = _case(name)
    assert c.n_reads * c.n_refs <= 1 << 24
    dense = CC.dense_of(c.cells, c.n_reads, c.n_refs)
    for norm, beta in c.tests:
        assert _same(CC.choose_model(c.cells, c.n_reads, c.n_refs, norm, beta), CC.choose_naive(dense, norm, beta)), (norm, beta)


def test_model_takes_every_description_and_drops_sums_of_zero():
    want = CC.choose_model(np.array([[0, 44, 0], [0, 0, 0], [1, 0, 255]], np.uint8), 3, 3, 4, 0.25)
    assert want[0].tolist() == [44, 0, 255] and want[1].tolist() == [1, 0, 2] and want[2].tolist() == [0, 1, 1, 3]
    assert want[3].tolist() == [[1, 44], [0, 1], [2, 255]]
    for x in ({(0, 1): 300, (2, 0): 1, (2, 2): 255, (1, 1): 256}, ([0, 2, 2, 1, 1], [1, 0, 2, 1, 1], [300, 1, 255, 255, 1]),
              CC.Cells.of([(0, 1, 150), (0, 1, 150), (2, 0, 1), (2, 2, 255, True), (1, 2, 512)])):
        assert _same(CC.choose_model(x, 3, 3, 4, 0.25), want)


# ---- the builder against the oracle ------------------------------------------------------------------------------------------------------
def test_builder_values_the_way_they_were_asked():
    """1, 33 and 255 come out as asked, 256 as 0, 300 as 44; a long cluster of 40 + 40 gives 40, one of 101 reads and 267 genomes 101"""
    cells = CC.Cells.of([(0, 0, 1), (0, 1, 33), (1, 0, 255), (1, 1, 256), (2, 2, 300), (3, 0, 40, True), (3, 2, 101, True)])
    cr, cg, kr, kg = CC.clusters_of(cells)
    assert kr.max() == 101 and sorted((kr + kg)[-2:].tolist()) == [80, 368] and (kr[:-2] <= CC.MAX_K).all() and (kr[:-2] == kg[:-2]).all()
    for eb in (None, CC.BASE):
        for seed in (None, 4):
            lcp, da, e = CC.arrays_of(cells, 4, 3, ebwt=eb, seed=seed)
            cl, nc, ml = O.detect(lcp, da, 4, CC.ALPHA)
            assert nc == CC.n_clusters_of(cells) == len(cr) and ml == 368
            assert O.score(da, e, cl, 4, 3).tolist() == [[1, 33, 0], [255, 0, 0], [0, 0, 44], [40, 0, 101]]


@pytest.mark.parametrize("name", list(CC.FREE_CASES))
def test_oracle_table_of_the_collection_is_the_chosen_one(name):
    c = _case(name)
    lin, val = CC.table_of(c.cells, c.n_reads, c.n_refs)
    for eb in (None, CC.BASE):
        lcp, da, e = CC.arrays_of(c.cells, c.n_reads, c.n_refs, ebwt=eb, seed=c.seed)
        cl, nc, ml = O.detect(lcp, da, c.n_reads, CC.ALPHA)
        assert nc == CC.n_clusters_of(c.cells)
        assert (ml > CC.MID_MAX) == bool(c.cells.long.any()) and ml <= 65536
        sim = O.score(da, e, cl, c.n_reads, c.n_refs, threads=4).reshape(-1)
        got = np.flatnonzero(sim)
        assert np.array_equal(got, lin) and np.array_equal(sim[got], val)
    # the layout the case asks for has a second level: the call goes without the table
    assert len(CC.region_rows(c.n_reads, c.n_refs)[0]) > int(c.levels.split(",")[0]) and c.n_refs < 1 << 25
    # only the long clusters arrive as 64-bit records: every other one closes inside the read-ahead of the scan window it begins in -- looked up in
    # the arrays themselves, cluster by cluster
    assert CC.n_big_of(c.cells, c.seed) == (int(c.cells.long.sum()), 0)
    s, ln = cl[:, 0].astype(np.int64), cl[:, 1].astype(np.int64)
    late = s + ln >= (s // CC.WIN + 1) * CC.WIN + CC.HALO
    assert not (late & (ln <= CC.MID_MAX)).any() and int((late | (ln > CC.MID_MAX)).sum()) == int(c.cells.long.sum())


@pytest.mark.parametrize("name", ["seg_estimate_307_walk", "border_in_piece", "segs_258_259_255"])
def test_collection_with_clusters_across_the_scan_windows(name):
    """arrays_of(fit=False): the same table, and short clusters that do not close inside their window's read-ahead -- in regions that hold no long one"""
    c = _case(name)
    lin, val = CC.table_of(c.cells, c.n_reads, c.n_refs)
    lcp, da, e = CC.arrays_of(c.cells, c.n_reads, c.n_refs, seed=c.seed, fit=False)
    cl, nc, ml = O.detect(lcp, da, c.n_reads, CC.ALPHA)
    sim = O.score(da, e, cl, c.n_reads, c.n_refs, threads=4).reshape(-1)
    got = np.flatnonzero(sim)
    assert nc == CC.n_clusters_of(c.cells) and np.array_equal(got, lin) and np.array_equal(sim[got], val)
    n_big, n_short = CC.n_big_of(c.cells, c.seed, fit=False)
    s, ln = cl[:, 0].astype(np.int64), cl[:, 1].astype(np.int64)
    late = s + ln >= (s // CC.WIN + 1) * CC.WIN + CC.HALO
    assert n_short == int((late & (ln <= CC.MID_MAX)).sum()) > 3 and n_big == int((late | (ln > CC.MID_MAX)).sum())
    region = (da[s[late]].astype(np.int64) * c.n_refs + da[(s + ln - 1)[late]] - c.n_reads) >> 16       # (a cluster: its reads, then its genomes)
    lk = CC.looks(c.cells, c.n_reads, c.n_refs)
    assert any(lk[k] == "walk" for k in region.tolist())          # (the look with fit; here that region is looked at piece by piece)


# ---- the geometry ------------------------------------------------------------------------------------------------------------------------
def test_region_rows_against_a_loop():
    for n_reads, n_refs in [(900, 300), (9, 200000), (4097, 16), (140000, 1), (129, 1027), (514, 255)]:
        r0, o0, nseg, ln = CC.region_rows(n_reads, n_refs)
        tb = n_reads * n_refs
        assert len(r0) == -(-tb // R) and int(ln.sum()) == tb
        for k in range(len(r0)):
            rows = {b // n_refs for b in (k * R, k * R + int(ln[k]) - 1)}
            assert int(r0[k]) == min(rows) and int(nseg[k]) == max(rows) - min(rows) + 1 and int(o0[k]) == k * R - min(rows) * n_refs


def _looks(c):
    return CC.looks(c.cells, c.n_reads, c.n_refs)


# ---- with the table: every case holds its edge --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_refs", CC.SHARED_REFS)
def test_shared_group(n_refs):
    c = _case(f"shared_group_{n_refs}")
    t = c.cells
    assert c.n_reads == 40 and CC.SHARED_REFS == [1, 2, 3, 5, 15, 16, 17, 31, 33, 47]
    rows = c.facts["rows"]
    for r, k in enumerate(rows):
        if k == "F":
            assert (t[r] == 255).all()
        elif k == "E":
            assert not t[r].any()
        elif k in "az":
            assert t[r].sum() == 1 and t[r, 0 if k == "a" else -1] == 1
    assert "FaF" in rows and "FzF" in rows and "FEF" in rows and "FEEF" in rows
    if n_refs < 16:                                                     # rows whose first and last 16-byte group are the same one, and rows that cross a border
        q0, q1 = (np.arange(40) * n_refs) >> 4, (np.arange(40) * n_refs + n_refs - 1) >> 4
        assert (q0 == q1).any() and (16 % n_refs == 0 or (q0 != q1).any())
    mx = CC.choose_model(t, 40, n_refs, 85, 0.02)[0]
    assert {0, 1, 255} <= set(mx.tolist())


def test_one_bit():
    c = _case("one_bit")
    lin = c.cells.lin(c.n_refs)
    assert {(int(v), int(b & 3)) for v, b in zip(c.cells.v, lin)} == {(1 << b, p) for b in range(8) for p in range(4)}
    assert (np.bincount(c.cells.r, minlength=32) == 1).all()


@pytest.mark.parametrize("n_refs", CC.SWEEP_REFS)
def test_sweep_edges(n_refs):
    c = _case(f"sweep_edges_{n_refs}")
    assert CC.SWEEP_REFS == [253, 254, 255, 256, 257, 258, 259, 260, 511, 513, 1008, 1023, 1024, 1025, 1040, 2049]
    mx, nnz, _, _ = CC.choose_model(c.cells, c.n_reads, n_refs, 85, 0.0)
    for r in c.facts["full_rows"]:
        assert nnz[r] == n_refs
    assert nnz[-1] == 0
    # the single cells: for either kernel the last byte of a sweep and the first of the next, where the row is long enough to have one
    single = np.flatnonzero(nnz == 1)
    lin = c.cells.lin(n_refs)
    sides = {CC.CHOOSE_SWEEP: set(), CC.GATHER_SWEEP: set()}
    for r in single:
        b = int(lin[c.cells.r == r][0])
        for sweep, unit in ((CC.CHOOSE_SWEEP, 16), (CC.GATHER_SWEEP, 4)):
            d = b - r * n_refs // unit * unit
            if d >= sweep and d % sweep == 0:
                sides[sweep].add(0)
            if d % sweep == sweep - 1:
                sides[sweep].add(-1)
    if n_refs >= 260:
        assert sides[CC.GATHER_SWEEP] == {-1, 0}
    if n_refs >= 1025:
        assert sides[CC.CHOOSE_SWEEP] == {-1, 0}
    if n_refs >= 1024:
        assert -1 in sides[CC.CHOOSE_SWEEP]
    assert -1 in sides[CC.GATHER_SWEEP] or n_refs < 256


def test_grid_stride():
    assert CC.GRID_SHAPES == [(262149, 3), (65539, 5)]
    for (n_reads, n_refs), caps in zip(CC.GRID_SHAPES, ((CC.CHOOSE_CAP, CC.GATHER_CAP), (CC.GATHER_CAP,))):
        c = _case(f"grid_stride_{n_reads}x{n_refs}")
        _, _, off, pairs = CC.choose_model(c.cells, n_reads, n_refs, 85, 0.02)
        n = np.diff(off.astype(np.int64))
        for cap in caps:
            assert n_reads > cap and all(n[r] > 0 for r in (0, cap - 1, cap, cap + 1, n_reads - 1))
            assert n[cap - 2] == 0 and (n[cap + 2] == 0 or cap + 2 == n_reads - 1) and (cap - 2) in c.facts["failing"]
        assert (n[c.facts["failing"]] == 0).all() and (n[c.facts["marked"]] > 0).all() and len(c.facts["failing"]) > 60
        assert len(pairs) == int(n.sum()) > 0


def test_padding_ends_at_every_residue():
    assert {(n * 17) % 16 for n in range(3, 19)} == set(range(16))
    for n in range(3, 19):
        c = _case(f"padding_{n}")
        assert (c.n_reads, c.n_refs) == (n, 17) and int(c.cells.lin(17).max()) == n * 17 - 1


def test_beyond_4g():
    c = _case("beyond_4g")
    lin = c.cells.lin(c.n_refs)
    assert c.n_reads * c.n_refs > 4.5e9 and 65535 * c.n_refs == (1 << 32) - 1
    assert (lin < 1 << 32).sum() > 10 and (lin >= 1 << 32).sum() > 10 and (1 << 32) - 1 in lin and (1 << 32) in lin
    assert int(lin.max()) == c.n_reads * c.n_refs - 1 and 20 < len(c.cells) < 100
    _, _, off, _ = CC.choose_model(c.cells, c.n_reads, c.n_refs, 85, 0.02)
    n = np.diff(off.astype(np.int64))
    assert n[65534] and n[65535] and n[65536] and n[70000] and not n[65532] and not n[65538] and int((n > 0).sum()) == 8


def test_beta_edges():
    c = _case("beta_edges")
    rows = c.facts["maxima"]
    for norm, beta, m in CC.BETA_TRIPLES:
        assert np.float32(m) / np.float32(norm) == np.float32(beta)                       # the quotient equals beta exactly: m fails
        n = np.diff(CC.choose_model(c.cells, c.n_reads, c.n_refs, norm, beta)[2].astype(np.int64))
        assert n[rows.index(m)] == 0 and n[rows.index(m + 1)] > 0 and n[rows.index(m - 1)] == 0
    assert CC.BETA_TRIPLES == [(4, 0.25, 1), (100, 0.02, 2), (85, 0.2, 17)]
    mx, nnz, off, pairs = CC.choose_model(c.cells, c.n_reads, c.n_refs, 85, -1.0)
    assert mx[0] == 0 and off[1] == 0 and int(off[-1]) == int(nnz.sum()) == len(pairs)     # every row passes, the empty one lists nothing
    n = np.diff(CC.choose_model(c.cells, c.n_reads, c.n_refs, 85, 0.0)[2].astype(np.int64))
    assert n[0] == 0 and (n[1:] > 0).all()
    assert len(CC.choose_model(c.cells, c.n_reads, c.n_refs, 85, 3.0)[3]) == 0
    assert {(85, -1.0), (85, 0.0), (85, 3.0)} <= set(c.tests)
    assert _case("no_reads").n_reads == 0 and len(_case("all_zero").cells) == 0 and (85, -1.0) in _case("all_zero").tests


def test_fuzz_tables_draw_from_the_named_shapes():
    shapes = {(CC.fuzz_table(i).n_reads, CC.fuzz_table(i).n_refs) for i in range(CC.FUZZ_TABLES)}
    assert CC.FUZZ_TABLES == 200 and {s[1] for s in shapes} <= set(CC.SHARED_REFS + CC.SWEEP_REFS) and len(shapes) > 60


# ---- without the table: every case holds its edge ---------------------------------------------------------------------------------------
def _has_edges(c, region):
    """a non-zero cell at the first and at the last byte of every row segment of the region"""
    lin, _ = CC.table_of(c.cells, c.n_reads, c.n_refs)
    return np.isin(CC.seg_edges(c.n_reads, c.n_refs, region), lin).all()


@pytest.mark.parametrize("n_refs", CC.SEGS_REFS)
def test_segs_258_259(n_refs):
    """FIN_SEGS lies between 255-wide tables (every whole region: 258 segments) and 254-wide ones (259 or 260): no width has regions of 258 AND 259"""
    c = _case(f"segs_258_259_{n_refs}")
    nseg = CC.region_rows(c.n_reads, n_refs)[2]
    assert 3 <= len(nseg) <= 5
    want = {253: {260, 261}, 254: {259, 260}, 255: {258}, 256: {256}, 257: {256}, 512: {128, 129}}[n_refs]
    assert set(nseg[:-1].tolist()) <= want and int(nseg[1]) in want and int(nseg[2]) in want
    assert all(set(CC.region_rows(4000, w)[2][:-1].tolist()) != {258, 259} for w in range(250, 262))
    assert _has_edges(c, 1) and _has_edges(c, 2)
    lk = _looks(c)
    assert (lk[1], lk[2]) == (("walk", "rows") if n_refs >= 255 else ("segs", "segs"))


@pytest.mark.parametrize("n_refs,tail", CC.SHORT_TAIL)
def test_small_refs_short_tail(n_refs, tail):
    c = _case(f"small_refs_short_tail_{n_refs}_{tail}")
    nseg = CC.region_rows(c.n_reads, n_refs)[2]
    last = len(nseg) - 1
    assert 16 <= n_refs < 256 and int(nseg[-1]) == tail and c.facts["tail"] == last and (nseg[:-1] > CC.FIN_SEGS - (n_refs == 255)).all()
    lk = _looks(c)
    assert lk[-1] == "walk" and (n_refs == 255 or set(lk[:-1]) == {"segs"}) and _has_edges(c, last)


@pytest.mark.parametrize("n_refs", [1, 3, 15])
def test_tiny_refs(n_refs):
    c = _case(f"tiny_refs_{n_refs}")
    lk = _looks(c)
    assert len(lk) == 3 and set(lk) == {"segs"}
    lin, _ = CC.table_of(c.cells, c.n_reads, n_refs)
    assert {0, R - 1, R, 2 * R - 1, 2 * R, c.n_reads * n_refs - 1} <= set(lin.tolist())


def test_border_in_piece():
    c = _case("border_in_piece")
    t = CC.dense_of(c.cells, c.n_reads, c.n_refs).reshape(-1)
    for k, p in enumerate(c.facts["pairs"]):
        lin = p.lin(c.n_refs)
        assert len(lin) == 4 and (lin >> 16 == k).all()
        for a, b in ((0, 1), (2, 3)):
            assert lin[b] == lin[a] + 1 and lin[a] >> 4 == lin[b] >> 4 and p.r[b] == p.r[a] + 1      # neighbours in one 16-byte piece, in two rows
        assert t[lin].tolist() == [255, 1, 1, 255]
    first, wrap, big, risky = CC.region_facts(c.cells, c.n_reads, c.n_refs)
    assert _looks(c)[:4] == ["walk", "rows", "rows", "rows"]
    assert wrap.tolist()[:4] == [False, True, False, False] and big.tolist()[:4] == [False, False, True, False]
    assert first[3] == CC.NWV * CC.QW + 1 and first[0] <= CC.QW and not risky[0]


@pytest.mark.parametrize("n_refs", CC.ESTIMATE_REFS + CC.ESTIMATE_LOW)
def test_seg_estimate(n_refs):
    for forced in (False, True):
        c = _case(f"seg_estimate_{n_refs}_{'rows' if forced else 'walk'}")
        r0, o0, nseg, ln = CC.region_rows(c.n_reads, n_refs)
        deep = c.facts["deep"]
        assert o0[0] == 0 and o0[deep] == o0.max() > 0 and _has_edges(c, 0) and _has_edges(c, deep)
        lk = _looks(c)
        assert lk[0] == lk[deep] == ("rows" if forced else "walk")


def _estimate_error(n_refs, x0):
    """float(x0) * float(1 / n_refs), truncated, minus the row segment x0 lies in (fin_region_rows and the walk correct it by one)"""
    x = np.asarray(x0, dtype=np.int64)
    est = (x.astype(np.float32) * (np.float32(1.0) / np.float32(n_refs))).astype(np.int64)
    return est - x // n_refs


def test_seg_estimate_is_one_too_low_and_one_too_high_somewhere():
    """the six widths of the first list never need the correction at their segments' edges (float32 arithmetic in numpy); 307 and 425 need ++seg at
    the first byte of dozens of rows, 83 in the short-tail case too; only 2^25 - 4 needs --seg"""
    def edge_errors(name, w, k):
        c = _case(name)
        o0 = CC.region_rows(c.n_reads, w)[1]
        return _estimate_error(w, CC.seg_edges(c.n_reads, w, k) - (k << 16) + int(o0[k]))
    for w in CC.ESTIMATE_REFS:
        for k in (0, _case(f"seg_estimate_{w}_walk").facts["deep"]):
            assert not edge_errors(f"seg_estimate_{w}_walk", w, k).any()
    assert CC.ESTIMATE_LOW == [307, 425]
    for w in CC.ESTIMATE_LOW:
        e = edge_errors(f"seg_estimate_{w}_walk", w, 0)
        assert set(e.tolist()) == {-1, 0} and (e == -1).sum() >= 10
    c = _case("small_refs_short_tail_83_258")
    assert (edge_errors(c.name, 83, c.facts["tail"]) == -1).any()
    assert CC.ESTIMATE_WIDE == [(1 << 25) - 4]
    w = CC.ESTIMATE_WIDE[0]
    c = _case(f"seg_estimate_wide_{w}")
    assert w - 1 in CC.table_of(c.cells, 2, w)[0] and _estimate_error(w, w - 1).tolist() == 1 and not _estimate_error(w, [0, w - 2, w, w + 1]).any()
    lk = _looks(c)
    assert lk[(w - 1) >> 16] == "walk" and len(lk) == 1024 and w < 1 << 25
    # rows 0 and 1 pass at (85, 0.02); at (200, 0.6) only a maximum above 120 does
    assert (np.diff(CC.choose_model(c.cells, 2, w, 200, 0.6)[2].astype(np.int64)) > 0).tolist() == [True, False]


def test_queue_overflow():
    c = _case("queue_overflow")
    first, wrap, big, _ = CC.region_facts(c.cells, c.n_reads, c.n_refs)
    assert first[1] == 6145 == CC.NWV * CC.QW + 1 and first[2] == 768 == CC.QW and not wrap.any() and not big.any()
    assert _looks(c)[:3] == ["walk", "rows", "walk"]


def test_wraps():
    c = _case("wraps")
    lin = c.cells.lin(c.n_refs)
    assert {255, 256, 257} <= set(c.cells.v[lin >> 16 == 0].tolist())
    r = c.facts["lone_256_row"]
    assert c.cells.v[c.cells.r == r].tolist() == [256]
    mx, nnz, off, pairs = CC.choose_model(c.cells, c.n_reads, c.n_refs, 85, -1.0)
    assert mx[r] == 0 and nnz[r] == 0 and off[r + 1] == off[r] and off[-1] == nnz.sum()
    assert np.diff(CC.choose_model(c.cells, c.n_reads, c.n_refs, 85, 0.0)[2].astype(np.int64))[r] == 0
    assert _looks(c)[0] == "rows" and {(85, -1.0), (85, 0.0)} <= set(c.tests)
    assert CC.table_of(c.cells, c.n_reads, c.n_refs)[1].tolist().count(1) >= 2       # 257 -> 1


def test_big_records():
    c = _case("big_records")
    first, wrap, big, _ = CC.region_facts(c.cells, c.n_reads, c.n_refs)
    assert big.tolist()[:4] == [True, True, True, False] and first[2] == 0 and first[1] > 0 and first[3] > 0 and not wrap.any()
    t = CC.dense_of(c.cells, c.n_reads, c.n_refs)
    assert t[5, 5] == 0 and t[6, 6] == 50 and t[500, 10] == 40 and t[250, 7] == 101
    assert _looks(c)[:4] == ["rows", "rows", "rows", "walk"]


@pytest.mark.parametrize("n_refs", CC.LONG_REFS)
def test_long_rows(n_refs):
    c = _case(f"long_rows_{n_refs}")
    assert CC.LONG_REFS == [65536, 65537, 131072, 200000, 196613]
    lin, _ = CC.table_of(c.cells, c.n_reads, n_refs)
    per_region = np.bincount(lin >> 16, minlength=len(CC.region_rows(c.n_reads, n_refs)[0]))
    regs = lambda r: np.arange((r * n_refs) >> 16, (((r + 1) * n_refs - 1) >> 16) + 1)
    in_row = lambda r: np.unique(lin[lin // n_refs == r] >> 16)
    span = len(regs(1))
    assert span == {65536: 1, 65537: 2, 131072: 2, 200000: 4, 196613: 4}[n_refs] or n_refs in (200000, 196613)
    assert in_row(0).tolist() == [regs(0)[0]] and in_row(1).tolist() == [regs(1)[-1]] and len(in_row(3)) == 0
    if len(regs(2)) >= 3:
        assert in_row(2).tolist() == [c.facts["mid"]] and regs(2)[0] < c.facts["mid"] < regs(2)[-1]
    if len(regs(4)) >= 3:                                               # the middle regions of row 4 hold nothing at all
        assert in_row(4).tolist() == [regs(4)[0], regs(4)[-1]] and (per_region[regs(4)[1:-1]] == 0).all()
        inner = [k for k in regs(4)[1:-1] if (k << 16) >= 4 * n_refs and ((k + 1) << 16) <= 5 * n_refs]
        assert n_refs < 3 * R or inner
    n = np.diff(CC.choose_model(c.cells, c.n_reads, n_refs, 85, 0.02)[2].astype(np.int64))
    assert (n > 0).tolist() == [True, True, True, False, True, False, True, False, True, False, False, True]
    if n_refs > R:                                                      # row 6 passes by a cell of its last region alone; its first region lists its 1s
        assert in_row(6).tolist() == [regs(6)[0], regs(6)[-1]]
        t6 = lin[lin // n_refs == 6]
        assert (CC.table_of(c.cells, c.n_reads, n_refs)[1][np.isin(lin, t6[t6 >> 16 == regs(6)[0]])] == 1).all()
    # a region none of whose rows passes between regions that have one
    r0, _, nseg, _ = CC.region_rows(c.n_reads, n_refs)
    has = np.array([n[int(a):int(a + s)].any() for a, s in zip(r0, nseg)])
    assert any(not has[k] and has[:k].any() and has[k + 1:].any() for k in range(len(has)))
    assert c.levels == "1,2" and set(c.tests) == {(85, 0.02), (85, 0.0), (85, -1.0)}


def test_many_regions_a_wave_per_segment():
    c = _case("many_regions_segs")
    nseg = CC.region_rows(c.n_reads, c.n_refs)[2]
    assert len(nseg) == 2106 and set(nseg[:-1].tolist()) == {656, 657} and set(_looks(c)) == {"segs"}
    first, wrap, big, _ = CC.region_facts(c.cells, c.n_reads, c.n_refs)
    filled, kind = first + big > 0, c.facts["kind"]
    # whatever the grid up to 1050: an empty region, and one with few cells, right behind one that holds thousands (its LDS copy is not left zero)
    for grid in list(range(8, 1051, 8)) + [1, 7, 255, 511, 513, 1049]:
        a, b = slice(0, 2106 - grid), slice(grid, 2106)
        assert ((kind[a] == 4) & ~filled[b]).any() and ((kind[a] == 4) & (kind[b] == 1)).any() and (filled[a] & ~filled[b]).sum() > 100


def test_many_regions():
    c = _case("many_regions")
    nreg = len(CC.region_rows(c.n_reads, c.n_refs)[0])
    assert nreg == 2106 > 2 * 1050 and CC.sim_bytes(c.n_reads, c.n_refs) == 138_000_000
    first, wrap, big, risky = CC.region_facts(c.cells, c.n_reads, c.n_refs)
    lk = np.array([x or "?" for x in _looks(c)])
    kind = c.facts["kind"]
    assert (first[kind == 4] == CC.NWV * CC.QW + 1).all() and 80 < (kind == 4).sum() < 200
    assert wrap[kind == 2].all() and big[kind == 3].all() and (lk[kind >= 2] == "rows").all() and (lk[kind <= 1] == "walk").all()
    assert min((kind == q).sum() for q in range(4)) > 400
    empty = first + big == 0
    assert empty.sum() > 400 and not empty[c.facts["always"]].any() and c.facts["always"] == [0, 511, 512, 513, 1023, 1024, 2105]
    # whatever the grid up to 1050, some workgroup takes: a region for the walk behind one looked at piece by piece, the reverse, two looked at
    # piece by piece, a region without a queue overflow behind one with, an empty region behind one with a wrap
    for grid in list(range(8, 1051, 8)) + [1, 7, 255, 511, 513, 1049]:
        a, b = slice(0, nreg - grid), slice(grid, nreg)
        assert ((lk[a] == "rows") & (lk[b] == "walk")).any() and ((lk[a] == "walk") & (lk[b] == "rows")).any() and ((lk[a] == "rows") & (lk[b] == "rows")).any()
        assert ((kind[a] == 4) & (kind[b] != 4)).any() and (wrap[a] & empty[b]).any() and ((kind[a] == 4) & (kind[b] == 1)).any()


def test_table_end():
    c = _case("table_end")
    tb = c.n_reads * c.n_refs
    assert tb % R and tb % 16 and tb - 1 in CC.table_of(c.cells, c.n_reads, c.n_refs)[0]


def test_fuzz_free_shapes():
    n = [len(CC.region_rows(CC.fuzz_free(i).n_reads, CC.fuzz_free(i).n_refs)[0]) for i in range(CC.FUZZ_FREE)]
    assert CC.FUZZ_FREE == 20 and min(n) >= 2 and max(n) <= 41 and len({CC.fuzz_free(i).levels for i in range(20)}) == 3
    assert all(CC.fuzz_free(i).cells.long.any() for i in range(20))
