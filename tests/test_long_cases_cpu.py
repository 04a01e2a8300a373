"""The collections of tests/long_cases.py have what tests/test_long_edges_gpu.py relies on, shown before anything is asked of the GPU: the
occurrence counts recounted with np.unique, k_score_big's hash recomputed and its linear probe simulated, the pair counts, and the oracle's
detection and table on each.  No GPU here."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests import long_cases as LC

SYM = {s: O.sym_index(s) for s in range(256)}


def _detected(lcp, da, n_reads, facts):
    cl, nc, ml = O.detect(lcp, da, n_reads, LC.ALPHA)
    assert np.array_equal(cl, facts["clusters"]) and nc == len(cl) and ml == int(facts["clusters"][:, 1].max())
    return cl


def _counts(da, eb, start, length):
    """{doc: {symbol index: count}} of one cluster, recounted"""
    out = {}
    keys, cnt = np.unique(np.stack([da[start:start + length].astype(np.int64), np.vectorize(SYM.get)(eb[start:start + length])]), axis=1, return_counts=True)
    for (d, s), c in zip(keys.T, cnt):
        out.setdefault(int(d), {})[int(s)] = int(c)
    return out


@pytest.mark.parametrize("ebwt_on", [False, True])
@pytest.mark.parametrize("shape", [(18, 18), (1800, 180)])
def test_count_edges_reaches_the_counts_it_states(ebwt_on, shape):
    lcp, da, eb, nr, ng, f = LC.count_edges(ebwt_on, *shape)
    assert (nr, ng) == shape and (15000 <= len(lcp) <= 20000 if ebwt_on else len(lcp) < 15000)
    cl = _detected(lcp, da, nr, f)
    long_ones = [(int(s), int(L)) for s, L in cl if L > 100]
    assert len(long_ones) == len(f["edge_specs"]) == (8 if ebwt_on else 3)
    read_totals, genome_totals, read_syms, genome_syms = set(), set(), set(), set()
    for (s, L), spec in zip(long_ones, f["edge_specs"]):
        got = _counts(da, eb, s, L)
        assert got == {d: {SYM[ord(k)]: c for k, c in syms.items()} for d, syms in spec.items()}
        reads = [d for d in got if d < nr]; genomes = [d for d in got if d >= nr]
        assert 2 <= len(reads) <= 4 and 2 <= len(genomes) <= 4
        for d, syms in got.items():
            (read_totals if d < nr else genome_totals).add(sum(syms.values()))
            (read_syms if d < nr else genome_syms).update(syms.values())
    assert {254, 255, 256, 257, 511, 512, 513} <= read_totals and {254, 255, 256, 300} <= genome_totals
    if ebwt_on:
        assert {254, 255, 256, 257, 511, 512, 513} <= read_syms and {254, 255, 256, 300} <= genome_syms
        assert {ord("R"), ord("Y"), ord("N")} <= set(eb.tolist())
    else:
        assert set(eb.tolist()) == {LC.A}
    # the list flow's border: clusters of 15, 16, 17 and 18 symbols, several of each
    lens = cl[:, 1].astype(np.int64)
    assert all(int((lens == L).sum()) >= 3 for L in (15, 16, 17, 18))
    assert int(lens[lens <= 100].max()) == 18
    # the filler keeps away from the documents whose cells are written down by hand
    hand_reads = {f["read_of"](r) for r, _ in f["by_hand"]}; hand_genomes = {nr + f["genome_of"](g) for _, g in f["by_hand"]}
    for s, L in cl[lens <= 100].astype(np.int64):
        assert not (set(da[s:s + L].tolist()) & (hand_reads | hand_genomes))


@pytest.mark.parametrize("ebwt_on", [False, True])
@pytest.mark.parametrize("shape", [(18, 18), (1800, 180)])
def test_count_edges_table_is_the_one_written_out_by_hand(ebwt_on, shape):
    lcp, da, eb, nr, ng, f = LC.count_edges(ebwt_on, *shape)
    cl = f["clusters"]
    sim0, sim1 = O.score(da, None, cl, nr, ng), O.score(da, eb, cl, nr, ng)
    assert len(f["by_hand"]) == (30 if ebwt_on else 16)
    for (r, g), (e0, e1) in f["by_hand"].items():
        assert int(sim0[f["read_of"](r), f["genome_of"](g)]) == e0, (r, g, "EBWT=0")
        assert int(sim1[f["read_of"](r), f["genome_of"](g)]) == e1, (r, g, "EBWT=1")
    # a read with 256 occurrences scores 0 against every genome of its cluster in the EBWT=0 build: read 2 meets genome 2 in that cluster only
    assert f["by_hand"][(2, 2)][0] == 0 and sim0[f["read_of"](2), f["genome_of"](2)] == 0
    for r, g in f["t256_cells"]:
        assert sim1[f["read_of"](r), f["genome_of"](g)] == 0
        assert sim1[f["read_of"](r)].any()                       # ... in a row that has other cells: the row is listed, the cell is not
    # every other cell: per-cluster counts, wrapped and saturated, through the pair arithmetic the goldens pin
    assert np.array_equal(sim0, LC.model_table(da, eb, cl, nr, ng, False))
    assert np.array_equal(sim1, LC.model_table(da, eb, cl, nr, ng, True, O))


def test_ht_hash_is_the_kernels():
    # (doc * 2654435761 mod 2^32) >> 15 by hand: 1 -> 0x9E3779B1 >> 15; 2 -> 0x3C6EF362 >> 15; 2^31 + 1 wraps
    assert [int(x) for x in LC.ht_hash([0, 1, 2, (1 << 31) + 1, 0xFFFFFFFF])] == [0, 0x9E3779B1 >> 15, 0x3C6EF362 >> 15, 0x1E3779B1 >> 15, (0x100000000 - 0x9E3779B1) >> 15]
    assert LC.HT_SIZE == 131072 and int(LC.ht_hash(np.arange(1 << 21)).max()) == LC.HT_SIZE - 1


@pytest.mark.parametrize("crafted", ["reads", "genomes"])
def test_hash_chains_wrap_past_the_last_slot(crafted):
    lcp, da, eb, nr, ng, f = LC.hash_chains(crafted)
    assert 16_000_000 <= nr * ng <= 16_800_000 and {nr, ng} & {8}
    cl = _detected(lcp, da, nr, f)
    s, L = f["cluster_a"]
    assert (int(cl[0, 0]), int(cl[0, 1])) == (s, L) and 250 <= L <= 420
    docs_a = da[s:s + L]
    is_read = (lambda d: d < nr)
    tail, pushed = f["tail"], f["pushed"]
    assert len(tail) >= 40 and (LC.ht_hash(tail) >= LC.HT_SIZE - 3).all() and len(pushed) == 20 and (LC.ht_hash(pushed) <= 30).all()
    assert set(tail.tolist()) | set(pushed.tolist()) <= set(docs_a.tolist())
    assert all(is_read(int(d)) == (crafted == "reads") for d in np.concatenate([tail, pushed]))
    # whatever the order of arrival: the chain runs from the last three slots over slot 0, and documents with homes in 0 .. 30 are not at home
    for order in (docs_a, docs_a[::-1], np.sort(docs_a)):
        slot_of, wrapped = LC.probe(order)
        assert wrapped
        over = [d for d in tail.tolist() if slot_of[d] < LC.HT_SIZE - 3]
        assert len(over) == len(tail) - 3 and max(slot_of[d] for d in over) >= len(tail) - 4
        assert sum(slot_of[int(d)] != int(LC.ht_hash(d)) for d in pushed) >= 10
        # reads and genomes inside the chain: a document of the other side sits in the run of filled slots around slot 0
        filled = set(slot_of.values())
        end = 0
        while end in filled:
            end += 1
        in_chain = [d for d, h in slot_of.items() if h >= LC.HT_SIZE - 3 or h < end]
        assert {is_read(d) for d in in_chain} == {True, False}
    # the further clusters: more than twice BIG_GRID, 65 .. 90 symbols (beyond the scan's own limit of 64), all from one pool of 200
    rest = cl[1:].astype(np.int64)
    assert len(rest) >= 70 > 2 * LC.BIG_GRID and rest[:, 1].min() >= LC.MID_MAX + 1 and rest[:, 1].max() <= 90
    pool = set(f["pool"].tolist()); assert len(pool) == 200 and (LC.ht_hash(f["pool"]) % (LC.HT_SIZE - 3) <= 12).all()
    seen = []
    for s, L in rest:
        d = da[s:s + L]
        side = d[(d < nr) == (crafted == "reads")]
        assert set(side.tolist()) <= pool
        assert LC.probe(d)[0] != {}                                        # (terminates)
        seen.append(tuple(side.tolist()))
    assert len(set(seen)) == len(seen)                                     # each in an order of its own
    # consecutive clusters of one workgroup (c, c + BIG_GRID) share colliding documents: a key left behind would be met
    big = cl.astype(np.int64)
    shared = [len(set(da[big[c, 0]:big[c, 0] + big[c, 1]].tolist()) & set(da[big[c + LC.BIG_GRID, 0]:big[c + LC.BIG_GRID, 0] + big[c + LC.BIG_GRID, 1]].tolist()))
              for c in range(len(big) - LC.BIG_GRID)]
    assert min(shared) >= 3


def test_full_load_fills_half_the_table():
    lcp, da, eb, nr, ng, f = LC.full_load()
    cl = _detected(lcp, da, nr, f)
    assert len(cl) == 1 and int(cl[0, 1]) == LC.MAX_CLUSTER == LC.HT_SIZE // 2
    s = int(cl[0, 0])
    d = da[s:s + LC.MAX_CLUSTER]
    docs, cnt = np.unique(d, return_counts=True)
    assert len(docs) == 65536 and (cnt == 1).all() and int((docs < nr).sum()) == 65000 and int((docs >= nr).sum()) == 536 == ng
    assert f["pairs"] == 34_840_000 == nr * ng and nr * ng <= 40_000_000
    assert len(set(eb[s:s + LC.MAX_CLUSTER].tolist())) == 1
    assert np.array_equal(O.score(da, eb, cl, nr, ng, threads=4), np.ones((nr, ng), np.uint8))


def test_record_list_overflow_makes_more_records_than_the_list_holds():
    lcp, da, eb, nr, ng, f = LC.record_list_overflow()
    cl = _detected(lcp, da, nr, f)
    s, L = f["long_cluster"]
    assert L == 8400 and [int(x) for x in cl[cl[:, 1] > 16].ravel()] == [s, L]
    docs, cnt = np.unique(da[s:s + L], return_counts=True)
    assert (cnt == 1).all() and int((docs < nr).sum()) == 4200 == int((docs >= nr).sum())
    assert f["pairs"] == 17_640_000 > LC.BIGREC_CAP == 16 * 2 ** 20
    short = cl[cl[:, 1] <= 16].astype(np.int64)
    assert 1500 <= int(short[short[:, 0] < s, 1].sum()) <= 2500 and 1000 <= int(short[short[:, 0] > s, 1].sum()) <= 2500
    assert set(eb.tolist()) == {LC.A}
    # the short clusters' updates: 256 to a cell, nothing modulo 256 -- but updates all the same (what the repeated pass makes again)
    without = O.score(da, None, short, nr, ng)
    assert not without.any()
    assert f["short_updates"] == sum(int((np.unique(da[a:a + b]) < nr).sum()) * int((np.unique(da[a:a + b]) >= nr).sum()) for a, b in short)
    for e in (eb, None):
        assert np.array_equal(O.score(da, e, cl, nr, ng, threads=4), np.ones((nr, ng), np.uint8))


def test_lonely_region_gets_long_cluster_records_only():
    lcp, da, eb, nr, ng, f = LC.lonely_region()
    cl = _detected(lcp, da, nr, f).astype(np.int64)
    R = f["region_bytes"]
    n_regions = (nr * ng + R - 1) // R
    assert n_regions == 5
    s, L = f["long_cluster"]
    assert L == 100 and [tuple(x) for x in cl[cl[:, 1] > LC.SMALL_MAX]] == [(s, L)]
    for a, b in cl:
        reads = da[a:a + b][da[a:a + b] < nr].astype(np.int64)
        if (a, b) == (s, L):
            assert (reads * ng >= (n_regions - 1) * R).all()                 # every cell of its rows lies in the last region
        else:
            assert ((reads + 1) * ng <= R).all()                             # ... of the short clusters' rows in the first
    for e in (eb, None):
        sim = O.score(da, e, cl, nr, ng).ravel()
        per_region = [int(np.count_nonzero(sim[k * R:(k + 1) * R])) for k in range(n_regions)]
        assert per_region[0] > 0 and per_region[-1] > 0 and per_region[1:-1] == [0, 0, 0]


def test_small_max_border_lengths():
    lcp, da, eb, nr, ng, f = LC.small_max_border()
    cl = _detected(lcp, da, nr, f)
    assert sorted(np.unique(cl[:, 1], return_counts=True)[1].tolist()) == [40, 40, 40, 40] and set(cl[:, 1].tolist()) == {15, 16, 17, 18}
    assert np.array_equal(O.score(da, eb, cl, nr, ng), LC.model_table(da, eb, cl, nr, ng, True, O))
    assert np.array_equal(O.score(da, None, cl, nr, ng), LC.model_table(da, eb, cl, nr, ng, False))
