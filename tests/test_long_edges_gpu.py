"""k_score_big (lime_kernels.hip) -- the scorer of clusters beyond the in-scan limit, with arithmetic and a hash table of its own -- at its
edges, on the collections of tests/long_cases.py (checked without a GPU in tests/test_long_cases_cpu.py), along the three routes its updates
leave by: added to the table (after the compare-and-swap scan, after k_apply / k_apply_tiles, after k_score_list), as 8-byte records for the
owner-partitioned exchange (k_apply_bigrecs), and as records bucketed by region for clusterChoose without the table (k_bigrec_count /
k_bigrec_scatter, k_apply_tiles<., 1> and <., 2>) -- with the list of those records regrown by lime_get_stats where it overflows.
Every comparison is np.array_equal / torch.equal against the oracle's table: no tolerance anywhere."""
import functools

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import long_cases as LC
from tests.test_gpu_choose_free import _expected, _run
from tests.test_gpu_records import _exchange_on_one_gpu

pytestmark = pytest.mark.gpu

WIDE = (1800, 180)                                # count_edges on a table of five regions: 18 + 18 names, 100 rows / 10 columns apart
GENERATORS = {
    "count_edges": lambda: LC.count_edges(True, *WIDE),
    "count_edges_one_symbol": lambda: LC.count_edges(False, *WIDE),
    "hash_chains_reads": lambda: LC.hash_chains("reads"),
    "hash_chains_genomes": lambda: LC.hash_chains("genomes"),
    "full_load": LC.full_load,
    "record_list_overflow": LC.record_list_overflow,
    "lonely_region": LC.lonely_region,
    "small_max_border": LC.small_max_border,
}
ALL_FIVE = ["count_edges", "count_edges_one_symbol", "hash_chains_reads", "hash_chains_genomes", "full_load", "record_list_overflow", "lonely_region"]
FOUR = ["count_edges", "hash_chains_reads", "hash_chains_genomes", "lonely_region", "record_list_overflow"]     # routes 2 and 3: not full_load (34.8 million records)


@functools.lru_cache(maxsize=None)
def _case(name):
    """the collection and the oracle's answers, computed once (nothing here writes to them): (lcp, da, eb, nr, ng, facts, clusters, n_clusters, max_len)"""
    lcp, da, eb, nr, ng, facts = GENERATORS[name]()
    cl, nc, ml = O.detect(lcp, da, nr, LC.ALPHA)
    assert np.array_equal(cl, facts["clusters"])
    return lcp, da, eb, nr, ng, facts, cl, nc, ml


@functools.lru_cache(maxsize=None)
def _table(name, ebwt_on):
    lcp, da, eb, nr, ng, _, cl, _, _ = _case(name)
    sim = O.score(da, eb if ebwt_on else None, cl, nr, ng, threads=8)
    sim.setflags(write=False)
    return sim


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} cells differ, first (read, genome) {bad[:4].tolist()}: got {[int(got[tuple(b)]) for b in bad[:4]]}, want {[int(want[tuple(b)]) for b in bad[:4]]}"


def _layout(lime_amd, nr, ng):
    c = lime_amd.Context()
    try:
        return c.records_layout(nr, ng)
    finally:
        c.close()


def _same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), _first_difference(got, want)


# ---- route 1: added to the table ---------------------------------------------------------------------------------------------------------
PATHS = {"cas": {"LIME_UPDATE_PATH": "cas"}, "bin": {"LIME_UPDATE_PATH": "bin"}, "bin_second_level": {"LIME_UPDATE_PATH": "bin", "LIME_BIN_LEVELS": "1,2"}}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", ALL_FIVE)
def test_fused_pass_adds_the_long_clusters_to_the_table(monkeypatch, name, path):
    import lime_amd
    lcp, da, eb, nr, ng, _, cl, nc, ml = _case(name)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    c = lime_amd.Context()
    try:
        for ebwt_on in (True, False):
            sim, gnc, gml = c.fused(lcp, da, eb if ebwt_on else None, nr, ng, LC.ALPHA)
            assert (gnc, gml) == (nc, ml)
            _same(sim, _table(name, ebwt_on))
    finally:
        c.close()


@pytest.mark.parametrize("path", ["cas", "bin"])
@pytest.mark.parametrize("name", ALL_FIVE + ["small_max_border"])
def test_list_flow_with_the_clusters_shuffled(monkeypatch, name, path):
    """lime_score (host arrays) and lime_score_dev (device arrays) on the oracle's cluster list in random order: k_score_list keeps clusters of up to
    SMALL_MAX = 16 symbols and hands every longer one to k_score_big -- the border the clusters of 15 .. 18 symbols sit on"""
    import torch
    import lime_amd
    lcp, da, eb, nr, ng, _, cl, _, _ = _case(name)
    shuffled = np.ascontiguousarray(cl[np.random.default_rng(5).permutation(len(cl))])
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    dev = torch.device("cuda", 0)
    c = lime_amd.Context()
    try:
        td = torch.from_numpy(da.view(np.int32).copy()).to(dev)
        tc = torch.from_numpy(shuffled.view(np.int64)).to(dev)
        for ebwt_on in (True, False):
            want = _table(name, ebwt_on)
            _same(c.score(da, eb if ebwt_on else None, shuffled, nr, ng), want)
            te = torch.from_numpy(eb.copy()).to(dev) if ebwt_on else None
            sim_t = torch.full((lime_amd.sim_bytes(nr, ng),), 0xAB, dtype=torch.uint8, device=dev)      # zero_sim: the library clears it
            c.score_dev(td, te, len(da), tc.data_ptr(), len(shuffled), nr, ng, sim_t, True)
            s, rc = c.stats()
            assert rc == 0
            torch.cuda.synchronize()
            _same(sim_t[:nr * ng].cpu().numpy().reshape(nr, ng), want)
    finally:
        c.close()


# ---- route 2: records for the owner of the cell --------------------------------------------------------------------------------------------
class _KeptContext:
    """a Context that outlives _exchange_on_one_gpu's close()"""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, k):
        return getattr(self._ctx, k)

    def close(self):
        pass


class _KeptContexts:
    """stands in for the lime_amd module in _exchange_on_one_gpu: Context() hands out the same `world` contexts again and again"""

    def __init__(self, lime_amd, world):
        self._lib, self.sim_bytes = lime_amd._lib, lime_amd.sim_bytes
        self.ctxs, self.k = [lime_amd.Context() for _ in range(world)], 0

    def Context(self):
        self.k += 1
        return _KeptContext(self.ctxs[(self.k - 1) % len(self.ctxs)])

    def close(self):
        for c in self.ctxs:
            c.close()


def _spy_on_records_get(monkeypatch, lime_amd):
    """what lime_records_get reported, per call: (n_bigrecs, records in bins)"""
    seen = []
    orig = lime_amd.Context.records_get

    def records_get(self, *a, **k):
        R, base = orig(self, *a, **k)
        seen.append((int(R.n_bigrecs), int(base[-1])))
        return R, base
    monkeypatch.setattr(lime_amd.Context, "records_get", records_get)
    return seen


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", [n for n in FOUR if n != "record_list_overflow"])
def test_owner_blocks_from_long_cluster_records(monkeypatch, name, world):
    import torch
    import lime_amd
    from lime_amd.dist import combine_edges
    lcp, da, eb, nr, ng, facts, cl, nc, ml = _case(name)
    seen = _spy_on_records_get(monkeypatch, lime_amd)
    for ebwt_on in (True, False):
        del seen[:]
        got, tot_c, tot_m, edges = _exchange_on_one_gpu(lime_amd, torch, lcp, da, eb if ebwt_on else None, len(lcp), nr, ng, LC.ALPHA, world, None, monkeypatch)
        combine_edges(edges)
        assert (tot_c, tot_m) == (nc, ml) and sum(b for b, _ in seen) > 0
        _same(got, _table(name, ebwt_on))
        if name == "lonely_region":                # the last owner's block holds the last region, which no record in a bin belongs to
            assert _layout(lime_amd, nr, ng) == (5, 16)


@pytest.mark.parametrize("world", [2, 3])
def test_list_of_long_cluster_records_is_regrown_and_the_contexts_stay_usable(monkeypatch, world):
    """17 640 000 records of one cluster against a list of 16 * 2^20: the pass sets LIME_FLAG_OVERFLOW, lime_get_stats regrows the list to the count
    and repeats the pass; lime_records_get then reports every record.  The cluster's start is in the first shard (which so makes all of them), its
    rows are all the table's rows: every owner's cell_lo (world 2: byte 135 * 65536 = row 2106, column 2160) falls inside them.  Then an ordinary
    pass on the same contexts."""
    import torch
    import lime_amd
    from lime_amd.dist import combine_edges
    lcp, da, eb, nr, ng, facts, cl, nc, ml = _case("record_list_overflow")
    n_bins, bin_shift = _layout(lime_amd, nr, ng)
    per = (n_bins + world - 1) // world
    assert ((per << bin_shift) % ng) != 0 and 0 < (per << bin_shift) // ng < nr                # the second owner starts in the middle of a row
    seen = _spy_on_records_get(monkeypatch, lime_amd)
    kept = _KeptContexts(lime_amd, world)
    try:
        for ebwt_on in (True, False):
            del seen[:]
            got, tot_c, tot_m, edges = _exchange_on_one_gpu(kept, torch, lcp, da, eb if ebwt_on else None, len(lcp), nr, ng, LC.ALPHA, world)      # (asserts rc == 0 of every stats())
            combine_edges(edges)
            assert (tot_c, tot_m) == (nc, ml)
            assert [b for b, _ in seen] == [17_640_000] + [0] * (world - 1) and 17_640_000 > LC.BIGREC_CAP
            assert sum(r for _, r in seen) == facts["short_updates"]
            _same(got, _table("record_list_overflow", ebwt_on))
        assert kept.k == 2 * world
        # the same contexts, an ordinary collection of another shape
        lcp2, da2, eb2, nr2, ng2, _, _, nc2, ml2 = _case("count_edges")
        got, tot_c, tot_m, edges = _exchange_on_one_gpu(kept, torch, lcp2, da2, eb2, len(lcp2), nr2, ng2, LC.ALPHA, world)
        combine_edges(edges)
        assert (tot_c, tot_m) == (nc2, ml2) and kept.k == 3 * world
        _same(got, _table("count_edges", True))
    finally:
        kept.close()


# ---- route 3: clusterChoose without the table ------------------------------------------------------------------------------------------------
# a beta that lets a part of the rows with a non-zero cell pass (norm 85); record_list_overflow's rows all have the maximum 1: none passes
PART_BETA = {"count_edges": 0.5, "hash_chains_reads": 0.1, "hash_chains_genomes": 0.19, "lonely_region": 0.015, "record_list_overflow": 0.5}


@pytest.mark.parametrize("wide", ["0", "1"])
@pytest.mark.parametrize("name", FOUR)
def test_choose_without_the_table_from_long_cluster_records(monkeypatch, name, wide):
    lcp, da, eb, nr, ng, facts, cl, nc, ml = _case(name)
    env = {"LIME_UPDATE_PATH": "bin", "LIME_CHOOSE_FREE": 1, "LIME_APPLY_WIDE": wide, "LIME_BIN_LEVELS": "1,2"}
    for ebwt_on in (True, False):
        sim = _table(name, ebwt_on)
        for beta in (0.0, PART_BETA[name]):
            emx, eoff, epairs = _expected(sim, 85, beta)
            rows_in = int((np.diff(eoff.astype(np.int64)) > 0).sum())
            if beta and name != "record_list_overflow":
                assert 0 < rows_in < int((emx > 0).sum())
            mx, off, pairs, s = _run(monkeypatch, lcp, da, eb if ebwt_on else None, nr, ng, 85, beta, **env)
            assert (s.n_clusters, s.max_len) == (nc, ml) and s.table_free == 1
            assert np.array_equal(mx, emx), int((mx != emx).sum())
            assert np.array_equal(off, eoff)
            assert np.array_equal(pairs, epairs), (len(pairs), len(epairs))
            if name == "count_edges" and ebwt_on and beta == 0.0:
                # the cells whose only update is t = 256: not in their rows' lists, and the rows list exactly their non-zero cells
                for r, g in facts["t256_cells"]:
                    row, col = facts["read_of"](r), facts["genome_of"](g)
                    mine = pairs[int(off[row]):int(off[row + 1])]
                    assert len(mine) == int(np.count_nonzero(sim[row])) > 0 and col not in mine[:, 0].tolist()


# ---- a side stream -----------------------------------------------------------------------------------------------------------------------
def test_full_load_on_a_side_stream():
    """Best effort, as in tests/test_index_edges_gpu.py: a pass that ignored `stream` shows only while the write of its input is still pending
    on that stream when it is called."""
    import torch
    import lime_amd
    lcp, da, eb, nr, ng, _, cl, nc, ml = _case("full_load")
    dev = torch.device("cuda", 0)
    n = len(lcp)
    tl = torch.from_numpy(lcp.view(np.int32).copy()).to(dev); td = torch.from_numpy(da.view(np.int32).copy()).to(dev); te = torch.from_numpy(eb.copy()).to(dev)
    nbytes = lime_amd.sim_bytes(nr, ng)
    c = lime_amd.Context()
    try:
        A = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)
        c.fused_dev(tl, td, te, n, n, True, nr, ng, LC.ALPHA, A, True)
        s0, rc = c.stats()
        assert rc == 0 and (s0.n_clusters, s0.max_len) == (nc, ml)
        torch.cuda.synchronize()
        _same(A[:nr * ng].cpu().numpy().reshape(nr, ng), _table("full_load", True))
        side = torch.cuda.Stream()
        assert side.cuda_stream != 0
        td_s = torch.zeros_like(td)                                              # not the documents yet
        B = torch.full((nbytes,), 0xCD, dtype=torch.uint8, device=dev)
        filler = torch.rand(16_000_000, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(6):
                filler = torch.sort(filler.flip(0))[0]                           # work in front of the write, so that it is still pending at the call
            td_s.copy_(td.flip(0).flip(0))
            c.fused_dev(tl, td_s, te, n, n, True, nr, ng, LC.ALPHA, B, True, stream=side.cuda_stream)
            s1, rc = c.stats(stream=side.cuda_stream)
        side.synchronize()
        assert rc == 0 and (s1.n_clusters, s1.max_len, s1.n_updates) == (nc, ml, s0.n_updates)
        assert torch.equal(A[:nr * ng], B[:nr * ng])
    finally:
        c.close()
