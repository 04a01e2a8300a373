"""clusterChoose on the device along both routes, on the chosen tables of tests/choose_cases.py (checked without a GPU in tests/test_choose_cases_cpu.py).
With the table: k_choose + k_gather_pairs through lime_choose_dev, lime_choose_pairs_dev and lime_choose_lists_dev + lime_lists_get.  Without it:
k_region_rows, k_bigrec_count / k_bigrec_scatter and k_apply_tiles<WIDE, 1> then <WIDE, 2> through lime_fused_choose_dev, on the collections
arrays_of() makes, against the model and against the same call with the table (choose_free 0).  Everything is compared exactly: row maxima,
non-zero counts, offsets and (idRef, sim) lists."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import choose_cases as CC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=4)
def _case(name):
    return CC.make(name)


@functools.lru_cache(maxsize=16)
def _model(name, norm, beta):
    """the model of a case for one test, computed once (nothing writes to it)"""
    c = _case(name)
    m = CC.choose_model(c.cells, c.n_reads, c.n_refs, norm, beta)
    for a in m:
        a.setflags(write=False)
    return m


def _same(what, got, want):
    assert got.shape == want.shape, f"{what}: {got.shape} for {want.shape}"
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
        raise AssertionError(f"{what}: {len(bad)} of {len(want)} differ, first at {bad[:8].tolist()}: got {got[bad[:4]].tolist()}, want {want[bad[:4]].tolist()}")


# ---- with the table ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import lime_amd
    c = lime_amd.Context()
    yield c
    c.close()


def _upload(torch, c):
    """the table in a lime_sim_bytes() block; what lies between n_reads * n_refs and the block's end is 0xFF"""
    import lime_amd
    dev = torch.device("cuda", 0)
    n, sb = c.n_reads * c.n_refs, lime_amd.sim_bytes(c.n_reads, c.n_refs)
    assert sb == CC.sim_bytes(c.n_reads, c.n_refs)
    if n > 1 << 30:                                                       # sparse: the cells are set on the device
        buf = torch.zeros(sb, dtype=torch.uint8, device=dev)
        lin, val = CC.table_of(c.cells, c.n_reads, c.n_refs)
        buf[torch.from_numpy(lin).to(dev)] = torch.from_numpy(val.astype(np.uint8)).to(dev)
        buf[n:] = 0xFF
        return buf
    buf = torch.full((max(sb, 16),), 0xFF, dtype=torch.uint8, device=dev)
    if n:
        buf[:n] = torch.from_numpy(CC.dense_of(c.cells, c.n_reads, c.n_refs).reshape(-1)).to(dev)
    return buf


def _check_table(torch, ctx, name, buf, stream=None):
    """the three entry points on one uploaded table, for every (norm, beta) of the case"""
    c = _case(name)
    nr, dev = c.n_reads, buf.device
    for k, (norm, beta) in enumerate(c.tests):
        mx, nnz, off, pairs = _model(name, norm, beta)
        what = f"{name} norm {norm} beta {beta}"
        if k == 0:                                                        # (the row scan knows no beta)
            mt = torch.full((nr + 1,), 0xAB, dtype=torch.uint8, device=dev)
            zt = torch.full((nr + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            if stream is not None:
                torch.cuda.synchronize()
            ctx.choose_dev(buf, nr, c.n_refs, mt, zt, stream=stream)
            torch.cuda.synchronize()
            _same(what + ": lime_choose_dev maxima", mt[:nr].cpu().numpy(), mx)
            _same(what + ": lime_choose_dev counts", zt[:nr].cpu().numpy().view(np.uint32), nnz)
            assert int(mt[nr]) == 0xAB and int(zt[nr]) == 0x5A5A5A5A, what + ": written behind the rows"
        gmx, goff, gpairs = ctx.choose_pairs_dev(buf, nr, c.n_refs, norm, beta, stream=stream)
        _same(what + ": lime_choose_pairs_dev maxima", gmx, mx)
        _same(what + ": lime_choose_pairs_dev offsets", goff, off)
        _same(what + ": lime_choose_pairs_dev pairs", gpairs, pairs)
        li = ctx.choose_lists_dev(buf, nr, c.n_refs, norm, beta, stream=stream)
        try:
            assert li.info()[:3] == (nr, len(pairs), norm) and np.float32(li.info()[3]) == np.float32(beta)
            lmx, loff, lpairs = li.get()
            _same(what + ": lime_lists_get maxima", lmx, mx)
            _same(what + ": lime_lists_get offsets", loff, off)
            _same(what + ": lime_lists_get pairs", lpairs, pairs)
        finally:
            li.close()


@pytest.mark.parametrize("name", [n for n in CC.TABLE_CASES if n != "beyond_4g"])
def test_table_route_equals_the_model(ctx, name):
    import torch
    _check_table(torch, ctx, name, _upload(torch, _case(name)))


def test_table_route_beyond_4g(ctx):
    """rows on both sides of byte 2^32 of a 4.59 GB table: r * n_refs in 64 bits in both kernels"""
    import torch
    free, _ = torch.cuda.mem_get_info(0)
    if free < 6 << 30:
        pytest.skip(f"{free >> 20} MB of device memory free, the table and its copies need 6 GB")
    buf = _upload(torch, _case("beyond_4g"))
    try:
        _check_table(torch, ctx, "beyond_4g", buf)
    finally:
        del buf
        torch.cuda.empty_cache()


def test_table_route_fuzz(ctx):
    """200 small seeded tables of the named widths"""
    import torch
    for i in range(CC.FUZZ_TABLES):
        c = CC.fuzz_table(i)
        buf = _upload(torch, c)
        for norm, beta in c.tests:
            mx, nnz, off, pairs = CC.choose_model(c.cells, c.n_reads, c.n_refs, norm, beta)
            gmx, goff, gpairs = ctx.choose_pairs_dev(buf, c.n_reads, c.n_refs, norm, beta)
            what = f"fuzz table {i} ({c.n_reads} x {c.n_refs}) norm {norm} beta {beta}"
            _same(what + ": maxima", gmx, mx); _same(what + ": offsets", goff, off); _same(what + ": pairs", gpairs, pairs)
        mt = torch.full((c.n_reads + 1,), 0xAB, dtype=torch.uint8, device=buf.device)
        zt = torch.full((c.n_reads + 1,), -1, dtype=torch.int32, device=buf.device)
        ctx.choose_dev(buf, c.n_reads, c.n_refs, mt, zt)
        torch.cuda.synchronize()
        _same(f"fuzz table {i}: counts", zt[:c.n_reads].cpu().numpy().view(np.uint32), nnz)
        assert int(mt[c.n_reads]) == 0xAB and int(zt[c.n_reads]) == -1


@pytest.mark.parametrize("name", ["shared_group_17", "sweep_edges_2049", "grid_stride_65539x5"])
def test_table_route_on_a_stream_of_its_own(ctx, name):
    import torch
    buf = _upload(torch, _case(name))
    st = torch.cuda.Stream()
    _check_table(torch, ctx, name, buf, stream=st.cuda_stream)


def test_table_route_scratch_grows_and_shrinks():
    """one context: a small table, one of 65539 rows, a small one again -- ensure_choose's scratch grows once and is then larger than the call needs;
    the first call's lists stay what they were"""
    import torch
    import lime_amd
    c = lime_amd.Context()
    try:
        first = _case("beta_edges")
        buf0 = _upload(torch, first)
        norm, beta = first.tests[1]
        kept = c.choose_lists_dev(buf0, first.n_reads, first.n_refs, norm, beta)
        for name in ("beta_edges", "grid_stride_65539x5", "one_bit", "sweep_edges_1025", "grid_stride_65539x5", "padding_7"):
            _check_table(torch, c, name, _upload(torch, _case(name)))
        mx, _, off, pairs = _model("beta_edges", norm, beta)
        gmx, goff, gpairs = kept.get()
        _same("kept lists: maxima", gmx, mx); _same("kept lists: offsets", goff, off); _same("kept lists: pairs", gpairs, pairs)
    finally:
        c.close()


def test_table_route_host_outputs_dirty_on_entry(ctx):
    """lime_choose_pairs_dev into host arrays full of 0xCD: every element up to n_reads is written, nothing behind; no pair: *pairs NULL"""
    import torch
    from lime_amd.api import _ptr
    name = "beta_edges"
    c = _case(name)
    buf = _upload(torch, c)
    for norm, beta in c.tests:
        mx, _, off, pairs = _model(name, norm, beta)
        hm = np.full(c.n_reads + 3, 0xCD, dtype=np.uint8)
        ho = np.full(c.n_reads + 4, 0xCDCDCDCDCDCDCDCD, dtype=np.uint64)
        pp, npairs = C.c_void_p(0x1234), C.c_uint64(77)
        rc = ctx.lib.lime_choose_pairs_dev(ctx.h, _ptr(buf), c.n_reads, c.n_refs, norm, beta, hm.ctypes.data, ho.ctypes.data, C.byref(pp), C.byref(npairs), None)
        assert rc == 0 and npairs.value == len(pairs)
        got = ctx._pairs_out(pp, npairs) if pp.value else np.zeros((0, 2), np.uint32)
        _same(f"beta {beta}: maxima", hm[:c.n_reads], mx); _same(f"beta {beta}: offsets", ho[:c.n_reads + 1], off); _same(f"beta {beta}: pairs", got, pairs)
        assert (hm[c.n_reads:] == 0xCD).all() and (ho[c.n_reads + 1:] == 0xCDCDCDCDCDCDCDCD).all()
        if not len(pairs):
            assert pp.value is None                                       # (NULL)


def test_table_route_refusals(ctx):
    """a table that is not 16-byte aligned and NULL outputs: LIME_ERR_ARG, nothing launched, the outputs as they were"""
    import torch
    from lime_amd._lib import ERR_ARG, LimeError
    from lime_amd.api import _ptr
    c = _case("one_bit")
    buf = _upload(torch, c)
    big = torch.zeros(len(buf) + 16, dtype=torch.uint8, device=buf.device)
    view = big[4:4 + len(buf)]
    view.copy_(buf)
    assert view.data_ptr() % 16 == 4
    mt = torch.full((c.n_reads,), 0xAB, dtype=torch.uint8, device=buf.device)
    zt = torch.full((c.n_reads,), 7, dtype=torch.int32, device=buf.device)
    calls = [lambda: ctx.choose_dev(view, c.n_reads, c.n_refs, mt, zt), lambda: ctx.choose_pairs_dev(view, c.n_reads, c.n_refs, 85, 0.0),
             lambda: ctx.choose_lists_dev(view, c.n_reads, c.n_refs, 85, 0.0),
             lambda: ctx.choose_dev(buf, c.n_reads, c.n_refs, None, zt), lambda: ctx.choose_dev(buf, c.n_reads, c.n_refs, mt, None),
             lambda: ctx.choose_dev(None, c.n_reads, c.n_refs, mt, zt), lambda: ctx.choose_pairs_dev(None, c.n_reads, c.n_refs, 85, 0.0),
             lambda: ctx.choose_lists_dev(None, c.n_reads, c.n_refs, 85, 0.0)]
    for k, call in enumerate(calls):
        with pytest.raises(LimeError) as e:
            call()
        assert e.value.code == ERR_ARG, k
    hm, ho = np.zeros(c.n_reads + 1, np.uint8), np.zeros(c.n_reads + 2, np.uint64)
    pp, npairs = C.c_void_p(), C.c_uint64(0)
    lib, a = ctx.lib, (_ptr(buf), c.n_reads, c.n_refs, 85, 0.0)
    assert lib.lime_choose_pairs_dev(ctx.h, *a, None, ho.ctypes.data, C.byref(pp), C.byref(npairs), None) == ERR_ARG
    assert lib.lime_choose_pairs_dev(ctx.h, *a, hm.ctypes.data, None, C.byref(pp), C.byref(npairs), None) == ERR_ARG
    assert lib.lime_choose_pairs_dev(ctx.h, *a, hm.ctypes.data, ho.ctypes.data, None, C.byref(npairs), None) == ERR_ARG
    assert lib.lime_choose_pairs_dev(ctx.h, *a, hm.ctypes.data, ho.ctypes.data, C.byref(pp), None, None) == ERR_ARG
    assert lib.lime_choose_lists_dev(ctx.h, *a, None, None) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((mt == 0xAB).all()) and bool((zt == 7).all())
    _check_table(torch, ctx, "one_bit", buf)                              # and the same table, aligned, is taken


# ---- without the table -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _arrays(name, eb, fit=True):
    c = _case(name)
    return CC.arrays_of(c.cells, c.n_reads, c.n_refs, ebwt=eb, seed=c.seed, fit=fit)


def _tensors(torch, name, eb, fit=True):
    """the collection on the device, and how many of its clusters must arrive as 64-bit records (fit: the long ones only)"""
    dev = torch.device("cuda", 0)
    lcp, da, e = _arrays(name, eb, fit)
    c = _case(name)
    return (torch.from_numpy(lcp.view(np.int32)).to(dev), torch.from_numpy(da.view(np.int32)).to(dev), None if e is None else torch.from_numpy(e).to(dev), len(lcp),
            CC.n_big_of(c.cells, c.seed, fit)[0])


def _context(monkeypatch, levels, free, wide="", group=None):
    import lime_amd
    env = {"LIME_UPDATE_PATH": "bin", "LIME_CHOOSE_FREE": free, "LIME_APPLY_WIDE": wide, "LIME_BIN_LEVELS": levels}
    if group is not None:
        env["LIME_APPLY_GROUP"] = group
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return lime_amd.Context()


def _fused(ctx, name, t, norm, beta, calls):
    """one call; `calls`: what the context's count of calls without the table must be behind it"""
    c = _case(name)
    tl, td, te, n, n_big = t
    mx, off, pairs, s = ctx.fused_choose_dev(tl, td, te, n, c.n_reads, c.n_refs, CC.ALPHA, norm, beta)
    assert ctx.host_times()["choose_without_table"] == calls, f"{name}: the call {'built' if calls else 'did not build'} the table"
    assert s.n_clusters == CC.n_clusters_of(c.cells)
    # (which look a region gets hangs on this: a region that a 64-bit record falls into is looked at piece by piece, or a wave per segment)
    assert s.n_big == n_big, f"{name}: {s.n_big} clusters arrived as 64-bit records, {n_big} were built to"
    return mx, off, pairs


def _check_free(torch, monkeypatch, name, wide="", group=None, tests=None, with_table=True, ebwts=(None, CC.BASE), fit=True):
    c = _case(name)
    free = _context(monkeypatch, c.levels, 1, wide, group)
    table = _context(monkeypatch, c.levels, 0, wide, group) if with_table else None
    try:
        calls = 0
        for eb in ebwts:
            t = _tensors(torch, name, eb, fit)
            for norm, beta in (tests or c.tests):
                mx, _, off, pairs = _model(name, norm, beta)
                what = f"{name} ebwt {eb} norm {norm} beta {beta} wide {wide!r} group {group!r}"
                calls += 1
                got = _fused(free, name, t, norm, beta, calls)
                _same(what + ": maxima", got[0], mx); _same(what + ": offsets", got[1], off); _same(what + ": pairs", got[2], pairs)
                if table is not None:
                    ref = _fused(table, name, t, norm, beta, 0)
                    _same(what + ": maxima with the table", got[0], ref[0]); _same(what + ": offsets with the table", got[1], ref[1])
                    _same(what + ": pairs with the table", got[2], ref[2])
    finally:
        free.close()
        if table is not None:
            table.close()


@pytest.mark.parametrize("wide", ["0", "1"])
@pytest.mark.parametrize("name", [n for n in CC.FREE_CASES if not n.startswith("many_regions")])
def test_without_the_table_equals_the_model_and_the_table_route(monkeypatch, name, wide):
    import torch
    _check_free(torch, monkeypatch, name, wide)


@pytest.mark.parametrize("wide", ["0", "1"])
@pytest.mark.parametrize("name", ["many_regions", "many_regions_segs"])
def test_without_the_table_many_regions(monkeypatch, name, wide):
    """2106 regions on at most 1050 workgroups: every workgroup carries its state from a region to its next, of another kind"""
    import torch
    _check_free(torch, monkeypatch, name, wide, with_table=False)


@pytest.mark.parametrize("wide", ["0", "1"])
@pytest.mark.parametrize("name", ["seg_estimate_307_walk", "border_in_piece", "segs_258_259_255"])
def test_without_the_table_clusters_across_the_scan_windows(monkeypatch, name, wide):
    """arrays_of(fit=False): short clusters that do not close inside their scan window's read-ahead arrive as 64-bit records like the long ones, in
    regions that hold no long cluster's cell -- those regions are then looked at piece by piece"""
    import torch
    c = _case(name)
    assert CC.n_big_of(c.cells, c.seed, fit=False)[1] > 3
    _check_free(torch, monkeypatch, name, wide, fit=False)


@pytest.mark.parametrize("group", ["", "1", "2", "3", "4", "5", "6"])
@pytest.mark.parametrize("name", CC.GROUPED)
def test_without_the_table_with_forced_lanes_per_run(monkeypatch, name, group):
    """LIME_APPLY_GROUP: 2^lg lanes share a run (6: a wave per run); process-wide, so back to the library's choice afterwards"""
    import torch
    try:
        _check_free(torch, monkeypatch, name, "0", group, tests=_case(name).tests[:1], with_table=False)
    finally:
        _context(monkeypatch, "1,1", 1, "", "").close()


@pytest.mark.parametrize("name", ["wraps", "big_records", "long_rows_200000"])
def test_without_the_table_lists_left_on_the_device(monkeypatch, name):
    import torch
    c = _case(name)
    ctx = _context(monkeypatch, c.levels, 1)
    try:
        t = _tensors(torch, name, CC.BASE)
        kept = []
        for k, (norm, beta) in enumerate(c.tests):
            li, s = ctx.fused_choose_lists_dev(t[0], t[1], t[2], t[3], c.n_reads, c.n_refs, CC.ALPHA, norm, beta)
            assert ctx.host_times()["choose_without_table"] == k + 1 and s.n_clusters == CC.n_clusters_of(c.cells) and s.n_big == t[4]
            kept.append(li)
        for li, (norm, beta) in zip(kept, c.tests):                      # (all of them alive at once: the later calls left the earlier lists alone)
            mx, _, off, pairs = _model(name, norm, beta)
            assert li.info()[:3] == (c.n_reads, len(pairs), norm)
            gmx, goff, gpairs = li.get()
            _same(f"{name} beta {beta}: maxima", gmx, mx); _same(f"{name} beta {beta}: offsets", goff, off); _same(f"{name} beta {beta}: pairs", gpairs, pairs)
    finally:
        ctx.close()


def test_without_the_table_cases_one_after_the_other_on_one_context(monkeypatch):
    """a dense case, then the long rows (their middle regions' counts lie in scratch the dense case used: released blocks are poisoned under the test
    hooks, so a count nobody wrote shows), then smaller and larger tables again"""
    import torch
    ctx = _context(monkeypatch, "1,2", 1)
    try:
        calls = 0
        for name in ("queue_overflow", "long_rows_200000", "table_end", "long_rows_196613", "border_in_piece", "long_rows_65537", "wraps"):
            c = _case(name)
            t = _tensors(torch, name, None)
            for norm, beta in c.tests:
                calls += 1
                mx, _, off, pairs = _model(name, norm, beta)
                got = _fused(ctx, name, t, norm, beta, calls)
                _same(f"{name} beta {beta}: maxima", got[0], mx); _same(f"{name} beta {beta}: offsets", got[1], off); _same(f"{name} beta {beta}: pairs", got[2], pairs)
    finally:
        ctx.close()
