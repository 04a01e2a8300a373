"""flush_direct of k_scan<., 0, 2> (tables of one or two sub-regions, records written by the scorers): a flush stores the LAST records
waiting in a sub-region's buffer and never moves the rest; the flush at the top of a window takes whole groups of `flush_gran` records
(option flush_gran: 64, or 16 as every flush did before), a flush that makes room for a scorer takes whole lines of 16, the kernel's
last one everything.  So records now wait across windows -- up to 63 per sub-region -- and a room flush may find such a carry in front
of it.  Every case runs with flush_gran 16 and 64 and compares the pass's return code, its counters (n_clusters, max_len, n_updates
against the oracle's count of scoring pairs) and the whole table with the ORACLE's (oracle_py.detect / score), never with another path
of the library.

Inputs: the oracle's generator, and hand-placed clusters (every symbol 'A', so every read x genome pair scores with both builds) on a
background in which every position is a run of its own."""
import numpy as np
import pytest

from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

ALPHA = 16
NR, NG = 3000, 300
WIN = 1024                                      # positions per window of the scan
GRANS = ("16", "64")
QCAP_SHORT = 160                                # the EBWT=1 record kernels' queue (QCAP_SCAN_SHORT)

_CTX, _REF = {}, {}


def _ctx(gran, **opts):
    import lime_amd
    key = (gran,) + tuple(sorted(opts.items()))
    if key not in _CTX:
        c = lime_amd.Context()
        c.set_option("update_path", "bin")
        c.set_option("flush_gran", gran)
        for k, v in opts.items():
            c.set_option(k, str(v))
        _CTX[key] = c
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear(); _REF.clear()


def _blank(n):
    """every position a run of its own (lcp 0), all of genome 0: no cluster"""
    return np.zeros(n, np.uint32), np.full(n, NR, np.uint32), np.full(n, ord("A"), np.uint8)


def _put(lcp, da, eb, p, docs):
    k = len(docs)
    lcp[p] = 0; lcp[p + 1:p + k] = ALPHA + 4
    if p + k < len(lcp):
        lcp[p + k] = 0
    da[p:p + k] = np.array(docs, np.uint64).astype(np.uint32); eb[p:p + k] = ord("A")


_SYM = None


def pair_count(da, eb, cl, nr):
    """the oracle's count of table cells incremented: (cluster, read, genome) with a score > 0.  EBWT=0: every read of a cluster
    with every genome of it (the score is min of the two counts); EBWT=1: the pairs O.pair_score gives more than 0"""
    global _SYM
    if _SYM is None:
        _SYM = [O.sym_index(b) for b in range(256)]
    dl = da.tolist()
    el = eb.tolist() if eb is not None else None
    total, seen = 0, {}
    for p, ln in cl.tolist():
        reads, gens = {}, {}
        for k in range(p, p + ln):
            d = dl[k]
            (reads if d < nr else gens).setdefault(d, []).append(_SYM[el[k]] if el is not None else 0)
        if el is None:
            total += len(reads) * len(gens)
            continue
        for r in reads.values():
            for g in gens.values():
                key = (tuple(sorted(r)), tuple(sorted(g)))
                if key not in seen:
                    cr, cg = np.zeros(16, np.uint8), np.zeros(16, np.uint8)
                    for s in r:
                        cr[s] += 1                                        # (reads wrap, genomes saturate: far from either here)
                    for s in g:
                        cg[s] = min(int(cg[s]) + 1, 255)
                    seen[key] = O.pair_score(cr, cg) > 0
                total += seen[key]
    return total


def _reference(key, make, nr=NR, ng=NG):
    """(arrays, {ebwt: (table, pairs)}, (n_clusters, max_len)) of an input, computed once per module and left unchanged"""
    if key not in _REF:
        arrs = make()
        cl, nc, ml = O.detect(arrs[0], arrs[1], nr, ALPHA)
        exp = {e: (O.score(arrs[1], arrs[2] if e else None, cl, nr, ng, threads=4), pair_count(arrs[1], arrs[2] if e else None, cl, nr)) for e in (1, 0)}
        _REF[key] = (arrs, exp, (nc, ml))
    return _REF[key]


def _run(c, arrs, ebwt, nr=NR, ng=NG):
    import torch
    import lime_amd
    tl = torch.from_numpy(arrs[0].view(np.int32)).cuda(); td = torch.from_numpy(arrs[1].view(np.int32)).cuda()
    te = torch.from_numpy(arrs[2]).cuda() if ebwt else None
    sim = torch.full((lime_amd.sim_bytes(nr, ng),), 0x5A, dtype=torch.uint8, device="cuda")       # every byte must be written
    n = len(arrs[0])
    c.fused_dev(tl, td, te, n, n, True, nr, ng, ALPHA, sim)
    s, rc = c.stats()
    return s, rc, sim[:nr * ng].cpu().numpy().reshape(nr, ng)


def _check(c, ref, ebwt):
    arrs, exp, cnt = ref
    s, rc, got = _run(c, arrs, ebwt)
    table, pairs = exp[ebwt]
    assert rc == 0, (rc, s.flags)
    assert (s.n_clusters, s.max_len) == cnt and s.n_updates == pairs, ((s.n_clusters, s.max_len, s.n_updates), cnt, pairs)
    assert s.wave_records_max > 0 or pairs == 0, "the pass left the record path"
    assert np.array_equal(got, table), int((got != table).sum())


def test_flush_gran_is_16_or_64():
    import lime_amd
    c = lime_amd.Context()
    try:
        for v in ("0", "15", "32", "128"):
            with pytest.raises(lime_amd.LimeError):
                c.set_option("flush_gran", v)
        for v in ("16", "64", ""):
            c.set_option("flush_gran", v)
    finally:
        c.close()


# ---- 1. counts at the edges of a line and of a full batch ------------------------------------------------------------------------
def _edge_input(k, more):
    """window 0 holds exactly k two-symbol read + genome clusters; `more` further windows of five such clusters each"""
    def make():
        lcp, da, eb = _blank(WIN * (1 + more))
        for j in range(k):
            _put(lcp, da, eb, 8 + 4 * j, [(7 * j + 1) % NR, NR + (13 * j + 5) % NG])
        for w in range(1, 1 + more):
            for j in range(5):
                _put(lcp, da, eb, w * WIN + 100 + 6 * j, [(31 * w + j) % NR, NR + (17 * w + 3 * j) % NG])
        return lcp, da, eb
    return make


@pytest.mark.parametrize("ebwt", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("more", [0, 16])
@pytest.mark.parametrize("k", [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129])
def test_counts_at_the_edges(k, more, gran, ebwt):
    """one window alone: the kernel's last flush is the only one; followed by 16 more windows in ONE workgroup: its 16 waves draw 17
    windows, so a wave scores a second window with what its first left waiting"""
    ref = _reference(("edge", k, more), _edge_input(k, more))
    assert ref[2][0] == k + 5 * more and ref[1][1][1] == ref[1][0][1] == k + 5 * more
    _check(_ctx(gran, max_blocks=1), ref, ebwt)


# ---- 2. carry across many windows -------------------------------------------------------------------------------------------------
N_CARRY = 200 * 1024 + 500                      # one workgroup: about 12 windows per wave, the last window short


@pytest.mark.parametrize("ebwt", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("dense_min", [64, 0])
@pytest.mark.parametrize("mode", [0, 1])
def test_carry_across_many_windows(mode, dense_min, gran, ebwt):
    ref = _reference(("carry", mode), lambda: O.synth(4700 + mode, 0, N_CARRY, NR, NG, ALPHA, mode))
    assert ref[1][ebwt][1] > 0
    _check(_ctx(gran, max_blocks=1, dense_min=dense_min), ref, ebwt)


# ---- 3. two sub-regions, the second one fed by a trickle --------------------------------------------------------------------------
@pytest.mark.parametrize("ebwt", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
def test_two_sub_regions_with_a_trickle(gran, ebwt):
    """The 4.4 GB table of test_records_written_by_the_scorers_or_through_the_queue -- the reads in the seven rows around cell 2^32 --
    with only every 50th read beyond the border: sub-region 1 gets a few records a window and fills a batch of 64 only across windows"""
    import torch
    import lime_amd
    n, nr, ng = 3_000_000, 1_100_000, 4000
    lo_r = (1 << 32) // ng - 3                                            # row lo_r + 3 straddles the border, rows lo_r + 4 .. 6 lie beyond it
    sb = lime_amd.sim_bytes(nr, ng)
    free = torch.cuda.mem_get_info()[0]
    if free < sb + (2 << 30):
        pytest.skip(f"{free >> 20} MB of device memory free, the table needs {sb >> 20}")
    if "trickle" not in _REF:
        lcp, da, eb = O.synth(99, 0, n, nr, ng, ALPHA, 1)
        sel = da < nr
        r = da[sel].astype(np.int64)
        da[sel] = (lo_r + np.where(r % 50 == 0, 4 + (r // 50) % 3, r % 4)).astype(np.uint32)
        cl, nc, ml = O.detect(lcp, da, nr, ALPHA)
        d7 = np.where(da < nr, da - lo_r, da - nr + 7).astype(np.uint32)  # the same clusters with the 7 reads renumbered 0..6
        rows = {e: (O.score(d7, eb if e else None, cl, 7, ng, threads=8), pair_count(d7, eb if e else None, cl, 7)) for e in (1, 0)}
        _REF["trickle"] = ((lcp, da, eb), rows, (nc, ml))
    (lcp, da, eb), rows, cnt = _REF["trickle"]
    beyond = int(rows[ebwt][0][4:].astype(np.int64).sum()), int(rows[ebwt][0][:3].astype(np.int64).sum())
    assert 0 < 10 * beyond[0] < beyond[1], beyond                        # a trickle: under a tenth of the records
    c = _ctx(gran, max_blocks=8)
    tl = torch.from_numpy(lcp.view(np.int32)).cuda(); td = torch.from_numpy(da.view(np.int32)).cuda(); te = torch.from_numpy(eb).cuda() if ebwt else None
    sim = torch.full((sb,), 0x5A, dtype=torch.uint8, device="cuda")
    c.fused_dev(tl, td, te, n, n, True, nr, ng, ALPHA, sim)
    s, rc = c.stats()
    assert rc == 0 and (s.n_clusters, s.max_len) == cnt and s.n_updates == rows[ebwt][1] and s.wave_records_max > 0
    got = sim[lo_r * ng:(lo_r + 7) * ng].cpu().numpy().reshape(7, ng)
    assert np.array_equal(got, rows[ebwt][0]), int((got != rows[ebwt][0]).sum())
    assert int(torch.count_nonzero(sim[:lo_r * ng])) == 0 and int(torch.count_nonzero(sim[(lo_r + 7) * ng:nr * ng])) == 0
    del sim


# ---- 4. a flush for room with records carried in front of it ----------------------------------------------------------------------
def _waiting_after_one_window(n4, k2, cap):
    """records a wave holds after scoring ONE of the windows below from an empty buffer, and the pairs of the window's first round of
    3- and 4-symbol clusters.  The window is dense (more than 64 clusters): its n4 four-symbol clusters of three pairs go first, in
    rounds of 64 -- a round whose pairs + 30 exceed the queue in two halves (pair slots 0..1, then 2..3) --, its k2 two-symbol clusters
    after them in rounds of 64; whoever finds no room flushes whole lines of 16 first."""
    n = 0

    def add(t):
        nonlocal n
        if n + t > cap:
            n %= 16
        n += t
        assert n <= cap
    first = 3 * min(n4, 64)
    for r0 in range(0, n4, 64):
        m = min(64, n4 - r0)
        if 3 * m + 30 > cap:
            add(2 * m); add(m)
        else:
            add(3 * m)
    for r0 in range(0, k2, 64):
        add(min(64, k2 - r0))
    return n, first


@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("k2", [112, 127])
def test_room_flush_with_a_carry(k2, gran):
    """EBWT=1 (queue of 160), 20 equal windows in one workgroup of 16 waves: a wave that scores a second window comes to it with
    48 / 63 records waiting (fewer than a batch of 64: they stay at the window's top), and that window's first round of score_small3
    holds 192 pairs: two halves, and the first of them has to flush for room in front of the carry."""
    n4, windows = 64, 20
    waiting, first = _waiting_after_one_window(n4, k2, QCAP_SHORT)
    assert 48 <= waiting < 64 and first > QCAP_SHORT - 30 and waiting + 2 * n4 > QCAP_SHORT, (waiting, first)

    def make():
        lcp, da, eb = _blank(WIN * windows)
        for w in range(windows):
            for j in range(n4):
                _put(lcp, da, eb, w * WIN + 8 + 4 * j, [(191 * w + j) % NR, NR + 1, NR + 2, NR + 3])
            for j in range(k2):
                _put(lcp, da, eb, w * WIN + 300 + 2 * j, [(191 * w + 64 + j) % NR, NR + 4 + (w + j) % (NG - 4)])
        return lcp, da, eb
    ref = _reference(("room", k2), make)
    assert ref[2] == (windows * (n4 + k2), 4) and ref[1][1][1] == windows * (3 * n4 + k2)
    _check(_ctx(gran, max_blocks=1), ref, 1)


# ---- 5. a pool too small: counted, repeated ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ebwt", [1, 0])
@pytest.mark.parametrize("gran", GRANS)
def test_overflow_and_repeat(gran, ebwt):
    """a sub-region that is full only counts (base0 / base1 run on): the pass raises LIME_FLAG_POOL_FULL and lime_get_stats repeats it
    once with a pool sized from the counts"""
    import lime_amd
    ref = _reference(("carry", 1), lambda: O.synth(4701, 0, N_CARRY, NR, NG, ALPHA, 1))
    c = lime_amd.Context()
    try:
        for k, v in (("update_path", "bin"), ("flush_gran", gran), ("max_blocks", 1), ("pool_density", "0.001"), ("pool_slack", 0)):
            c.set_option(k, str(v))
        _check(c, ref, ebwt)
        assert c.host_times()["repeats"] == 1, c.host_times()
    finally:
        c.close()
