"""Out-of-range document ids on every update path (include/lime_hip.h, LIME_ERR_DOCID; DESIGN.md "malformed document ids").

A `da` value >= n_reads + n_refs is not exotic: numGenomes is a command-line argument of the drop-in programs, and a .da file can
belong to another collection.  The contract checked here, case by case:
  A. the pass ends in LIME_ERR_DOCID (-6) -- compare-and-swap, binned through the queue, binned with records written by the scorers;
     every cluster class; the id compared on all 32 bits (an id whose low 25 bits are a valid column must not alias to it);
  B. nothing outside the table is written: the table is a slice of a larger tensor with 1 MB of a known pattern on both sides;
  C. the same context then runs the well-formed background bit-exactly, and calls that do more after the pass (clusterChoose,
     lists, streams, the drop-in programs) return the error and hand out nothing.
And the boundary is exact: the same cluster with the id moved to n_reads + n_refs - 1 scores like the oracle says.

Inputs: a valid background of the oracle's generator into which ONE cluster of a chosen class with one out-of-range genome id
is spliced; O.detect must accept the spliced cluster with the intended length, or the case fails.  The reference's programs play
no part: they index SimArray_ with such an id unchecked (ClusterBWT_DA.cpp:178-184), which is undefined behaviour; the oracle is
used on valid inputs only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA = 16
BAND = 1 << 20
FILL = 0x3C
N_SMALL = 40 * 1024 + 500                       # 41 windows, the last one short
CLASSES = {"len2": 2, "len3": 3, "len4": 4, "dense4": 4, "rows8": 7, "rows16": 12, "mid": 40, "big": 100, "dup": 4}
# scorer of each class: score_len2; score_small3 (dense4: a window dense enough that a batch goes in two halves on the 16-wave EBWT=1
# kernel); score_rows3 G = 8, 16; group_score on the whole wave; k_score_big; dup_push -> group_score
POSITIONS = ("inside", "edge", "last")
IDS = ("exact", "beyond", "alias", "ffef")
# (n_reads, n_refs, LIME_BIN_LEVELS); compare-and-swap does not depend on the bin layout: the forced layouts run on the binned paths only
SMALL = [("cas", 3000, 300, None), ("cas", 40000, 700, None)] + \
        [(p, nr, ng, lv) for p in ("queue", "direct") for nr, ng, lv in ((3000, 300, None), (40000, 700, None), (3000, 300, "1,1"), (40000, 700, "4,7"))]

_CTX, _BUF, _BG = {}, {}, {}


def _ctx(path, levels=None):
    import lime_amd
    key = (path, levels)
    if key not in _CTX:
        c = lime_amd.Context()
        c.set_option("update_path", "cas" if path == "cas" else "bin")
        if levels:
            c.set_option("bin_levels", levels)
        if path != "cas":
            c.set_option("no_direct", "1" if path == "queue" else "0")
        _CTX[key] = c
    return _CTX[key]


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear(); _BUF.clear(); _BG.clear()


def _table(nr, ng):
    """the table as a slice of a larger caller-owned tensor: BAND bytes of FILL in front of it and behind it"""
    import torch
    import lime_amd
    sb = lime_amd.sim_bytes(nr, ng)
    if (nr, ng) not in _BUF:
        free = torch.cuda.mem_get_info()[0]
        if free < sb + 2 * BAND + (2 << 30):
            pytest.skip(f"{free >> 20} MB of device memory free, the table needs {sb >> 20}")
        _BUF.clear()                                                       # one table at a time
        _BUF[(nr, ng)] = torch.full((sb + 2 * BAND,), FILL, dtype=torch.uint8, device="cuda")
    big = _BUF[(nr, ng)]
    return big, big[BAND:BAND + sb]


def _bands_intact(big):
    import torch
    return bool(torch.all(big[:BAND] == FILL)) and bool(torch.all(big[-BAND:] == FILL))


def _dev(lcp, da, eb, ebwt):
    import torch
    return (torch.from_numpy(lcp.view(np.int32)).cuda(), torch.from_numpy(da.view(np.int32)).cuda(), torch.from_numpy(eb).cuda() if ebwt else None)


def _put(lcp, da, eb, p, docs):
    k = len(docs)
    lcp[p] = 0; lcp[p + 1:p + k] = ALPHA + 4
    if p + k < len(lcp):
        lcp[p + k] = 0
    da[p:p + k] = np.array(docs, np.uint64).astype(np.uint32); eb[p:p + k] = ord("A")


def splice(bg, pos, cls, gid, nr, reads, fill=(0, 0)):
    """bg with one cluster of class `cls` at `pos` whose last symbol belongs to document `gid`; the other documents are distinct valid
    ones (reads[0], more of `reads` as the class needs; genomes 1 ..), every symbol 'A' so that every read x genome pair scores"""
    lcp, da, eb = (x.copy() for x in bg)
    L, r0 = CLASSES[cls], reads[0]
    if cls == "len2":
        docs = [r0, gid]
    elif cls == "len3":
        docs = [nr + 1, r0, gid]
    elif cls in ("len4", "dense4"):
        docs = [r0, nr + 1, nr + 2, gid]
    elif cls == "dup":
        docs = [r0, r0, nr + 1, gid]
    else:
        n_r = 2 if L <= 16 else 5
        rs = list(reads[:n_r])
        assert len(set(rs)) == n_r
        docs = rs[1:] + [nr + 1 + i for i in range(L - n_r - 1)] + [r0, gid]
    assert len(docs) == L
    for j in range(1, fill[0] + 1):                                       # dense4: clusters of three pairs each in front of it and behind it
        _put(lcp, da, eb, pos - 4 * j, [reads[j % len(reads)], nr + 1, nr + 2, nr + 3])
    for j in range(fill[1], 0, -1):
        _put(lcp, da, eb, pos + 4 * j, [reads[j % len(reads)], nr + 1, nr + 2, nr + 3])
    _put(lcp, da, eb, pos, docs)
    return lcp, da, eb


DENSE_MIN = 64                                  # the scan lists a window's 2-symbol clusters apart once it owns more clusters than this
HALVES_PAIRS = 160 - 30                         # QCAP_SCAN_SHORT - 2 x 15: a round of score_small3 with more pairs goes out in two halves


def _round_of(cl, pos, fill):
    """The scan scores a window's clusters (those whose head it holds) in rounds of 64, in ascending position -- in a dense window without the
    2-symbol ones.  -> (filler clusters in the round of the cluster at `pos`, read x genome pairs of that round's 3- and 4-symbol fillers)"""
    w = pos // 1024
    own = cl[(cl[:, 0] // 1024) == w]
    if len(own) > DENSE_MIN:
        own = own[own[:, 1] != 2]
    starts = np.sort(own[:, 0].astype(np.int64))
    idx = int(np.searchsorted(starts, pos))
    assert starts[idx] == pos
    members = starts[64 * (idx // 64):64 * (idx // 64) + 64]
    fillers = {pos - 4 * j for j in range(1, fill[0] + 1)} | {pos + 4 * j for j in range(1, fill[1] + 1)}
    k = sum(int(m) in fillers for m in members)
    return idx, k, 3 * (k + 1)


def _dense_fill(bg, pos, where, nr, reads):
    """how many filler clusters go in front of / behind the dense4 cluster so that its round of 64 holds more than HALVES_PAIRS pairs"""
    if where != "edge":
        return (60, 60)                                                   # 60 on either side: its round holds fillers only
    fill = (64, 0)                                                        # the window ends with it: so many in front that it closes a round
    for _ in range(3):
        arrs = splice(bg, pos, "dense4", nr + 1 + 3, nr, reads, fill)
        idx, k, pairs = _round_of(O.detect(arrs[0], arrs[1], nr, ALPHA)[0], pos, fill)
        if idx % 64 == 63:
            break
        fill = (fill[0] + (63 - idx % 64), 0)
    return fill


def _pos(which, L, n):
    return {"inside": 7 * 1024 + 600, "edge": 20 * 1024 - 1, "last": n - L - 3}[which]


def _pos_of(which, cls, n):
    if cls == "dense4" and which == "last":
        return n - 4 - 3 - 4 * 60                                          # room for the fillers behind it, still in the last window
    return _pos(which, CLASSES[cls], n)


def _bad_id(kind, nr, ng):
    return {"exact": nr + ng, "beyond": nr + ng + 4096, "alias": nr + (1 << 25) + ng // 2, "ffef": 0xFFFFFFEF}[kind]


def _accepted(lcp, da, nr, pos, L):
    cl, nc, ml = O.detect(lcp, da, nr, ALPHA)
    assert ((cl[:, 0] == pos) & (cl[:, 1] == L)).any(), "the detector does not accept the spliced cluster: the case would pass vacuously"
    return cl, nc, ml


def _pass(c, arrs, ebwt, nr, ng, sim):
    tl, td, te = _dev(*arrs, ebwt)
    n = len(arrs[0])
    c.fused_dev(tl, td, te, n, n, True, nr, ng, ALPHA, sim)
    return c.stats()


def _background(nr, ng, n):
    key = (nr, ng, n)
    if key not in _BG:
        bg = O.synth(6100 + ng, 0, n, nr, ng, ALPHA, 1)
        cl, nc, ml = O.detect(bg[0], bg[1], nr, ALPHA)
        _BG.clear()
        _BG[key] = (bg, {e: O.score(bg[1], bg[2] if e else None, cl, nr, ng, threads=4) for e in (1, 0)}, (nc, ml))
    return _BG[key]


@pytest.mark.parametrize("where", POSITIONS)
@pytest.mark.parametrize("idkind", IDS)
@pytest.mark.parametrize("ebwt", [1, 0])
@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("path,nr,ng,levels", SMALL)
def test_bad_id_small_tables(path, nr, ng, levels, cls, ebwt, idkind, where):
    import torch
    n = N_SMALL
    bg, exp_bg, cnt_bg = _background(nr, ng, n)
    L = CLASSES[cls]
    pos = _pos_of(where, cls, n)
    reads = [nr - 1 if idkind == "beyond" else 17, 23, 29, 31, 37]       # "beyond": rd the last read, the cell lies behind the table
    fill = _dense_fill(bg, pos, where, nr, reads) if cls == "dense4" else (0, 0)
    bad = splice(bg, pos, cls, _bad_id(idkind, nr, ng), nr, reads, fill)
    cl_bad = _accepted(bad[0], bad[1], nr, pos, L)[0]
    if cls == "dense4":
        # the bad cluster sits in a round of 64 whose pairs do not fit the short queue of the 16-wave EBWT=1 record kernels: that round goes out
        # in two halves, the bad pair (slot 2 of its list) in the second -- checked here on the host, so that the case cannot pass vacuously
        idx, k, pairs = _round_of(cl_bad, pos, fill)
        assert pos // 1024 == (pos - 4 * fill[0]) // 1024 == (pos + 4 * fill[1]) // 1024, "the fillers lie in another window"
        assert k >= 44 and pairs > HALVES_PAIRS, (idx, k, pairs)
    c = _ctx(path, levels)
    big, sim = _table(nr, ng)
    # A + B
    s, rc = _pass(c, bad, ebwt, nr, ng, sim)
    assert rc == -6, (rc, s.flags)
    assert _bands_intact(big), "a failed pass wrote outside its table"
    # the context, its pool and its block cache are intact: the background, bit for bit
    s, rc = _pass(c, bg, ebwt, nr, ng, sim)
    assert rc == 0 and (s.n_clusters, s.max_len) == cnt_bg
    assert np.array_equal(sim[:nr * ng].cpu().numpy().reshape(nr, ng), exp_bg[ebwt])
    # the boundary is exact: the last column scores
    good = splice(bg, pos, cls, nr + ng - 1, nr, reads, fill)
    cl, nc, ml = _accepted(good[0], good[1], nr, pos, L)
    exp = O.score(good[1], good[2] if ebwt else None, cl, nr, ng, threads=4)
    s, rc = _pass(c, good, ebwt, nr, ng, sim)
    assert rc == 0 and (s.n_clusters, s.max_len) == (nc, ml)
    got = sim[:nr * ng].cpu().numpy().reshape(nr, ng)
    assert np.array_equal(got, exp), int((got != exp).sum())
    assert exp[reads[0], ng - 1] >= 1 and _bands_intact(big)


# ---- tables of two and of several sub-regions: a listed subset (path, class, id, EBWT, side of the 2^32 border the cluster's read lies on) ----
BIG_TWO = [
    ('cas', 'len2', 'beyond', 1, 'below'), ('cas', 'len2', 'beyond', 1, 'above'), ('cas', 'len2', 'beyond', 0, 'below'),
    ('cas', 'len2', 'beyond', 0, 'above'), ('cas', 'len2', 'alias', 1, 'below'), ('cas', 'len2', 'alias', 1, 'above'),
    ('cas', 'len2', 'alias', 0, 'below'), ('cas', 'len2', 'alias', 0, 'above'), ('cas', 'len4', 'beyond', 1, 'below'),
    ('cas', 'len4', 'beyond', 1, 'above'), ('cas', 'len4', 'beyond', 0, 'below'), ('cas', 'len4', 'beyond', 0, 'above'),
    ('cas', 'len4', 'alias', 1, 'below'), ('cas', 'len4', 'alias', 1, 'above'), ('cas', 'len4', 'alias', 0, 'below'),
    ('cas', 'len4', 'alias', 0, 'above'), ('cas', 'rows8', 'beyond', 1, 'below'), ('cas', 'rows8', 'beyond', 1, 'above'),
    ('cas', 'rows8', 'beyond', 0, 'below'), ('cas', 'rows8', 'beyond', 0, 'above'), ('cas', 'rows8', 'alias', 1, 'below'),
    ('cas', 'rows8', 'alias', 1, 'above'), ('cas', 'rows8', 'alias', 0, 'below'), ('cas', 'rows8', 'alias', 0, 'above'),
    ('queue', 'len2', 'beyond', 1, 'below'), ('queue', 'len2', 'beyond', 1, 'above'), ('queue', 'len2', 'beyond', 0, 'below'),
    ('queue', 'len2', 'beyond', 0, 'above'), ('queue', 'len2', 'alias', 1, 'below'), ('queue', 'len2', 'alias', 1, 'above'),
    ('queue', 'len2', 'alias', 0, 'below'), ('queue', 'len2', 'alias', 0, 'above'), ('queue', 'len4', 'beyond', 1, 'below'),
    ('queue', 'len4', 'beyond', 1, 'above'), ('queue', 'len4', 'beyond', 0, 'below'), ('queue', 'len4', 'beyond', 0, 'above'),
    ('queue', 'len4', 'alias', 1, 'below'), ('queue', 'len4', 'alias', 1, 'above'), ('queue', 'len4', 'alias', 0, 'below'),
    ('queue', 'len4', 'alias', 0, 'above'), ('queue', 'rows8', 'beyond', 1, 'below'), ('queue', 'rows8', 'beyond', 1, 'above'),
    ('queue', 'rows8', 'beyond', 0, 'below'), ('queue', 'rows8', 'beyond', 0, 'above'), ('queue', 'rows8', 'alias', 1, 'below'),
    ('queue', 'rows8', 'alias', 1, 'above'), ('queue', 'rows8', 'alias', 0, 'below'), ('queue', 'rows8', 'alias', 0, 'above'),
    ('direct', 'len2', 'beyond', 1, 'below'), ('direct', 'len2', 'beyond', 1, 'above'), ('direct', 'len2', 'beyond', 0, 'below'),
    ('direct', 'len2', 'beyond', 0, 'above'), ('direct', 'len2', 'alias', 1, 'below'), ('direct', 'len2', 'alias', 1, 'above'),
    ('direct', 'len2', 'alias', 0, 'below'), ('direct', 'len2', 'alias', 0, 'above'), ('direct', 'len4', 'beyond', 1, 'below'),
    ('direct', 'len4', 'beyond', 1, 'above'), ('direct', 'len4', 'beyond', 0, 'below'), ('direct', 'len4', 'beyond', 0, 'above'),
    ('direct', 'len4', 'alias', 1, 'below'), ('direct', 'len4', 'alias', 1, 'above'), ('direct', 'len4', 'alias', 0, 'below'),
    ('direct', 'len4', 'alias', 0, 'above'), ('direct', 'rows8', 'beyond', 1, 'below'), ('direct', 'rows8', 'beyond', 1, 'above'),
    ('direct', 'rows8', 'beyond', 0, 'below'), ('direct', 'rows8', 'beyond', 0, 'above'), ('direct', 'rows8', 'alias', 1, 'below'),
    ('direct', 'rows8', 'alias', 1, 'above'), ('direct', 'rows8', 'alias', 0, 'below'), ('direct', 'rows8', 'alias', 0, 'above'),
]
BIG_THREE = [
    ('queue', 'len2', 'beyond', 1, 'below'), ('queue', 'len2', 'beyond', 0, 'below'), ('queue', 'len2', 'alias', 1, 'below'),
    ('queue', 'len2', 'alias', 0, 'below'), ('queue', 'len4', 'beyond', 1, 'below'), ('queue', 'len4', 'beyond', 0, 'below'),
    ('queue', 'len4', 'alias', 1, 'below'), ('queue', 'len4', 'alias', 0, 'below'), ('queue', 'rows8', 'beyond', 1, 'below'),
    ('queue', 'rows8', 'beyond', 0, 'below'), ('queue', 'rows8', 'alias', 1, 'below'), ('queue', 'rows8', 'alias', 0, 'below'),
]


def _big_case(nr, ng, k_border, path, cls, idkind, ebwt, side):
    """every read of the background in the seven rows around cell k_border * 2^32 (as test_records_written_by_the_scorers_or_through_the_queue
    places them): those rows against the oracle, every other byte of the table zero"""
    import torch
    n = 200 * 1024 + 300
    lo_r = (k_border << 32) // ng - 3
    key = ("big", nr, ng)
    if key not in _BG:
        lcp, da, eb = O.synth(99 + ng, 0, n, nr, ng, ALPHA, 1)
        sel = da < nr
        da[sel] = (lo_r + da[sel] % 7).astype(np.uint32)
        _BG.clear()
        _BG[key] = (lcp, da, eb)
    bg = _BG[key]

    def rows_of(arrs):
        cl, nc, ml = O.detect(arrs[0], arrs[1], nr, ALPHA)
        d7 = np.where(arrs[1] < nr, arrs[1] - lo_r, arrs[1] - nr + 7).astype(np.uint32)     # the same clusters with the 7 reads renumbered 0..6
        return O.score(d7, arrs[2] if ebwt else None, cl, 7, ng, threads=4), (nc, ml)

    def check(sim, arrs):
        rows, cnt = rows_of(arrs)
        got = sim[lo_r * ng:(lo_r + 7) * ng].cpu().numpy().reshape(7, ng)
        assert np.array_equal(got, rows), int((got != rows).sum())
        assert int(torch.count_nonzero(sim[:lo_r * ng])) == 0 and int(torch.count_nonzero(sim[(lo_r + 7) * ng:nr * ng])) == 0
        return rows, cnt

    L = CLASSES[cls]
    pos = _pos("inside", L, n)
    r0 = lo_r if side == "below" else lo_r + 6
    assert (r0 * ng < (k_border << 32)) == (side == "below")
    good_reads = [r0, lo_r + 2, lo_r + 4]
    bad_reads = [nr - 1 if idkind == "beyond" else r0, lo_r + 2, lo_r + 4]
    bad = splice(bg, pos, cls, _bad_id(idkind, nr, ng), nr, bad_reads)
    _accepted(bad[0], bad[1], nr, pos, L)
    c = _ctx(path)
    big, sim = _table(nr, ng)
    s, rc = _pass(c, bad, ebwt, nr, ng, sim)
    assert rc == -6, (rc, s.flags)
    assert _bands_intact(big), "a failed pass wrote outside its table"
    s, rc = _pass(c, bg, ebwt, nr, ng, sim)
    assert rc == 0
    _, cnt = check(sim, bg)
    assert (s.n_clusters, s.max_len) == cnt
    good = splice(bg, pos, cls, nr + ng - 1, nr, good_reads)
    _accepted(good[0], good[1], nr, pos, L)
    s, rc = _pass(c, good, ebwt, nr, ng, sim)
    assert rc == 0
    rows, cnt = check(sim, good)
    assert (s.n_clusters, s.max_len) == cnt and rows[r0 - lo_r, ng - 1] >= 1 and _bands_intact(big)


@pytest.mark.parametrize("path,cls,idkind,ebwt,side", BIG_TWO)
def test_bad_id_two_sub_regions(path, cls, idkind, ebwt, side):
    _big_case(1_100_000, 4000, 1, path, cls, idkind, ebwt, side)          # 4.4 GB


@pytest.mark.parametrize("path,cls,idkind,ebwt,side", BIG_THREE)
def test_bad_id_three_sub_regions(path, cls, idkind, ebwt, side):
    _big_case(3_000_000, 3423, 2, path, cls, idkind, ebwt, side)          # 10.3 GB, the shape of test_tables_of_several_sub_regions_vs_oracle


# ---- beyond the matrix ----------------------------------------------------------------------------------------------------
# (the smallest case -- four positions, a 1 x 2 table, compare-and-swap through emit() -- stays where it was:
# tests/test_gpu_parity.py::test_docid_out_of_range_is_reported)
EXTRA_SHAPE = (3000, 300)


def _extra_inputs(idkind="alias", cls="len4", where="inside"):
    nr, ng = EXTRA_SHAPE
    bg, exp_bg, cnt_bg = _background(nr, ng, N_SMALL)
    pos = _pos(where, CLASSES[cls], N_SMALL)
    bad = splice(bg, pos, cls, _bad_id(idkind, nr, ng), nr, [17, 23, 29, 31, 37])
    cl, nc, ml = _accepted(bad[0], bad[1], nr, pos, CLASSES[cls])
    return bg, exp_bg, bad, cl


@pytest.mark.parametrize("path", ["cas", "queue", "direct"])
@pytest.mark.parametrize("idkind", ["exact", "alias"])
def test_score_list_with_a_bad_id(path, idkind):
    """lime_score_dev over a cluster list (k_score_list)"""
    import torch
    nr, ng = EXTRA_SHAPE
    bg, exp_bg, bad, cl = _extra_inputs(idkind)
    c = _ctx(path)
    big, sim = _table(nr, ng)
    tl, td, te = _dev(*bad, True)
    tc = torch.from_numpy(np.ascontiguousarray(cl, np.uint64).view(np.int64)).cuda()
    c.score_dev(td, te, len(bad[1]), tc.data_ptr(), len(cl), nr, ng, sim)
    s, rc = c.stats()
    assert rc == -6 and _bands_intact(big)
    s, rc = _pass(c, bg, 1, nr, ng, sim)
    assert rc == 0 and np.array_equal(sim[:nr * ng].cpu().numpy().reshape(nr, ng), exp_bg[1])


@pytest.mark.parametrize("path", ["queue", "direct"])
@pytest.mark.parametrize("free", ["0", "1"])
@pytest.mark.parametrize("idkind", ["exact", "alias"])
def test_choose_hands_out_nothing_after_a_bad_id(free, idkind, path):
    """lime_fused_choose_dev with the table and without it, lime_fused_choose_lists_dev: -6 from the call, no pairs, no lists (so nothing
    lime_classify_lists_dev could be given)"""
    import lime_amd
    from lime_amd import _lib
    from lime_amd.api import _ptr
    nr, ng = EXTRA_SHAPE
    bg, exp_bg, bad, cl = _extra_inputs(idkind)
    c = lime_amd.Context()
    try:
        c.set_option("update_path", "bin"); c.set_option("bin_levels", "1,2"); c.set_option("choose_free", free)
        c.set_option("no_direct", "1" if path == "queue" else "0")
        tl, td, te = _dev(*bad, True)
        n = len(bad[0])
        mx = np.zeros(nr + 1, np.uint8); off = np.zeros(nr + 2, np.uint64)
        pp, npairs, st = C.c_void_p(), C.c_uint64(0), _lib.Stats()
        rc = c.lib.lime_fused_choose_dev(c.h, _ptr(tl), _ptr(td), _ptr(te), n, nr, ng, ALPHA, 85, C.c_float(0.0), mx.ctypes.data, off.ctypes.data,
                                         C.byref(pp), C.byref(npairs), C.byref(st), None)
        assert rc == -6 and not pp.value and npairs.value == 0
        assert st.wave_records_max > 0 and c.host_times()["cas_fallbacks"] == 0      # the pass left update records: binned, not compare-and-swap
        assert c.host_times()["choose_without_table"] == int(free)
        h = C.c_void_p()
        rc = c.lib.lime_fused_choose_lists_dev(c.h, _ptr(tl), _ptr(td), _ptr(te), n, nr, ng, ALPHA, 85, C.c_float(0.0), C.byref(h), C.byref(st), None)
        assert rc == -6 and not h.value and st.wave_records_max > 0
        # the same context, the background: lists as from the oracle's table
        tl, td, te = _dev(*bg, True)
        rmx, roff, pairs, s = c.fused_choose_dev(tl, td, te, n, nr, ng, ALPHA, 85, 0.0)
        assert np.array_equal(rmx, exp_bg[1].max(axis=1)) and len(pairs) == int((exp_bg[1] > 0).sum())
    finally:
        c.close()


@pytest.mark.parametrize("path", ["queue", "direct"])
@pytest.mark.parametrize("chunk,where", [(65536, "inside"), (8192, "inside"), (8192, "last")])
def test_stream_with_a_bad_id_in_the_first_or_a_later_chunk(path, chunk, where):
    """lime_fused_stream.  One chunk (65536 >= n): the forced record path serves it.  Chunks of 8192, the bad id in chunk 0 / in the last one:
    the chunks of a multi-chunk stream ADD to one table, which only compare-and-swap can do (fused_dev_impl, no_bin) -- whatever path is
    asked for, and the test says so instead of assuming a path."""
    import lime_amd
    nr, ng = EXTRA_SHAPE
    bg, exp_bg, bad, cl = _extra_inputs("alias", "len4", where)
    c = lime_amd.Context()
    try:
        c.set_option("update_path", "bin"); c.set_option("no_direct", "1" if path == "queue" else "0")
        with pytest.raises(lime_amd.LimeError) as e:
            c.fused_stream(bad[0], bad[1], bad[2], nr, ng, ALPHA, chunk=chunk)
        assert e.value.code == -6
        s, rc = c.stats()
        assert rc == -6 and (s.wave_records_max > 0) == (chunk >= N_SMALL) and c.host_times()["cas_fallbacks"] == 0
        sim, nc, ml = c.fused_stream(bg[0], bg[1], bg[2], nr, ng, ALPHA, chunk=chunk)
        assert np.array_equal(sim, exp_bg[1])
    finally:
        c.close()


@pytest.mark.parametrize("path", ["cas", "queue", "direct"])
def test_sharded_pass_reports_from_the_owner_of_the_head(path):
    """two position-range shards; the bad cluster lies in shard 0's halo = shard 1's owned range: shard 1 alone reports it"""
    from lime_amd.dist import shard_ranges
    nr, ng, n = 3000, 300, 400_000
    bg = O.synth(6200, 0, n, nr, ng, ALPHA, 1)
    ranges = list(shard_ranges(n, 2, halo=65536 + 4096))
    pos = ranges[0][1] + 1000
    assert ranges[1][0] <= pos < ranges[1][1] and pos + 8 < ranges[0][2]
    bad = splice(bg, pos, "len4", _bad_id("alias", nr, ng), nr, [17, 23, 29])
    _accepted(bad[0], bad[1], nr, pos, 4)
    c = _ctx(path)
    big, sim = _table(nr, ng)
    rcs = []
    for lo, hi, hi_halo in ranges:
        tl, td, te = _dev(bad[0][lo:hi_halo], bad[1][lo:hi_halo], bad[2][lo:hi_halo], True)
        c.fused_dev(tl, td, te, hi - lo, hi_halo - lo, hi_halo == n, nr, ng, ALPHA, sim)
        st, rc = c.stats()
        assert (st.wave_records_max > 0) == (path != "cas"), (path, st.wave_records_max)      # the path asked for served the shard
        rcs.append(rc)
    assert rcs == [0, -6], (path, rcs)
    assert _bands_intact(big)


def _example_files(d, drop_last_genome_of_lineage):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_example as G
    from lime_amd.builder import build_arrays_sa
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_full.npz"))
    genomes, sets = G.collections(z["reads_1"], z["reads_2"], z["src"])
    bases = []
    for name in G.SETS:
        base = os.path.join(d, f"{name}.fasta")
        ebwt, lcp, da = build_arrays_sa(sets[name], genomes, term=0)
        lcp.astype("<u4").tofile(base + ".lcp"); da.astype("<u4").tofile(base + ".da"); ebwt.tofile(base + ".ebwt")
        bases.append((base, lcp, da))
    tax = os.path.join(d, "LineageFile.csv")
    lines = bytes(z["lineage"]).splitlines(keepends=True)
    if drop_last_genome_of_lineage:                                       # (the taxonomy must have as many entries as numGenomes says)
        last = max(k for k, l in enumerate(lines) if l.strip())
        del lines[last]
    open(tax, "wb").write(b"".join(lines))
    return bases, tax, len(z["reads_1"]), len(genomes), G.READ_LEN


def test_drop_ins_with_numgenomes_one_too_small(tmp_path):
    """ClusterBWT_DA and LiME_paired on the example with numGenomes one too small: a normal non-zero exit, the DOCID message, no output file"""
    from lime_amd import _lib
    d = str(tmp_path)
    bases, tax, n_reads, n_gen, read_len = _example_files(d, True)
    before = set(os.listdir(d))
    exe = os.path.join(ROOT, "lime_amd", "bin", "LiME_paired")
    out = os.path.join(d, "classification.txt")
    p = subprocess.run([exe] + [b[0] for b in bases] + [out, str(n_reads), str(n_gen - 1), tax, str(read_len), "4"], capture_output=True, timeout=600, cwd=d)
    assert p.returncode > 0, (p.returncode, p.stderr.decode()[-2000:])
    assert b"da value >= n_reads + n_refs" in p.stderr, p.stderr.decode()[-2000:]
    assert set(os.listdir(d)) == before
    # ClusterBWT_DA: the cluster list and the auxiliary file of the first collection, written for one genome too few
    lib = _lib.load()
    base, lcp, da = bases[0]
    cl, nc, ml = O.detect(lcp.astype(np.uint32), da.astype(np.uint32), n_reads, ALPHA)
    cl = np.ascontiguousarray(cl, np.uint64)
    assert lib.lime_write_clrs((base + f".{ALPHA}.clrs").encode(), cl.ctypes.data, len(cl)) == 0
    assert lib.lime_write_aux(os.path.join(d, os.path.basename(base)[:-len(".fasta")] + ".out").encode(), n_reads, n_gen - 1, ALPHA, ml, nc) == 0
    before = set(os.listdir(d))
    exe = os.path.join(ROOT, "lime_amd", "bin", "ClusterBWT_DA")
    p = subprocess.run([exe, base, str(read_len), "0.25", "4"], capture_output=True, timeout=600, cwd=d)
    assert p.returncode > 0, (p.returncode, p.stderr.decode()[-2000:])
    assert b"da value >= n_reads + n_refs" in p.stderr, p.stderr.decode()[-2000:]
    assert set(os.listdir(d)) == before
