"""tests/part_cases.py without a GPU: every named case holds the edge it is named for -- derived again from the pool and the counts, not from
the builder's parameters, so that tests/test_part_edges_gpu.py cannot lose an edge quietly when a builder changes --, the model against a
record-by-record loop and against the library's own lime_rec_bin, every case against lime_partition_records_dev's argument rules, and the
comparer against corrupted outputs: that is how the GPU tests are known to be able to fail."""
import functools

import numpy as np
import pytest

from tests import part_cases as PC

ALL = list(PC.CASES) + PC.FUZZ
T = PC.PART_TILE


@functools.lru_cache(maxsize=None)
def _case(name):
    c = PC.make(name)
    m = PC.Model(c)
    return c, m


@functools.lru_cache(maxsize=None)
def _sim(name):
    c, m = _case(name)
    return PC.carry_sim(c, m)


def _kinds(name):
    return [[t[0] for t in tiles] for tiles in PC.tile_table(_case(name)[0])]


@pytest.mark.parametrize("name", ALL)
def test_case_obeys_the_entry_points_rules(name):
    c, m = _case(name)
    assert PC.geometry_error(c.n_prod, c.prod_waves, c.n_sub, c.cap_w, c.pool, c.wave_cnt, c.n_bins, c.bin_shift, m.total) is None
    assert len(c.pool) * 4 <= 9 << 20                                     # a pool of a few MB
    # beyond a segment's count lies the filling, and nothing else
    live = np.zeros(len(c.pool), dtype=bool)
    r = m.rec
    live[r.seg * c.cap_w + (r.spos - r.seg_p[r.prod, r.seg % c.n_seg])] = True
    assert int(live.sum()) == m.total and (c.pool[~live] == PC.FILL).all()
    assert int(m.binbase[-1]) == m.total == int(m.counts.sum())


@pytest.mark.parametrize("name", ALL)
def test_bins_agree_with_the_library(name):
    """lime_rec_bin (the host side of lime_device.h's rec_bin) on every record of the case"""
    from lime_amd import _lib
    lib = _lib.load()
    c, m = _case(name)
    r = m.rec
    pairs = np.unique(np.stack([r.rec.astype(np.int64), r.sub, r.bin], axis=1), axis=0)
    if len(pairs) > 20000:
        pairs = pairs[np.random.default_rng(1).permutation(len(pairs))[:20000]]
    for rec, sub, b in pairs.tolist():
        assert lib.lime_rec_bin(rec, sub, c.bin_shift) == b
    assert len(pairs) == 0 or (0 <= pairs[:, 2].min() and pairs[:, 2].max() < c.n_bins)


@pytest.mark.parametrize("name", ALL)
def test_model_is_a_permutation_of_the_input_per_bin(name):
    c, m = _case(name)
    r = m.rec
    order = np.lexsort((r.word, r.bin))
    lo = m.binbase.astype(np.int64)
    assert np.array_equal(np.bincount(r.bin, minlength=c.n_bins), np.diff(lo))
    # the model's words of bin b, sorted, are the input's words of bin b, sorted
    mb = m.rid // c.n_prod
    assert np.array_equal(mb, r.bin[order])
    assert np.array_equal(m.want[np.lexsort((m.want, mb))], r.word[order])
    assert m.total == 0 or int((m.want >> np.uint32(c.bin_shift)).min()) == int((m.want >> np.uint32(c.bin_shift)).max()) == 1


SMALL = [n for n in ALL if not n.startswith(("fuzz_", "bins_")) and n not in ("tile_edges", "tile_straddle", "one_bin_full_tiles", "carry_trickle")] + \
        ["bins_65_dense", "bins_513_sparse", "fuzz_0"]


@pytest.mark.parametrize("name", SMALL)
def test_model_equals_a_loop_over_the_records(name):
    c, m = _case(name)
    base, ranges = PC.model_naive(c)
    assert base == m.binbase.tolist()
    at = 0
    for b in range(c.n_bins):
        for p in range(c.n_prod):
            w = ranges.get((b, p), [])
            assert int(m.start[b, p]) == at and int(m.counts[b, p]) == len(w)
            assert m.want[at:at + len(w)].tolist() == w
            at += len(w)
    assert at == m.total


# ---- the facts the cases are named for -------------------------------------------------------------------------------------------------
def test_empty_and_one_record():
    c, m = _case("empty")
    assert m.total == 0 and c.n_bins == 3 and (m.binbase == 0).all() and all(t == [] for t in PC.tile_table(c))
    c, m = _case("one_record")
    assert m.total == 1 and c.wave_cnt.tolist() == [0] * (len(c.wave_cnt) - 1) + [1] and c.n_sub == 2 and int(m.rec.sub[0]) == 1


def test_pad_mod4():
    c, m = _case("pad_mod4")
    assert c.n_prod == 1 and c.wave_cnt.tolist() == [1, 2, 3, 5, 6, 7, 0, 4] == c.facts["counts"]
    assert {(-n) % 4 for n in c.wave_cnt.tolist()} == {0, 1, 2, 3}
    (tiles,) = PC.tile_table(c)
    assert tiles == [("mixed", 28, [0, 1, 2, 3, 4, 5, 7])]


def test_tile_edges():
    c, m = _case("tile_edges")
    assert c.wave_cnt.tolist() == [T - 1, T, T + 1, 2 * T, 2 * T + 1] and c.n_seg == 1
    tt = PC.tile_table(c)
    assert [[t[:2] for t in p] for p in tt] == [[("one", T - 1)], [("one", T)], [("one", T), ("one", 1)], [("one", T)] * 2, [("one", T)] * 2 + [("one", 1)]]
    assert {t[1] % 4 for p in tt for t in p} >= {0, 1, 3}                  # tn that is no multiple of four


def test_tile_straddle():
    c, m = _case("tile_straddle")
    assert c.wave_cnt.tolist() == [8190, 6, 0, 8200, 3, 5, 16376, 0, 0, 0]
    t0, t1 = PC.tile_table(c)
    assert t0 == [("one", 8190, [0]), ("mixed", 6 + 8184, [1, 3]), ("mixed", 16 + 3, [3, 4])]        # the cut at 8192 lies behind two padding words
    assert t1 == [("mixed", 5 + 8184, [0, 1]), ("one", 8192, [1])]
    kinds = _kinds("tile_straddle")
    assert ["one", "mixed"] == kinds[0][:2] and ["mixed", "one"] == kinds[1]


def test_one_bin_full_tiles():
    c, m = _case("one_bin_full_tiles")
    sim = _sim("one_bin_full_tiles")
    r = m.rec
    assert c.n_bins == 64
    full = [(p, t) for p in range(c.n_prod) for t in range(3) if ((r.prod == p) & (r.tile == t)).sum() == T and (r.bin[(r.prod == p) & (r.tile == t)] == 5).all()]
    assert full == [(0, 0), (1, 0), (2, 0), (3, 2)]
    assert (m.start[5, :4] % 16).tolist() == [0, 1, 15, 15]
    assert sim["lines"][0][0] == sim["lines"][1][0] == sim["lines"][2][0] == 512
    assert max(sim["lines"][3]) == 526 > 512                             # 511 lines of bin 5 and 15 completed carries in one tile
    assert sim["lines"][3][1] <= T // 16 + 16                              # (PL_TASKS)
    assert sim["max_carry"] == 15


def test_carry_trickle():
    c, m = _case("carry_trickle")
    sim = _sim("carry_trickle")
    assert all(len(t) == 18 and all(k == ("one", T, [0]) for k in t) for t in PC.tile_table(c))
    assert sim["max_carry"] == 15
    left = {lo for ca, lo in sim["completes"] if ca == 15}
    assert 0 in left and 1 in left and max(left) >= 2, sim["completes"]
    per_tile = np.bincount(m.rec.tile[m.rec.bin > 0] * 32 + m.rec.bin[m.rec.bin > 0], minlength=18 * 32 * 2)
    assert set(np.unique(per_tile).tolist()) >= {0, 1, 2} and (m.counts[0] > 18 * T - 1000).all()
    assert (m.start % 16 == 0).all()


def test_first_piece():
    c, m = _case("first_piece")
    sim = _sim("first_piece")
    assert c.n_prod == 20 and int(c.wave_cnt.max()) <= 256 and all(len(t) == 1 for t in PC.tile_table(c))
    have = {(s, e) for s, e, n in sim["first"] if n <= 32}
    for r in range(16):
        for e in (15, 0, 1):
            assert (r, e) in have, (r, e)
    assert c.facts["pieces"] <= have


def test_producers_and_prod_waves():
    assert PC.PRODUCER_COUNTS == [1, 63, 64, 65, 128, 130] and PC.PROD_WAVES == [1, 4, 6, 8, 12, 16]
    for n in PC.PRODUCER_COUNTS:
        c, m = _case(f"producers_{n}")
        assert c.n_prod == n and m.total > 0
        per = m.counts.sum(axis=0)
        assert n < 8 or ((per == 0).any() and (per[64:] > 0).any() == (n > 64))
        if n > 64:                                                        # the rowscan's carry from the first chunk of 64 producers is not zero
            assert (m.counts[:, :64].sum(axis=1) > 0).all() and (m.counts[:, 64:].sum(axis=1) > 0).any()
    shapes = set()
    for pw in PC.PROD_WAVES:
        c, m = _case(f"prod_waves_{pw}")
        assert c.prod_waves == pw and c.n_sub == 2
        shapes.add((c.n_prod, c.n_bins, c.bin_shift))
        assert set(np.unique(m.rec.sub).tolist()) == {0, 1}
    assert len(shapes) == 1


def test_bins():
    assert PC.BINS_LINES == [1, 2, 63, 64, 65, 255, 256] and PC.BINS_EITHER == [511, 512, 513, 1024, 1025, 1536, 1537, 3071, 3072]
    for n in PC.BINS_LINES + PC.BINS_EITHER + PC.BINS_LAYOUT:
        c, m = _case(f"bins_{n}_dense")
        assert c.n_bins == n and (np.diff(m.binbase.astype(np.int64)) > 0).all()
        c, m = _case(f"bins_{n}_sparse")
        nz = np.nonzero(np.diff(m.binbase.astype(np.int64)))[0].tolist()
        assert c.n_bins == n and nz == sorted(set([0, n - 1] + list(range(0, n, 97))))


def test_sub_regions():
    for key, (n_sub, sh, n_bins, pw) in PC.SUB_REGIONS.items():
        c, m = _case(f"sub_regions_{key}")
        assert (c.n_sub, c.bin_shift, c.n_bins, c.prod_waves) == (n_sub, sh, n_bins, pw)
        subs = set(np.unique(m.rec.sub).tolist())
        assert subs == ({0} if key == "3_20" else set(range(4)) if key == "8_25_low" else set(range(n_sub)))
        if key != "3_20":                                                 # tiles mix segments of different sub-regions
            r = m.rec
            per_tile = {}
            for p, t, s in set(zip(r.prod.tolist(), r.tile.tolist(), r.sub.tolist())):
                per_tile.setdefault((p, t), set()).add(s)
            assert any(len(v) > 1 for v in per_tile.values())
        off = m.rec.rec & np.uint32((1 << sh) - 1)
        assert (off == 0).any() and (off == (0xFFFFFFFF >> (32 - sh))).any()
    for key in ("8_25", "8_25_low"):
        c, _ = _case(f"sub_regions_{key}")
        assert c.n_seg == 128 == PC.PROD_WAVES_MAX * PC.MAX_SUB
    assert PC.bins_per_sub(20) > PC.BIN_MAX                               # why "3_20" cannot hold a record outside sub-region 0


def test_offsets():
    for sh in (16, 25):
        c, m = _case(f"offsets_{sh}")
        assert c.bin_shift == sh
        for b in (0, c.n_bins - 1):
            w = m.want[int(m.binbase[b]):int(m.binbase[b + 1])] & np.uint32((1 << sh) - 1)
            assert 0 in w and (1 << sh) - 1 in w
    c, m = _case("offsets_25")
    assert (m.rec.rec == PC.FILL).any() and c.n_bins == PC.bins_per_sub(25)


def test_fuzz_shapes():
    assert len(PC.FUZZ) == 12
    seen = dict(n_sub=set(), pw=set(), zero=False, near=False, mixed=False, one=False)
    for name in PC.FUZZ:
        c, m = _case(name)
        assert c.n_prod <= 6 and c.n_bins <= 600 and int(c.wave_cnt.max()) <= 20000
        seen["n_sub"].add(c.n_sub); seen["pw"].add(c.prod_waves)
        cnt = c.wave_cnt.astype(np.int64)
        seen["zero"] |= bool((cnt == 0).any())
        seen["near"] |= bool(((cnt > 100) & (np.abs((cnt + T // 2) % T - T // 2) <= 2)).any())
        kinds = {k for p in _kinds(name) for k in p}
        seen["mixed"] |= "mixed" in kinds; seen["one"] |= "one" in kinds
    assert len(seen["n_sub"]) >= 3 and len(seen["pw"]) >= 3 and seen["zero"] and seen["near"] and seen["mixed"] and seen["one"], seen


def test_test_bases():
    """the p64_test_base values the GPU test takes from the model put 2^32 where they say"""
    kinds = {}
    for name in ALL:
        c, m = _case(name)
        sim = _sim(name)
        for kind, base in PC.p64_bases(c, m, sim).items():
            assert base % 16 == 0
            pos = (1 << 32) - base
            kinds.setdefault(kind, []).append(name)
            if kind == "bin_first":
                assert pos in m.binbase[1:-1].astype(np.int64).tolist() and 0 < pos < m.total
            elif kind == "mid_range":
                inside = (m.start + 2 * T <= pos) & (pos < m.start + m.counts)
                assert inside.sum() == 1
            elif kind == "flush":
                inside = (sim["flush_g"] == pos) & (sim["flush_c"] > 0)
                assert inside.sum() == 1 and 0 < pos < m.total
            else:
                assert base == (1 << 33) + 48
    assert all("one_bin_full_tiles" in kinds[k] for k in ("bin_first", "mid_range", "flush", "above")) and "tile_edges" in kinds["flush"]
    assert "carry_trickle" in kinds["mid_range"] and "carry_trickle" in kinds["bin_first"]
    assert len(kinds["flush"]) > 20 and len(kinds["bin_first"]) > 20


# ---- the comparer ----------------------------------------------------------------------------------------------------------------------
def _good(c, m, seed=1):
    """a correct output: the model's ranges, each in a seeded order of its own"""
    rng = np.random.default_rng(seed)
    buf = PC.output_buffer(m.total)
    body = m.want.copy()
    key = rng.random(m.total)
    body = body[np.lexsort((key, m.rid))]
    buf[PC.GUARD:PC.GUARD + m.total] = body
    return buf


@pytest.mark.parametrize("name", ALL)
def test_comparer_accepts_any_order_inside_a_range(name):
    c, m = _case(name)
    assert PC.compare(c, m, _good(c, m), m.binbase) is None


@pytest.mark.parametrize("name", ["first_piece", "tile_straddle", "carry_trickle", "sub_regions_8_25", "bins_3072_dense", "fuzz_3"])
def test_comparer_rejects_corrupted_outputs(name):
    c, m = _case(name)
    G = PC.GUARD
    good = _good(c, m)
    body = good[G:G + m.total]
    cnt = m.counts

    def rejected(buf, binbase=m.binbase, *needles):
        msg = PC.compare(c, m, buf, binbase)
        assert msg is not None and all(n in msg for n in needles), msg
        return msg

    # two records swapped between neighbouring producers' ranges of one bin
    found = False
    for b, p in np.argwhere((cnt[:, :-1] > 0) & (cnt[:, 1:] > 0)).tolist():
        i, j = int(m.start[b, p]), int(m.start[b, p + 1])
        if body[i] != body[j] and body[i] not in body[j:j + cnt[b, p + 1]] and body[j] not in body[i:i + cnt[b, p]]:
            bad = good.copy(); bad[G + i], bad[G + j] = good[G + j], good[G + i]
            msg = rejected(bad, m.binbase, f"bin {b} producer {p} ", "from tiles")
            assert f"bin {b} producer {p + 1} " in msg
            found = True
            break
    assert found or c.n_prod == 1
    # a record's t bit cleared
    bad = good.copy(); bad[G + m.total // 2] &= np.uint32((1 << c.bin_shift) - 1)
    rejected(bad)
    # a padding word in place of a record
    bad = good.copy(); bad[G + m.total // 3] = PC.FILL
    rejected(bad)
    # one word shifted by one position across a bin border: the last word of a bin is written one place further, over the next bin's first
    b = next(b for b in range(c.n_bins - 1) if m.binbase[b + 1] > m.binbase[b] and m.binbase[b + 2] > m.binbase[b + 1]
             and body[int(m.binbase[b + 1]) - 1] != body[int(m.binbase[b + 1])])
    e = int(m.binbase[b + 1])
    bad = good.copy(); bad[G + e] = good[G + e - 1]; bad[G + e - 1] = PC.OUT_FILL
    rejected(bad, m.binbase, "never written")
    # a guard word changed, on either side
    bad = good.copy(); bad[G - 1] = 0
    rejected(bad, m.binbase, "guard words in front")
    bad = good.copy(); bad[G + m.total] = good[G]
    rejected(bad, m.binbase, "guard words behind")
    # a bin base off by one
    bb = m.binbase.copy(); bb[c.n_bins // 2] += np.uint64(1)
    rejected(good, bb, "binbase")
    # and a record that went to the neighbouring tile's producer: a word of the model replaced by a word of another bin
    bad = good.copy(); bad[G] = good[G + m.total - 1] ^ np.uint32(1)
    rejected(bad)


def test_geometry_rules():
    c, m = _case("pad_mod4")
    ok = dict(n_prod=c.n_prod, prod_waves=c.prod_waves, n_sub=c.n_sub, cap_w=c.cap_w, pool=c.pool, wave_cnt=c.wave_cnt, n_bins=c.n_bins,
              bin_shift=c.bin_shift, out_words=m.total)
    assert PC.geometry_error(**ok) is None
    over = c.wave_cnt.copy(); over[2] = c.cap_w + 1
    far = c.pool.copy(); far[0] = (c.n_bins << c.bin_shift) | 5
    for change in (dict(cap_w=24), dict(wave_cnt=over), dict(prod_waves=17), dict(n_sub=9), dict(bin_shift=15), dict(bin_shift=26),
                   dict(n_bins=PC.BIN_MAX + 1), dict(pool=far), dict(out_words=m.total - 1), dict(out_align=16), dict(n_prod=0), dict(n_bins=0),
                   dict(prod_waves=0), dict(n_sub=0), dict(pool=None)):
        assert PC.geometry_error(**{**ok, **change}) is not None, list(change)
    assert PC.geometry_error(**{**ok, "n_bins": PC.BIN_MAX}) is None
