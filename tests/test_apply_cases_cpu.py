"""tests/apply_cases.py without a GPU: the model against a record-by-record loop, the builder against a numpy restatement of k_regroup and
k_sort_tiles (every named case holds the edge it is named for, so that tests/test_apply_edges_gpu.py cannot lose one quietly when the builder
changes), and every case against lime_apply_records_dev's argument rules."""
import functools

import numpy as np
import pytest

from tests import apply_cases as AC


@functools.lru_cache(maxsize=2)
def _case(name):
    return AC.make(name)


@functools.lru_cache(maxsize=2)
def _runs(name):
    return AC.runs(_case(name))


@pytest.mark.parametrize("name", list(AC.CASES))
def test_case_obeys_the_entry_points_rules(name):
    c = _case(name)
    assert AC.geometry_error(c.n_src, c.nb, c.bin_shift, c.block_bytes, c.cell_lo, c.srcoff) is None
    assert c.srcoff.shape == (c.n_src, c.nb + 1) and int(c.srcoff.max()) <= len(c.rx)
    # every record's t field is 1 or 0, and k_sort_tiles' 16-bit record is the whole offset inside the region
    inside = np.zeros(len(c.rx), dtype=bool)
    for s in range(c.n_src):
        inside[int(c.srcoff[s, 0]):int(c.srcoff[s, -1])] = True
    assert set(np.unique(c.rx[inside] >> np.uint32(c.bin_shift)).tolist()) <= {0, 1}
    assert (c.rx[~inside] == AC.GAP_WORD).all()
    assert c.n_records == int(inside.sum()) <= 1025 * AC.PART_TILE and c.block_bytes <= 96 << 20
    _, r = _runs(name)
    assert len(r) == 0 or (r[:, 4] + r[:, 3]).max() <= AC.PART_TILE
    if len(c.bigrecs):
        assert int((c.bigrecs >> np.uint64(AC.CELL_BITS)).max()) <= 255 and int((c.bigrecs >> np.uint64(AC.CELL_BITS)).min()) >= 1


LARGE = ["run_lengths_2", "run_lengths_32", "grouped_64", "grouped_128", "grouped_256", "grouped_512", "wrap_alternate", "big_many"] + \
        [f"tiles_{n}" for n in AC.TILE_COUNTS if n > 9]


@pytest.mark.parametrize("name", [n for n in AC.CASES if n not in LARGE])
def test_model_equals_a_loop_over_the_records(name):
    c = _case(name)
    assert np.array_equal(AC.model(c), AC.model_naive(c))


@pytest.mark.parametrize("name", LARGE)
def test_the_cases_without_the_loop_are_the_large_ones(name):
    c = _case(name)
    assert c.n_records + len(c.bigrecs) >= 100_000


@pytest.mark.parametrize("name", [n for n in AC.CASES if n not in ("per_region_16", "per_region_18", "part2_align") and not n.startswith("regroup_")])
def test_tiles_per_bin(name):
    tiles_per_bin, _ = _runs(name)
    assert tiles_per_bin == _case(name).facts["tiles"]


@pytest.mark.parametrize("name", ["run_lengths_2", "run_lengths_32", "grouped_64", "grouped_128", "grouped_256", "grouped_512"])
def test_runs_of_every_named_length_at_every_start(name):
    c = _case(name)
    _, r = _runs(name)
    have = set(zip(r[:, 3].tolist(), (r[:, 4] & 3).tolist()))
    assert c.facts["runs"] <= have, sorted(c.facts["runs"] - have)
    f2 = 1 << (c.bin_shift - AC.REGION_SHIFT)
    if name.startswith("run_lengths"):
        assert {(L, k) for L in AC.RUN_LENGTHS if L for k in range(4)} | {(AC.PART_TILE, 0)} == c.facts["runs"]
        # an empty region between two that are not, in a tile (the run of length 0)
        t0 = r[(r[:, 0] == 0) & (r[:, 1] == 0)][:, 2]
        assert f2 == 2 or (np.diff(t0) > 1).any()
    else:
        lg = AC.default_group(f2)
        assert {L for L, _ in c.facts["runs"]} == {(8 << lg) - 1, 8 << lg, (8 << lg) + 1, 2 * (8 << lg) + 3}
        rpi = c.facts["runs_per_wave_not_multiple_of"]
        assert rpi == 64 >> lg
        for wave in range(8):                                             # k_apply_tiles: wave w takes the tiles w, w + 8, ... of the bin
            assert len(range(wave, c.facts["tiles"][0], 8)) % rpi != 0
        assert (r[:, 3] > 4 * (8 << lg)).any()                            # and a run of many passes


def test_tile_counts_and_last_tiles():
    assert AC.TILE_COUNTS == [1, 8, 9, 255, 256, 257, 307, 511, 512, 513, 1025]
    for n in (1, 257, 1025):                                              # the rest: test_tiles_per_bin
        c = _case(f"tiles_{n}")
        st = AC.bin_streams(c)[0]
        assert len(st) == (n - 1) * AC.PART_TILE + (AC.PART_TILE if n == 1 else 1)
    _, r = _runs("tiles_307")
    per_tile = np.bincount(r[r[:, 0] == 0][:, 1])
    assert (per_tile[:-1] == 32).all()                                    # every region has a run in every full tile


def test_cell_sums():
    c = _case("cell_sums")
    m = AC.model(c)
    for cell, v in c.facts["cells"].items():
        assert m[cell] == v, cell
    assert sorted({v for v in c.facts["cells"].values()}) == [0, 1, 255]
    st = AC.bin_streams(c)[0]
    cells = np.bincount((st[(st >> np.uint32(18)) != 0] & np.uint32((1 << 18) - 1)).astype(np.int64))
    assert set(AC.CELL_SUMS) <= set(cells.tolist())
    for region in (0, 1):
        for p in range(4):                                                # byte p of the word gets 256, the other three 255
            w = cells[(region << 16) + 2000 + 4 * p:(region << 16) + 2004 + 4 * p].tolist()
            assert w == [256 if q == p else 255 for q in range(4)]
    _, r = _runs("cell_sums")
    assert set(r[(r[:, 0] == 0) & (r[:, 2] == 1)][:, 1].tolist()) == {0, 1, 2}            # region 1's records come from three tiles


def test_wrap_alternate():
    c = _case("wrap_alternate")
    assert c.block_bytes == 1536 << 16 == 96 << 20 and c.nb == 3
    st = AC.bin_streams(c)
    for b in range(3):
        w = st[b][(st[b] >> np.uint32(25)) != 0] & np.uint32((1 << 25) - 1)
        top = np.bincount(w.astype(np.int64), minlength=1 << 25).reshape(512, 1 << 16).max(axis=1)
        assert (top[1::2] >= 300).all() and (top[0::2] < 255).all() and (top[0::2] >= 240).all()


def test_block_ends():
    for sh in (16, 17, 19):
        c = _case(f"block_tail_{sh}")
        assert c.block_bytes % 16 == 0 and c.block_bytes % 65536 == 1040
        _, r = _runs(c.name)
        f2 = 1 << (sh - 16)
        region = r[:, 0] * f2 + r[:, 2]
        cut = c.facts["cut_region"]
        assert cut == c.block_bytes >> 16 and (region == cut).any() and (region == cut + 1).any()
        b, sub = divmod(cut, f2)
        st = AC.bin_streams(c)[b]
        off = st[((st & np.uint32((1 << sh) - 1)) >> np.uint32(16)) == sub] & np.uint32(0xFFFF)
        assert (off < 1040).any() and (off >= 1040).any() and 1039 in off and 1040 in off and off.max() > 60000
    c = _case("block_short")
    assert c.block_bytes == 9 << 16 and (c.nb << c.bin_shift) == 12 << 16
    _, r = _runs("block_short")
    assert set((r[:, 0] * 4 + r[:, 2]).tolist()) == set(range(12))


def test_padding():
    c = _case("padding")
    st = AC.bin_streams(c)
    z = [(s >> np.uint32(c.bin_shift)) == 0 for s in st]
    t = AC.PART_TILE
    assert z[0][:t].sum() == t - 5000 and z[0][:t // 2].any() and z[0][t // 2:t].any()    # scattered
    assert z[0][t:2 * t].all()                                                            # a whole tile
    assert z[0][2 * t:2 * t + 3].all() and z[0][3 * t - 4:3 * t].all() and z[0][3 * t]     # at tile borders, on both sides
    assert not z[0][2 * t + 3:3 * t - 4].any()
    assert z[1][t:].all() and len(st[1]) == t + 17                                        # a bin's last tile
    assert z[2].all() and len(st[2]) == 300                                               # a whole bin
    assert (st[0][z[0]] != 0).any()                                                       # the no-record words are not all-zero words


def test_per_region_and_part2_alignment():
    for sh in (16, 18):
        c = _case(f"per_region_{sh}")
        f2 = 1 << (sh - 16)
        _, r = _runs(c.name)
        got = np.zeros(c.nb * f2, dtype=np.int64)
        np.add.at(got, r[:, 0] * f2 + r[:, 2], r[:, 3])
        assert got.tolist() == c.facts["per_region"] and set([0, 1, 2047, 2048, 2049]) <= set(got.tolist())
    c = _case("part2_align")
    base = np.concatenate([[0], np.cumsum([len(s) for s in AC.bin_streams(c)])])
    assert np.diff(base).tolist() == c.facts["bin_sizes"]
    assert {1, 2, 3} <= set((base[:-1] & 3).tolist()) and {1, 2, 3} <= set((base[1:] & 3).tolist())
    assert any(a & 3 and e & 3 and e - a > AC.PART_TILE for a, e in zip(base[:-1], base[1:]))


@pytest.mark.parametrize("n_src", [1, 2, 7, 64])
def test_regroup_slices(n_src):
    c = _case(f"regroup_{n_src}")
    assert c.n_src == n_src
    size = (c.srcoff[:, 1:] - c.srcoff[:, :-1]).astype(np.int64)
    if n_src == 1:
        assert set(size[0].tolist()) >= {0, 1, 255, 256, 257}
    else:
        assert set(size[:-1].ravel().tolist()) >= c.facts["slices"]
    if n_src >= 7:
        assert (size[3] == 0).all() and (size[:, 2] == 0).sum() == n_src - 1               # an empty source; a bin that one source fills alone
        assert ((size == 0).any(axis=1) & (size > 0).any(axis=1)).any()
    # three foreign words in front of every source and behind the last
    assert int(c.srcoff[0, 0]) == 3 and len(c.rx) == int(c.srcoff[-1, -1]) + 3
    for s in range(1, n_src):
        assert int(c.srcoff[s, 0]) - int(c.srcoff[s - 1, -1]) == 3


def test_long_cluster_records():
    c = _case("big_edges")
    cell = (c.bigrecs & np.uint64((1 << AC.CELL_BITS) - 1)).astype(np.int64)
    t = (c.bigrecs >> np.uint64(AC.CELL_BITS)).astype(np.int64)
    assert c.cell_lo == 5 << 32 and c.cell_lo % (1 << c.bin_shift) == 0
    for edge in (c.cell_lo - 1, c.cell_lo, c.cell_lo + c.block_bytes - 1, c.cell_lo + c.block_bytes):
        assert edge in cell
    assert set(range(1, 256)) <= set(t.tolist())
    m = AC.model(c).astype(np.int64)
    only32 = AC.model(AC.Case(**{**c.__dict__, "bigrecs": np.zeros(0, np.uint64)})).astype(np.int64)
    wrapped = (1 << 16) + 4321
    assert only32[wrapped] == 300 - 256 and m[wrapped] == (300 + 750) & 255
    assert m[0] == (only32[0] + 12) & 255 and m[-1] == (only32[-1] + 13) & 255 and m[9000] == (only32[9000] + 968) & 255
    for k in range(1, 256):
        assert m[100 + k] == (only32[100 + k] + k) & 255
    c = _case("big_many")
    assert len(c.bigrecs) == (1 << 20) + 300 > AC.BIG_GRID_THREADS
    cell = (c.bigrecs & np.uint64((1 << AC.CELL_BITS) - 1)).astype(np.int64)
    own = (cell >= c.cell_lo) & (cell < c.cell_lo + c.block_bytes)
    assert own[-300:].all() and 0.2 < own.mean() < 0.8


def test_geometry_rules():
    ok = dict(n_src=1, nb=2, bin_shift=17, block_bytes=1 << 17, cell_lo=0, srcoff=[[0, 1, 2]])
    assert AC.geometry_error(**ok) is None
    for change in (dict(nb=AC.BIN_MAX + 1, srcoff=np.zeros((1, AC.BIN_MAX + 2))), dict(bin_shift=15), dict(bin_shift=26), dict(block_bytes=24),
                   dict(block_align=8), dict(block_bytes=(2 << 17) + 16), dict(cell_lo=1 << 16), dict(srcoff=[[0, 5, 3]]), dict(n_src=0)):
        assert AC.geometry_error(**{**ok, **change}) is not None, change
    assert AC.geometry_error(**{**ok, "nb": AC.BIN_MAX, "srcoff": np.zeros((1, AC.BIN_MAX + 1))}) is None
