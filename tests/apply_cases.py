"""Hand-made record streams for the second half of the binned update path -- k_regroup, k_tile_bases, k_sort_tiles, k_apply_tiles<WIDE, 0>,
k_part2, k_apply, k_apply_bigrecs -- as lime_apply_records_dev (include/lime_hip.h) takes them, and a numpy model of the block they build.
tests/test_apply_cases_cpu.py shows without a GPU that every case holds the edge it is named for, tests/test_apply_edges_gpu.py runs them
through every path.  Everything is seeded, pure numpy.

Why the shapes are under control.  k_regroup lays a bin's sources one after the other, in source order; k_sort_tiles takes records
[8192 k, 8192 (k + 1)) of that stream as tile k of the bin and sorts it by 64 KB region (the order inside a run is whatever the lanes make it); so a region's run in a tile has as many
records as the tile holds of that region and starts at the sum of the lower regions' counts in that tile.  A case is therefore described
per bin as a list of TILES, a tile as a map region-of-the-bin -> (run length, how its cells are chosen):

    {3: (257, None), 4: (5, 0x1234), 7: (n, offsets), "pad": 100, "pad_first": 2, "pad_last": 2}

None: seeded random cells inside the region; an int: that offset inside the region for all of them; an array: those offsets.  "pad": words
with a zero t field ("no record": include/lime_hip.h) shuffled among the records, "pad_first" / "pad_last": at the tile's borders.  Every
tile of a bin but its last holds exactly PART_TILE words.  The contract for 32-bit records is t == 1; the builder writes nothing else."""
import numpy as np

# lime_amd/csrc/lime_kernels.h
PART_TILE = 8192                  # records per tile of k_sort_tiles (PART_WG * PART_PER)
REGION_SHIFT = 16                 # k_apply / k_apply_tiles build 64 KB of the table per workgroup pass
BIN_MAX = 3072                    # bins of a block (k_tile_bases' LDS counters)
BIN_SHIFT_MAX = 25                # offset inside the bin + 7 bits of t fill 32 bits
CELL_BITS = 40                    # 64-bit record: cell | t << CELL_BITS
APPLY_READ = 2048                 # k_apply: APPLY_WG * 4 records per round
BIG_GRID_THREADS = 4096 * 256     # k_apply_bigrecs' largest grid
GAP_WORD = 0xFFFFFFFF             # what lies in d_rx between the sources' slices: a record (t != 0) if anything read it
RMASK = (1 << REGION_SHIFT) - 1


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_records(self):
        return int((self.srcoff[:, -1] - self.srcoff[:, 0]).sum())


def _tile_words(tile, bin_shift, rng):
    parts = []
    for r in sorted(k for k in tile if not isinstance(k, str)):
        n, how = tile[r]
        if how is None:
            off = rng.integers(0, 1 << REGION_SHIFT, n, dtype=np.int64)
        elif isinstance(how, np.ndarray):
            off = how.astype(np.int64)
            assert len(off) == n
        else:
            off = np.full(n, int(how), dtype=np.int64)
        assert 0 <= r < (1 << (bin_shift - REGION_SHIFT)) and (n == 0 or (off.min() >= 0 and off.max() <= RMASK))
        parts.append(((r << REGION_SHIFT) | off) | (1 << bin_shift))
    pads = lambda n: rng.integers(0, 1 << bin_shift, n, dtype=np.int64)          # t == 0, the other bits anything
    body = np.concatenate(parts + [pads(tile.get("pad", 0))]) if parts or tile.get("pad", 0) else np.zeros(0, np.int64)
    rng.shuffle(body)
    return np.concatenate([pads(tile.get("pad_first", 0)), body, pads(tile.get("pad_last", 0))]).astype(np.uint32)


def build(name, bin_shift, bins, n_src=1, cuts=None, gap=0, bigrecs=None, cell_lo=0, block_bytes=None, seed=1, facts=None):
    """bins[b]: the tiles of bin b.  cuts: None -- every bin's stream is cut at n_src - 1 seeded random positions; or cuts[b]: the slice
    sizes of sources 0 .. n_src - 2 (the last source gets the rest).  gap: GAP_WORDs in rx in front of every source's slices and behind the last."""
    rng = np.random.default_rng(seed)
    nb = len(bins)
    streams = []
    for b, tiles in enumerate(bins):
        words = [_tile_words(t, bin_shift, rng) for t in tiles]
        for k, w in enumerate(words):
            assert 1 <= len(w) <= PART_TILE and (k == len(words) - 1 or len(w) == PART_TILE), (name, b, k, len(w))
        streams.append(np.concatenate(words) if words else np.zeros(0, np.uint32))
    slices = []                                                                    # slices[b][s]
    for b, st in enumerate(streams):
        if cuts is None:
            at = np.sort(rng.integers(0, len(st) + 1, n_src - 1))
        else:
            at = np.cumsum(np.asarray(cuts[b], dtype=np.int64))
            assert len(at) == n_src - 1 and (len(at) == 0 or at[-1] <= len(st)), (name, b)
        edges = np.concatenate([[0], at, [len(st)]]).astype(np.int64)
        slices.append([st[edges[s]:edges[s + 1]] for s in range(n_src)])
    srcoff = np.zeros((n_src, nb + 1), dtype=np.uint64)
    out, at = [], 0
    for s in range(n_src):
        out.append(np.full(gap, GAP_WORD, dtype=np.uint32)); at += gap
        for b in range(nb):
            srcoff[s, b] = at
            out.append(slices[b][s]); at += len(slices[b][s])
        srcoff[s, nb] = at
    out.append(np.full(gap, GAP_WORD, dtype=np.uint32))
    rx = np.concatenate(out)
    big = np.zeros(0, np.uint64) if bigrecs is None else np.ascontiguousarray(bigrecs, dtype=np.uint64)
    return Case(name=name, rx=rx, srcoff=srcoff, nb=nb, bin_shift=bin_shift, n_src=n_src, bigrecs=big, cell_lo=int(cell_lo),
                block_bytes=int((nb << bin_shift) if block_bytes is None else block_bytes), facts=dict(facts or {}))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def bin_streams(case):
    """k_regroup in numpy: every bin's records, the sources' slices one after the other in source order"""
    so = case.srcoff.astype(np.int64)
    return [np.concatenate([case.rx[so[s, b]:so[s, b + 1]] for s in range(case.n_src)]) for b in range(case.nb)]


def model(case):
    """the block lime_apply_records_dev must build: every 32-bit word of bin b with a non-zero t field adds 1 modulo 256 at
    (b << bin_shift) + (word & mask) if that is below block_bytes; every 64-bit record whose cell lies in [cell_lo, cell_lo + block_bytes)
    adds its t modulo 256 at cell - cell_lo"""
    block = np.zeros(case.block_bytes, dtype=np.uint8)
    width, sh = 1 << case.bin_shift, case.bin_shift
    for b, st in enumerate(bin_streams(case)):
        lo = b << sh
        room = min(width, case.block_bytes - lo)
        if room <= 0 or not len(st):
            continue
        off = (st[(st >> np.uint32(sh)) != 0] & np.uint32(width - 1)).astype(np.int64)
        block[lo:lo + room] = np.bincount(off[off < room], minlength=room).astype(np.uint8)          # (astype wraps modulo 256)
    if len(case.bigrecs):
        cell = (case.bigrecs & np.uint64((1 << CELL_BITS) - 1)).astype(np.int64)
        t = (case.bigrecs >> np.uint64(CELL_BITS)).astype(np.int64)
        own = (cell >= case.cell_lo) & (cell < case.cell_lo + case.block_bytes)
        at = cell[own] - case.cell_lo
        span = np.unique(at)
        add = np.bincount(np.searchsorted(span, at), weights=t[own].astype(np.float64), minlength=len(span)).astype(np.int64)       # (sums far below 2^53)
        block[span] = ((block[span].astype(np.int64) + add) & 255).astype(np.uint8)
    return block


def model_naive(case):
    """the same, record by record"""
    block = [0] * case.block_bytes
    so = case.srcoff
    mask = (1 << case.bin_shift) - 1
    for b in range(case.nb):
        for s in range(case.n_src):
            for w in case.rx[int(so[s, b]):int(so[s, b + 1])].tolist():
                if w >> case.bin_shift:
                    c = (b << case.bin_shift) + (w & mask)
                    if c < case.block_bytes:
                        block[c] = (block[c] + 1) & 255
    for r in case.bigrecs.tolist():
        c, t = r & ((1 << CELL_BITS) - 1), r >> CELL_BITS
        if case.cell_lo <= c < case.cell_lo + case.block_bytes:
            block[c - case.cell_lo] = (block[c - case.cell_lo] + t) & 255
    return np.array(block, dtype=np.uint8)


def runs(case):
    """k_sort_tiles in numpy -> (tiles per bin, int64 [n, 5]: bin, tile of the bin, region of the bin, the run's length, its start in the tile),
    the non-empty runs only"""
    f2 = 1 << (case.bin_shift - REGION_SHIFT)
    tiles_per_bin, rows = [], []
    for b, st in enumerate(bin_streams(case)):
        nt = (len(st) + PART_TILE - 1) // PART_TILE
        tiles_per_bin.append(nt)
        for k in range(nt):
            w = st[k * PART_TILE:(k + 1) * PART_TILE]
            w = w[(w >> np.uint32(case.bin_shift)) != 0]
            cnt = np.bincount(((w & np.uint32((1 << case.bin_shift) - 1)) >> np.uint32(REGION_SHIFT)).astype(np.int64), minlength=f2)
            start = np.cumsum(cnt) - cnt
            nz = np.nonzero(cnt)[0]
            rows.append(np.stack([np.full(len(nz), b), np.full(len(nz), k), nz, cnt[nz], start[nz]], axis=1))
    return tiles_per_bin, (np.concatenate(rows) if rows else np.zeros((0, 5), np.int64)).astype(np.int64)


def geometry_error(n_src, nb, bin_shift, block_bytes, cell_lo, srcoff, block_align=0):
    """lime_apply_records_dev's argument rules (lime_pass.cpp): None, or what is refused"""
    if not n_src:
        return "n_src == 0"
    if bin_shift < REGION_SHIFT or bin_shift > BIN_SHIFT_MAX:
        return "bin_shift"
    if block_bytes & 15 or block_align & 15:
        return "block not in 16-byte units"
    if block_bytes > (nb << bin_shift):
        return "block beyond its bins"
    if cell_lo & ((1 << bin_shift) - 1):
        return "cell_lo not bin-aligned"
    if nb > BIN_MAX:
        return "nb > BIN_MAX"
    so = np.asarray(srcoff, dtype=np.uint64).reshape(n_src, nb + 1)
    if (so[:, 1:] < so[:, :-1]).any():
        return "source offsets descend"
    return None


# ---- pieces of cases ------------------------------------------------------------------------------------------------------------------
def pack_runs(pairs, f2, fill, first_region=0):
    """tiles that hold, for every (L, k) of pairs, a run of L records that starts at a position = k mod 4 of its tile: runs go to ascending regions,
    a run of 1 .. 3 records in a region of its own in front where the position has to be moved.  What a tile has left goes to pad words (fill
    "pad") or to a run in the bin's last region (fill "last").  L == 0 leaves a region empty; L == PART_TILE takes a whole tile (k == 0 only)."""
    top = f2 if fill == "pad" else f2 - 1
    tiles, state = [], {"cur": {}, "pos": 0, "r": first_region}

    def close():
        left = PART_TILE - state["pos"]
        if left:
            if fill == "pad":
                state["cur"]["pad"] = left
            else:
                state["cur"][f2 - 1] = (left, None)
        tiles.append(state["cur"])
        state.update(cur={}, pos=0, r=first_region)

    for L, k in pairs:
        assert 0 <= L <= PART_TILE and 0 <= k < 4 and (L < PART_TILE or k == 0) and L + k <= PART_TILE
        f = (k - state["pos"]) % 4
        if state["r"] + (2 if f else 1) > top or state["pos"] + f + L > PART_TILE:
            close()
            f = k
        if f:
            state["cur"][state["r"]] = (f, None); state["r"] += 1; state["pos"] += f
        if L:
            state["cur"][state["r"]] = (L, None)
        state["r"] += 1; state["pos"] += L
    if state["cur"] or state["pos"] == 0 and not tiles:
        close()
    return tiles


def spread_tile(rng, f2, n=PART_TILE, regions=None):
    """n records over the regions of a bin (all of them, or `regions`), multinomially"""
    regs = np.arange(f2) if regions is None else np.asarray(regions)
    cnt = rng.multinomial(n, np.full(len(regs), 1.0 / len(regs)))
    return {int(r): (int(c), None) for r, c in zip(regs, cnt) if c}


RUN_LENGTHS = [0, 1, 2, 3, 4, 5] + list(range(253, 261)) + list(range(316, 325)) + list(range(509, 517)) + list(range(1020, 1029))
RUN_PAIRS = [(L, k) for L in RUN_LENGTHS for k in range(4)] + [(PART_TILE, 0)]


def _with_runs(name, bin_shift, copies, fill, seed):
    """RUN_PAIRS `copies` times, each copy in another order, in one bin; a second bin of one short tile"""
    rng = np.random.default_rng(seed)
    f2 = 1 << (bin_shift - REGION_SHIFT)
    tiles = []
    for _ in range(copies):
        tiles += pack_runs([RUN_PAIRS[i] for i in rng.permutation(len(RUN_PAIRS))], f2, fill)
    return build(name, bin_shift, [tiles, [spread_tile(rng, f2, 1000)]], n_src=3, seed=seed,
                 facts={"tiles": [len(tiles), 1], "runs": {(L, k) for L, k in RUN_PAIRS if L}})


def run_lengths_2():
    """2 regions per bin: a wave per run; a run's tile holds little else (pad words fill it)"""
    return _with_runs("run_lengths_2", 17, 1, "pad", 11)


def run_lengths_32():
    """32 regions per bin, the N = 1e10 series' shape: a wave per run, five to six runs a wave"""
    return _with_runs("run_lengths_32", 21, 4, "last", 12)


def default_group(f2):
    """k_apply_tiles: lanes per run as a power of two, by the regions per bin"""
    return 2 if f2 >= 512 else 3 if f2 == 256 else 4 if f2 == 128 else 5 if f2 == 64 else 6


def grouped(f2):
    """f2 = 64 .. 512 regions per bin: 2^lg lanes share a run and take 8 << lg of its records per pass, 64 >> lg runs an instruction.  Runs of one
    record less, exactly, one more than a pass and of two passes and three, at every start mod 4; 8 * ((64 >> lg) + 1) tiles: every wave gets one run
    more than a multiple of 64 >> lg"""
    lg = default_group(f2)
    bin_shift = REGION_SHIFT + int(np.log2(f2))
    step = 8 << lg
    lens = [step - 1, step, step + 1, 2 * step + 3]
    pairs = [(L, k) for L in lens for k in range(4)]
    rpi = 64 >> lg
    n_tiles = 8 * (rpi + 1)
    rng = np.random.default_rng(100 + f2)
    tiles = []
    for t in range(n_tiles):
        order = [pairs[i] for i in rng.permutation(len(pairs))]
        got = pack_runs(order, f2, "last", first_region=int(rng.integers(0, f2 - 2 * len(pairs) - 1)))
        assert len(got) == 1
        tiles += got
    return build(f"grouped_{f2}", bin_shift, [tiles], n_src=2, seed=100 + f2,
                 facts={"tiles": [n_tiles], "runs": set(pairs), "runs_per_wave_not_multiple_of": rpi})


TILE_COUNTS = [1, 8, 9, 255, 256, 257, 307, 511, 512, 513, 1025]


def tiles(n):
    """a bin of n tiles at 32 regions per bin (33 .. 63 runs per wave, a last step of fewer than four runs, a second and third round of 512 tiles);
    n == 1: a bin of exactly 8192 records; n == 257 and n == 1025: the last tile holds ONE record.  A second bin of one short tile behind it."""
    rng = np.random.default_rng(1000 + n)
    f2, bin_shift = 32, 21
    last = PART_TILE if n == 1 else 1 if n in (257, 1025) else int(rng.integers(2, PART_TILE))
    t = [spread_tile(rng, f2) for _ in range(n - 1)] + [spread_tile(rng, f2, last)]
    return build(f"tiles_{n}", bin_shift, [t, [spread_tile(rng, f2, 777)]], n_src=2, seed=1000 + n,
                 facts={"tiles": [n, 1], "last_tile_records": last})


def empty_bins():
    """empty bins first, between full ones and last"""
    rng = np.random.default_rng(21)
    full = lambda k: [spread_tile(rng, 4) for _ in range(k)] + [spread_tile(rng, 4, 333)]
    bins = [[], full(1), [], [], full(0), full(2), []]
    return build("empty_bins", 18, bins, n_src=2, seed=21, facts={"tiles": [0, 2, 0, 0, 1, 3, 0]})


def _big(cell, t):
    return np.asarray(cell, dtype=np.uint64) | (np.asarray(t, dtype=np.uint64) << np.uint64(CELL_BITS))


def no_records(with_big):
    """no 32-bit record at all: every byte of the block is still written"""
    big = _big([5, 70000, 70000, 3 * 131072 - 1, 3 * 131072], [7, 200, 100, 255, 9]) if with_big else None
    return build("no_records_big" if with_big else "no_records", 17, [[], [], []], n_src=2, bigrecs=big, facts={"tiles": [0, 0, 0]})


CELL_SUMS = [255, 256, 257, 511, 512]


def cell_sums():
    """sums of 255 .. 512 in one cell, and for every byte position of a word the other three cells at 255 while this one gets its 256th record: the
    fast adds (one LDS add per record on the cell's word) carry into the neighbour there, which the exact rebuild must undo.  Region 0: everything
    in one tile; region 1: the same cells, their records spread over three tiles (three waves)."""
    rng = np.random.default_rng(31)
    off, want = [], {}
    for i, s in enumerate(CELL_SUMS):
        off += [1000 + 8 * i] * s; want[1000 + 8 * i] = s & 255
    for p in range(4):
        for q in range(4):
            c = 2000 + 4 * p + q
            off += [c] * (256 if q == p else 255); want[c] = 0 if q == p else 255
    off = rng.permutation(np.array(off))
    third = [off[k::3] for k in range(3)]
    t0 = {0: (len(off), off), 1: (len(third[0]), third[0]), 3: (50, None)}
    t0["pad"] = PART_TILE - sum(v[0] for v in t0.values())
    t1 = {1: (len(third[1]), third[1]), 2: (100, None)}
    t1["pad"] = PART_TILE - sum(v[0] for v in t1.values())
    t2 = {1: (len(third[2]), third[2])}
    return build("cell_sums", 18, [[t0, t1, t2], [spread_tile(rng, 4, 500)]], n_src=2, seed=31,
                 facts={"tiles": [3, 1], "cells": {(r << REGION_SHIFT) + c: v for r in (0, 1) for c, v in want.items()}})


def wrap_alternate():
    """1536 regions, three bins of 512: more regions than workgroups fit the device, so every workgroup walks several.  Every odd region holds a
    cell of 300 records (the region is rebuilt with the exact adds), every even region a cell of 240 and no wrap: the exact-rebuild flag and the
    cleared LDS copy must carry nothing from a region to the next.  20 tiles per bin, each with 15 / 12 of the cell's records and a random one."""
    rng = np.random.default_rng(41)
    f2 = 512
    bins, cells = [], {}
    for b in range(3):
        fixed = rng.integers(0, 1 << REGION_SHIFT, f2)
        t = []
        for _ in range(20):
            tile = {}
            for r in range(f2):
                n = 15 if r & 1 else 12
                tile[r] = (n + 1, np.concatenate([np.full(n, fixed[r]), rng.integers(0, 1 << REGION_SHIFT, 1)]))
            tile["pad"] = PART_TILE - sum(v[0] for v in tile.values())
            t.append(tile)
        bins.append(t)
        for r in range(f2):
            cells[(b << 25) + (r << REGION_SHIFT) + int(fixed[r])] = r & 1
    return build("wrap_alternate", 25, bins, n_src=2, seed=41, facts={"tiles": [20, 20, 20], "wraps": cells})


def block_tail(bin_shift):
    """block_bytes a multiple of 16 and not of 64 KB: the last region is cut after 1040 bytes, and records are addressed into what is cut off (they
    touch the region's LDS copy only) and into the region behind it"""
    rng = np.random.default_rng(51 + bin_shift)
    f2 = 1 << (bin_shift - REGION_SHIFT)
    nb = 6 // f2 if f2 <= 2 else 2
    n_reg = nb * f2
    cut = n_reg - 2                                                      # the region that is cut; one more lies behind it
    bins = []
    for b in range(nb):
        tile = spread_tile(rng, f2, 3000)
        for r in range(f2):
            if b * f2 + r == cut:
                tile[r] = (600, np.concatenate([rng.integers(0, 1040, 300), rng.integers(1040, 1 << REGION_SHIFT, 298), [1039, 1040]]))
        bins.append([tile])
    return build(f"block_tail_{bin_shift}", bin_shift, bins, n_src=2, seed=51, block_bytes=(cut << REGION_SHIFT) + 1040,
                 facts={"tiles": [1] * nb, "cut_region": cut})


def block_short():
    """the block ends three whole regions before nb << bin_shift: the records of those regions change nothing"""
    rng = np.random.default_rng(61)
    bins = [[spread_tile(rng, 4), spread_tile(rng, 4, 4000)] for _ in range(3)]
    return build("block_short", 18, bins, n_src=3, seed=61, block_bytes=9 << REGION_SHIFT, facts={"tiles": [2, 2, 2]})


def padding():
    """words with a zero t field: scattered inside tiles, at the tiles' borders, as a whole tile, as a bin's last tile and as a whole bin"""
    rng = np.random.default_rng(71)
    scattered = dict(spread_tile(rng, 4, 5000), pad=PART_TILE - 5000)
    borders = dict(spread_tile(rng, 4, PART_TILE - 7), pad_first=3, pad_last=4)
    whole = {"pad": PART_TILE}
    bins = [[scattered, whole, borders, dict(spread_tile(rng, 4, 100), pad_first=1)],
            [borders, {"pad": 17}],
            [{"pad": 300}],
            [spread_tile(rng, 4, 64)]]
    return build("padding", 18, bins, n_src=2, seed=71, facts={"tiles": [4, 2, 1, 1]})


PER_REGION = [0, 1, APPLY_READ - 1, APPLY_READ, APPLY_READ + 1, 2 * APPLY_READ + 1]


def per_region(bin_shift):
    """records per region on both sides of the 2048 k_apply reads per round.  bin_shift 16: the bins are the regions (one level); 18: the regions
    of two bins, for k_part2 + k_apply"""
    f2 = 1 << (bin_shift - REGION_SHIFT)
    counts = PER_REGION + [3, 0][:(-len(PER_REGION)) % f2]
    bins = [[{r: (counts[b * f2 + r], None) for r in range(f2) if counts[b * f2 + r]}] for b in range(len(counts) // f2)]
    bins = [[t for t in tl if t] for tl in bins]
    return build(f"per_region_{bin_shift}", bin_shift, bins, n_src=2, seed=81, facts={"per_region": counts})


def part2_align():
    """k_part2's first sweep reads aligned groups of four records: bins that start and end at 1, 2, 3 mod 4 of the regrouped array"""
    rng = np.random.default_rng(91)
    sizes = [1, 1, 1, 5, 6, PART_TILE + 3, 2, 4, 7]                      # starts 0 1 2 3 0 2 1 3 3, ends 1 2 3 0 2 1 3 3 2 (mod 4)
    bins = []
    for n in sizes:
        bins.append([spread_tile(rng, 2, min(n, PART_TILE))] + ([spread_tile(rng, 2, n - PART_TILE)] if n > PART_TILE else []))
    return build("part2_align", 17, bins, n_src=1, seed=91, facts={"bin_sizes": sizes})


def regroup(n_src):
    """n_src sources with slices of 0, 1, 255, 256 and 257 records (k_regroup copies 256 a round), sources that are empty for some bins or for
    all of them, and three words between the sources' slices in d_rx that belong to nobody"""
    rng = np.random.default_rng(200 + n_src)
    nb = 6
    special = [0, 1, 255, 256, 257]
    cuts, bins = [], []
    for b in range(nb):
        if n_src == 1:
            sl, total = [], [0, 1, 255, 256, 257, 300][b]
        else:
            sl = [special[(s + b) % 5] if s % 2 == 0 or n_src <= 2 else 0 for s in range(n_src - 1)]
            if n_src >= 7:
                sl[3] = 0                                                # source 3 is empty for every bin
                if b == 2:
                    sl = [0] * (n_src - 1)                               # bin 2: everything from the last source
            total = sum(sl) + [0, 1, 255, 256, 257, PART_TILE + 5][b]
        cuts.append(sl)
        t = [spread_tile(rng, 2) for _ in range(total // PART_TILE)] + ([spread_tile(rng, 2, total % PART_TILE)] if total % PART_TILE else [])
        bins.append(t)
    return build(f"regroup_{n_src}", 17, bins, n_src=n_src, cuts=cuts, gap=3, seed=200 + n_src, facts={"slices": set(special), "gap": 3})


def big_edges():
    """long-cluster records at the block's four borders, every t of 1 .. 255, several to one cell, and on a cell that the 32-bit records wrap;
    cell_lo = 5 << 32"""
    rng = np.random.default_rng(301)
    cell_lo, bb = 5 << 32, 2 << 17
    tile = spread_tile(rng, 2, 2000)
    tile[1] = (300, 4321)                                                 # 300 records on one cell: 44
    wrapped = (1 << REGION_SHIFT) + 4321
    cells = [cell_lo - 1, cell_lo, cell_lo + bb - 1, cell_lo + bb] + [cell_lo + 100 + t for t in range(1, 256)] + \
            [cell_lo + 9000] * 5 + [cell_lo + wrapped] * 3 + [5, bb + 5, (5 << 32) - (1 << 17) + 7, (6 << 32) + 7]
    ts = [11, 12, 13, 14] + list(range(1, 256)) + [255, 255, 255, 3, 200] + [250, 250, 250] + [1, 2, 3, 4]
    return build("big_edges", 17, [[tile], [spread_tile(rng, 2, 100)]], n_src=2, seed=301, bigrecs=_big(cells, ts), cell_lo=cell_lo,
                 facts={"tiles": [1, 1], "cells": {0: 12, bb - 1: 13, 9000: (255 * 3 + 203) & 255, wrapped: (300 + 750) & 255}})


def big_many():
    """2^20 + 300 long-cluster records: more than k_apply_bigrecs' grid of 4096 x 256 threads, half of them outside the block"""
    rng = np.random.default_rng(302)
    n = (1 << 20) + 300
    cell_lo, bb = 3 << 18, 2 << 18
    cells = rng.integers(0, cell_lo + 2 * bb, n)
    cells[-300:] = cell_lo + rng.integers(0, 64, 300)                      # the records beyond the grid: all on 64 cells
    return build("big_many", 18, [[spread_tile(rng, 4, 3000)], []], n_src=1, seed=302, bigrecs=_big(cells, rng.integers(1, 256, n)), cell_lo=cell_lo,
                 block_bytes=bb, facts={"tiles": [1, 0], "n_big": n})


# name -> (bin_shift, generator): the GPU tests choose the paths by bin_shift without building anything
CASES = {
    "run_lengths_2": (17, run_lengths_2), "run_lengths_32": (21, run_lengths_32),
    **{f"grouped_{f2}": (REGION_SHIFT + f2.bit_length() - 1, (lambda f2=f2: grouped(f2))) for f2 in (64, 128, 256, 512)},
    **{f"tiles_{n}": (21, (lambda n=n: tiles(n))) for n in TILE_COUNTS},
    "empty_bins": (18, empty_bins), "no_records": (17, lambda: no_records(False)), "no_records_big": (17, lambda: no_records(True)),
    "cell_sums": (18, cell_sums), "wrap_alternate": (25, wrap_alternate),
    "block_tail_16": (16, lambda: block_tail(16)), "block_tail_17": (17, lambda: block_tail(17)), "block_tail_19": (19, lambda: block_tail(19)),
    "block_short": (18, block_short), "padding": (18, padding),
    "per_region_16": (16, lambda: per_region(16)), "per_region_18": (18, lambda: per_region(18)), "part2_align": (17, part2_align),
    **{f"regroup_{s}": (17, (lambda s=s: regroup(s))) for s in (1, 2, 7, 64)},
    "big_edges": (17, big_edges), "big_many": (18, big_many),
}
GROUPED = ["run_lengths_32", "grouped_64", "grouped_128", "grouped_256", "grouped_512"]     # the streams that also run with apply_group 1 .. 6


def make(name):
    case = CASES[name][1]()
    assert case.name == name and case.bin_shift == CASES[name][0]
    for a in (case.rx, case.srcoff, case.bigrecs):
        a.setflags(write=False)
    return case
