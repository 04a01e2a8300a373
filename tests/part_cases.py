"""Hand-made record pools for the first-level partition of the binned update path -- k_bin_rowscan, k_bin_bases, then k_part or k_part_lines --
as lime_partition_records_dev (include/lime_hip.h) takes them, and a numpy model of the binned array they must leave.
tests/test_part_cases_cpu.py shows without a GPU that every case holds the edge it is named for, tests/test_part_edges_gpu.py runs them
through every path.  Everything is seeded, pure numpy.

Why the shapes are under control.  A producer's workgroup sees its prod_waves * n_sub pool segments -- (wave, sub-region), sub-region fastest --
one after the other, each padded to a multiple of four words, as ONE stream cut into tiles of PART_TILE words.  A case is therefore a list of
producers, a producer a list of segments, a segment a list of pieces laid out in this order:

    (bin, count, offsets)        offsets: None -- seeded random inside the bin; an int -- that offset for all; an array -- those offsets
    [piece, piece, ...]          the pieces' records shuffled together

so every segment count, every tile cut and every tile's records per bin are what the builder says.  The bins of sub-region s are
s << (32 - bin_shift) .. : a piece must sit in a segment of its bin's sub-region.  What a segment holds beyond its count (the padding included)
is FILL, 0xFFFFFFFF: anything that counted or moved one would show up."""
import numpy as np

# lime_amd/csrc/lime_kernels.h
PART_TILE = 8192                  # records per tile of k_part / k_part_lines (PART_WG * PART_PER)
REGION_SHIFT = 16
BIN_MAX = 3072
BIN_SHIFT_MAX = 25
MAX_SUB = 8
PROD_WAVES_MAX = 16               # segp_s holds 16 * MAX_SUB segments
LINES_BINS_MAX = 1536             # k_part_lines owns at most three bins per thread (launch_part: n_bins <= 3 * PART_WG)
FILL = 0xFFFFFFFF                 # pool words that are no record
OUT_FILL = 0xABABABAB             # what the output array holds before the call
GUARD = 1024                      # words in front of and behind the output's `total` words


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_seg(self):
        return self.prod_waves * self.n_sub

    @property
    def total(self):
        return int(self.wave_cnt.sum())


def bins_per_sub(bin_shift):
    return 1 << (32 - bin_shift)


def _offsets(rng, how, n, bin_shift):
    if how is None:
        return rng.integers(0, 1 << bin_shift, n, dtype=np.int64)
    if isinstance(how, np.ndarray):
        assert len(how) == n
        return how.astype(np.int64)
    return np.full(n, int(how), dtype=np.int64)


def _piece_records(rng, piece, sub, n_bins, bin_shift):
    b, n, how = piece
    assert 0 <= b < n_bins and b >> (32 - bin_shift) == sub, (b, sub)
    off = _offsets(rng, how, n, bin_shift)
    assert n == 0 or (off.min() >= 0 and off.max() < (1 << bin_shift))
    return ((np.int64(b) << bin_shift) | off) & 0xFFFFFFFF              # the cell's low 32 bits; its high part is the sub-region


def build(name, bin_shift, n_bins, n_sub, prod_waves, producers, seed=1, cap_w=None, facts=None):
    rng = np.random.default_rng(seed)
    n_seg = prod_waves * n_sub
    segs = []
    for p, prod in enumerate(producers):
        assert len(prod) == n_seg, (name, p, len(prod), n_seg)
        for i, seg in enumerate(prod):
            parts = []
            for item in seg:
                if isinstance(item, list):
                    mix = np.concatenate([_piece_records(rng, q, i % n_sub, n_bins, bin_shift) for q in item]) if item else np.zeros(0, np.int64)
                    rng.shuffle(mix)
                    parts.append(mix)
                else:
                    parts.append(_piece_records(rng, item, i % n_sub, n_bins, bin_shift))
            segs.append(np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32))
    longest = max(len(s) for s in segs)
    if cap_w is None:
        cap_w = max(16, (longest + 15) & ~15)
    assert cap_w % 16 == 0 and longest <= cap_w
    pool = np.full(len(segs) * cap_w, FILL, dtype=np.uint32)
    for i, s in enumerate(segs):
        pool[i * cap_w:i * cap_w + len(s)] = s
    wave_cnt = np.array([len(s) for s in segs], dtype=np.uint32)
    return Case(name=name, n_prod=len(producers), prod_waves=prod_waves, n_sub=n_sub, cap_w=cap_w, pool=pool, wave_cnt=wave_cnt,
                n_bins=n_bins, bin_shift=bin_shift, facts=dict(facts or {}))


# ---- what the arrays say (nothing below looks at a builder's parameters) -------------------------------------------------------------------
class Records:
    """every record of the pool, in pool order: its global segment, producer, sub-region, bin, output word, position in the producer's padded
    stream and tile of that stream"""

    def __init__(self, case):
        cnt = case.wave_cnt.astype(np.int64)
        nseg = case.n_seg
        self.seg = np.repeat(np.arange(len(cnt)), cnt)
        k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        self.rec = case.pool[self.seg * case.cap_w + k]
        self.sub = self.seg % case.n_sub
        self.prod = self.seg // nseg
        self.bin = (self.rec.astype(np.int64) >> case.bin_shift) + (self.sub << (32 - case.bin_shift))
        self.word = (self.rec & np.uint32((1 << case.bin_shift) - 1)) | np.uint32(1 << case.bin_shift)
        pad = ((cnt + 3) & ~3).reshape(case.n_prod, nseg)
        self.seg_p = np.concatenate([np.zeros((case.n_prod, 1), np.int64), np.cumsum(pad, axis=1)], axis=1)      # padded starts, [n_prod][n_seg + 1]
        self.spos = self.seg_p[self.prod, self.seg % nseg] + k
        self.tile = self.spos // PART_TILE


class Model:
    """binbase[b] = the lower bins' records; producer p's records of bin b occupy [start[b][p], + counts[b][p]); every word is
    (rec & mask) | 1 << bin_shift.  want: the output with every (bin, producer) range sorted; rid[i]: the range position i belongs to."""

    def __init__(self, case):
        r = self.rec = Records(case)
        nb, npr = case.n_bins, case.n_prod
        self.counts = np.bincount(r.bin * npr + r.prod, minlength=nb * npr).reshape(nb, npr)
        totals = self.counts.sum(axis=1)
        self.binbase = np.concatenate([[0], np.cumsum(totals)]).astype(np.uint64)
        self.start = self.binbase[:-1, None].astype(np.int64) + np.cumsum(self.counts, axis=1) - self.counts
        order = np.lexsort((r.word, r.prod, r.bin))
        self.want = r.word[order]
        self.rid = (r.bin * npr + r.prod)[order]
        self.total = len(self.want)
        for a in (self.want, self.rid, self.binbase, self.counts, self.start):
            a.setflags(write=False)


def model_naive(case):
    """the same, record by record -> (binbase list, {(bin, producer): sorted list of words})"""
    ranges, totals = {}, [0] * case.n_bins
    nseg = case.n_seg
    mask = (1 << case.bin_shift) - 1
    for i, n in enumerate(case.wave_cnt.tolist()):
        s, p = i % case.n_sub, i // nseg
        for rec in case.pool[i * case.cap_w:i * case.cap_w + n].tolist():
            b = (rec >> case.bin_shift) + (s << (32 - case.bin_shift))
            ranges.setdefault((b, p), []).append((rec & mask) | (1 << case.bin_shift))
            totals[b] += 1
    base = [0]
    for t in totals:
        base.append(base[-1] + t)
    return base, {k: sorted(v) for k, v in ranges.items()}


def output_buffer(total):
    return np.full(total + 2 * GUARD, OUT_FILL, dtype=np.uint32)


def compare(case, m, buf, binbase):
    """buf: GUARD words, the `total` output words, GUARD words.  None where the output is right, else what is wrong: bin, producer, the tiles of
    the producer's stream the missing records came from, the first differing words.  The order inside a (bin, producer) range is free, nothing
    else is: both sides are compared with every such range sorted."""
    buf = np.asarray(buf, dtype=np.uint32)
    if len(buf) != m.total + 2 * GUARD:
        return f"{case.name}: the buffer holds {len(buf)} words, not {m.total} + 2 * {GUARD}"
    bad = []
    bb = np.asarray(binbase, dtype=np.uint64)
    if len(bb) != case.n_bins + 1:
        bad.append(f"binbase holds {len(bb)} words, not {case.n_bins + 1}")
    elif not np.array_equal(bb, m.binbase):
        first = int(np.nonzero(bb != m.binbase)[0][0])
        bad.append(f"binbase differs from bin {first} on: got {bb[first:first + 4].tolist()}, want {m.binbase[first:first + 4].tolist()}")
    for name, g, lo in (("in front of", buf[:GUARD], -GUARD), ("behind", buf[GUARD + m.total:], m.total)):
        w = np.nonzero(g != OUT_FILL)[0]
        if len(w):
            bad.append(f"{len(w)} guard words {name} the output were written, the first at position {lo + int(w[0])}: {hex(int(g[w[0]]))}")
    body = buf[GUARD:GUARD + m.total]
    left = np.nonzero(body == OUT_FILL)[0]
    if len(left):
        bad.append(f"{len(left)} positions were never written, the first {left[:8].tolist()}")
    got = body[np.lexsort((body, m.rid))]
    diff = np.nonzero(got != m.want)[0]
    if len(diff):
        r = m.rec
        rids = np.unique(m.rid[diff])
        msg = [f"{len(diff)} words differ in {len(rids)} (bin, producer) ranges"]
        for rid in rids[:3].tolist():
            b, p = divmod(rid, case.n_prod)
            lo, n = int(m.start[b, p]), int(m.counts[b, p])
            g, w = got[lo:lo + n], m.want[lo:lo + n]
            gu, gc = np.unique(g, return_counts=True)
            wu, wc = np.unique(w, return_counts=True)
            have = dict(zip(gu.tolist(), gc.tolist()))
            missing = [x for x, c in zip(wu.tolist(), wc.tolist()) if have.get(x, 0) < c]
            mine = (r.bin == b) & (r.prod == p) & np.isin(r.word, np.array(missing, dtype=np.uint32))
            first = np.nonzero(g != w)[0][:4]
            msg.append(f"bin {b} producer {p} (positions {lo} .. {lo + n - 1}): {len(missing)} distinct words missing, from tiles "
                       f"{np.unique(r.tile[mine]).tolist()[:12]} of the producer's stream; sorted range at {first.tolist()}: got "
                       f"{[hex(int(x)) for x in g[first]]}, want {[hex(int(x)) for x in w[first]]}")
        bad.append("; ".join(msg))
    return f"{case.name}: " + " | ".join(bad) if bad else None


def tile_table(case):
    """tile_at / load_tile of the kernels in numpy -> per producer a list of (kind, records, segments touched): kind "one" -- the tile's words
    lie in one segment (the two-word description) --, or "mixed" (the per-group meta words)"""
    r = Records(case)
    cnt = case.wave_cnt.astype(np.int64).reshape(case.n_prod, case.n_seg)
    out = []
    for p in range(case.n_prod):
        sp, tiles = r.seg_p[p], []
        l_pad = int(sp[-1])
        for v0 in range(0, l_pad, PART_TILE):
            end = min(v0 + PART_TILE, l_pad)
            w0 = int(np.searchsorted(sp[1:], v0, side="right"))           # the first segment whose padded end lies behind v0
            one = end <= sp[w0 + 1]
            valid = np.minimum(sp[:-1] + cnt[p], end) - np.maximum(sp[:-1], v0)
            touched = np.nonzero(valid > 0)[0]
            tiles.append(("one" if one else "mixed", int(valid[valid > 0].sum()), touched.tolist()))
        out.append(tiles)
    return out


def carry_sim(case, m):
    """k_part_lines' bookkeeping in numpy: per producer and tile, per bin, the position G of the bin's next record, the C records carried, the
    tile's N; E = the records up to the last line border reached are emitted as L lines, the rest is carried.
    -> dict: max_carry; lines[p] = lines per tile; completes = {(carry before, left over)} of the tiles that completed a carried line;
    first = {(start % 16, (start + count) % 16, count)} per non-empty (bin, producer); flush[b][p] = (G, C) at the producer's end"""
    r = m.rec
    nb = case.n_bins
    res = dict(max_carry=0, lines=[], completes=set(), first=set(), flush_g=np.zeros((nb, case.n_prod), np.int64),
               flush_c=np.zeros((nb, case.n_prod), np.int64))
    for p in range(case.n_prod):
        mine = r.prod == p
        nt = int(r.tile[mine].max()) + 1 if mine.any() else 0
        per = np.bincount(r.tile[mine] * nb + r.bin[mine], minlength=nt * nb).reshape(nt, nb)
        G, C = m.start[:, p].copy(), np.zeros(nb, np.int64)
        lines = []
        for t in range(nt):
            N = per[t]
            end = G + C + N
            border = end & ~15
            emit = border > G
            E = np.where(emit, border - G, 0)
            L = np.where(emit, (border >> 4) - (G >> 4), 0)
            done = emit & (C > 0) & (N > 0)
            res["completes"] |= set(zip(C[done].tolist(), (C + N - E)[done].tolist()))
            G, C = G + E, C + N - E
            assert C.max() <= 15
            res["max_carry"] = max(res["max_carry"], int(C.max()))
            lines.append(int(L.sum()))
        res["lines"].append(lines)
        res["flush_g"][:, p], res["flush_c"][:, p] = G, C
        nz = m.counts[:, p] > 0
        s, c = m.start[nz, p], m.counts[nz, p]
        res["first"] |= set(zip((s % 16).tolist(), ((s + c) % 16).tolist(), c.tolist()))
    return res


def p64_bases(case, m, sim=None):
    """option p64_test_base values (multiples of 16: the option masks the low four bits) that put position 2^32 of the shifted output
    "bin_first": on a bin's first position; "mid_range": inside one producer's range of a bin, at least two tiles into it; "flush": on the first
    of the records k_part_lines' final flush of the carries writes for some (bin, producer); "above": everything above 2^33.  A kind the
    case's model has no place for is left out."""
    sim = sim or carry_sim(case, m)
    out = {"above": (1 << 33) + 48}
    totals = np.diff(m.binbase.astype(np.int64))
    bb = m.binbase[:-1].astype(np.int64)
    ok = np.nonzero((bb % 16 == 0) & (totals > 0) & (bb > 0))[0]
    if len(ok):
        out["bin_first"] = (1 << 32) - int(bb[ok[np.argmax(totals[ok])]])
    big = np.argwhere(m.counts >= 2 * PART_TILE + PART_TILE // 2 + 16)
    if len(big):
        b, p = big[0]
        out["mid_range"] = (1 << 32) - int((m.start[b, p] + 2 * PART_TILE + PART_TILE // 2) & ~15)
    fl = np.argwhere((sim["flush_c"] > 0) & (sim["flush_g"] % 16 == 0) & (sim["flush_g"] > 0))
    if len(fl):
        b, p = fl[np.argmax(sim["flush_c"][fl[:, 0], fl[:, 1]])]
        out["flush"] = (1 << 32) - int(sim["flush_g"][b, p])
    assert all(v % 16 == 0 for v in out.values())
    return out


def geometry_error(n_prod, prod_waves, n_sub, cap_w, pool, wave_cnt, n_bins, bin_shift, out_words, out_align=0):
    """lime_partition_records_dev's argument rules (lime_pass.cpp): None, or what is refused"""
    if pool is None or wave_cnt is None:
        return "NULL array"
    if n_prod < 1:
        return "n_prod"
    if not 1 <= prod_waves <= PROD_WAVES_MAX:
        return "prod_waves"
    if not 1 <= n_sub <= MAX_SUB:
        return "n_sub"
    if cap_w % 16:
        return "cap_w not a multiple of 16"
    if not REGION_SHIFT <= bin_shift <= BIN_SHIFT_MAX:
        return "bin_shift"
    if not 1 <= n_bins <= BIN_MAX:
        return "n_bins"
    if out_align % 64:
        return "d_out not 64-byte aligned"
    if prod_waves * n_sub * cap_w > 0xFFFFFFF0:
        return "pool too large"
    cnt = np.asarray(wave_cnt, dtype=np.int64)
    segs = n_prod * prod_waves * n_sub
    if len(cnt) != segs or len(pool) != segs * cap_w:
        return "array sizes"
    if (cnt > cap_w).any():
        return "a count above cap_w"
    if int(cnt.sum()) > out_words:
        return "more records than out_words"
    seg = np.repeat(np.arange(segs), cnt)
    k = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    rec = np.asarray(pool, dtype=np.uint32)[seg * cap_w + k].astype(np.int64)
    if ((rec >> bin_shift) + ((seg % n_sub) << (32 - bin_shift)) >= n_bins).any():
        return "a record's bin is n_bins or more"
    return None


# ---- pieces of cases ------------------------------------------------------------------------------------------------------------------------
def _spread(rng, n_seg, n_sub, bin_shift, pieces, mix=True):
    """a producer's segments with every piece in a random segment of its bin's sub-region; mix: a segment's pieces shuffled together"""
    segs = [[] for _ in range(n_seg)]
    for b, n, how in pieces:
        s = b >> (32 - bin_shift)
        segs[int(rng.integers(0, n_seg // n_sub)) * n_sub + s].append((b, n, how))
    return [[sg] if mix and sg else sg for sg in segs]


def _some(rng, n_bins, lo, hi, bins=None):
    """(bin, count, None) pieces: a seeded count in [lo, hi] for every bin of `bins` (all of them)"""
    bins = range(n_bins) if bins is None else bins
    return [(int(b), int(rng.integers(lo, hi + 1)), None) for b in bins]


def empty():
    """all counts 0: a workgroup returns before its first tile; the bases are all 0 and nothing is written"""
    return build("empty", 16, 3, 1, 2, [[[], []], [[], []]], facts={"total": 0})


def one_record():
    """a single record, in the last segment of the last producer (sub-region 1 of its last wave)"""
    prods = [[[] for _ in range(4)] for _ in range(3)]
    prods[2][3] = [(129, 1, 0x1ABCDEF)]
    return build("one_record", 25, 130, 2, 2, prods, facts={"total": 1})


def pad_mod4():
    """one producer, segments of 1, 2, 3, 5, 6, 7, 0, 4 records: one tile spans all of them -- the per-group meta words -- and every padding of
    0 .. 3 words occurs"""
    rng = np.random.default_rng(3)
    counts = [1, 2, 3, 5, 6, 7, 0, 4]
    prod = [[[(int(b), 1, None) for b in rng.integers(0, 7, n)]] if n else [] for n in counts]
    return build("pad_mod4", 17, 7, 1, 8, [prod], seed=3, facts={"counts": counts})


def _stream(rng, n_bins, n):
    """n records over all bins, multinomially, shuffled together"""
    c = rng.multinomial(n, np.full(n_bins, 1.0 / n_bins))
    return [[(b, int(k), None) for b, k in enumerate(c) if k]]


TILE_EDGE_COUNTS = [PART_TILE - 1, PART_TILE, PART_TILE + 1, 2 * PART_TILE, 2 * PART_TILE + 1]


def tile_edges():
    """single-segment producers of 8191, 8192, 8193, 16384 and 16385 records: whole "one" tiles, a last tile of one record, tile counts that are
    no multiple of four"""
    rng = np.random.default_rng(4)
    return build("tile_edges", 18, 37, 1, 1, [[_stream(rng, 37, n)] for n in TILE_EDGE_COUNTS], seed=4, facts={"counts": TILE_EDGE_COUNTS})


def tile_straddle():
    """producer 0: segments 8190, 6, 0, 8200, 3 -- a tile ends in a segment's padding, a tile starts in one segment and ends in another with an
    empty one between, a "one" tile is followed by a mixed one; producer 1: 5, 16376 -- a mixed tile is followed by a "one" tile"""
    rng = np.random.default_rng(5)
    p0 = [_stream(rng, 50, n) if n else [] for n in (8190, 6, 0, 8200, 3)]
    p1 = [_stream(rng, 50, n) if n else [] for n in (5, 16376, 0, 0, 0)]
    return build("tile_straddle", 16, 50, 1, 5, [p0, p1], seed=5, facts={"counts": [8190, 6, 0, 8200, 3, 5, 16376, 0, 0, 0]})


def one_bin_full_tiles():
    """64 bins; producers 0, 1, 2 each hold a tile of 8192 records that all go to bin 5, and start in that bin at residues 0, 1 and 15 of a
    line; producer 3 starts at residue 15 too, carries 15 records in each of bins 6 .. 20 through its first tile and completes all those lines in
    its second, next to 511 lines of bin 5: more than 512 lines in one tile; a third tile of bin 5 follows.  Producer 4 makes the lower bins' totals multiples of 16."""
    T = PART_TILE
    p0 = [[(5, T, None), (5, 1, None)]]
    p1 = [[(5, T, None), [(5, 14, None)] + [(b, 16, None) for b in (30, 31)]]]
    p2 = [[(5, T, None)]]
    p3 = [[[(5, T - 225, None)] + [(b, 15, None) for b in range(6, 21)], [(5, T - 15, None)] + [(b, 1, None) for b in range(6, 21)], (5, T, None)]]
    p4 = [[[(5, 1, None)] + [(b, 16, None) for b in range(5)] + [(b, 3, None) for b in range(21, 64)]]]
    return build("one_bin_full_tiles", 20, 64, 1, 1, [p0, p1, p2, p3, p4], seed=6, facts={"residues": [0, 1, 15], "bin": 5})


TRICKLE = {   # records per tile, 18 tiles, the sum a multiple of 16 (so every producer's start in every bin is a line border)
    "ones": [1] * 16 + [0, 0],                            # the carry climbs 1 .. 15, the 16th record completes the line: nothing left over
    "twos": [2] * 7 + [1, 2] + [2] * 7 + [1, 0],          # 15 carried, two more: one left over; then up to 15 again
    "burst": [1] * 15 + [6, 11, 0],                       # 15 carried, six more: five left over
    "gaps": [0, 2, 0, 1, 0, 2, 2, 0, 1, 2, 0, 2, 1, 2, 0, 0, 1, 0],
}


def carry_trickle():
    """18 tiles per producer, each one segment.  Bin 0 takes nearly everything; bins 1 .. 20 get 0, 1 or 2 records per tile (once a burst), so
    that their carries climb to exactly 15 and a line is then completed with 0, 1 and several records left over"""
    kinds = list(TRICKLE)
    prods = []
    for p in range(2):
        tiles = []
        for t in range(18):
            small = [(b, TRICKLE[kinds[(b + p) % 4]][t], None) for b in range(1, 21)]
            small = [q for q in small if q[1]]
            tiles.append([(0, PART_TILE - sum(q[1] for q in small), None)] + small)
        prods.append([tiles])
    return build("carry_trickle", 19, 24, 1, 1, prods, seed=7, facts={"tiles": 18})


def first_piece():
    """20 producers with two tiny segments each, 48 bins whose totals are multiples of 16: in bin (r, k) one producer holds r records, the next
    one -- which starts at residue r of a line -- a piece that ends one short of, exactly on, or one beyond the next line border, and the last
    producer what fills the line"""
    rng = np.random.default_rng(8)
    pieces = [[] for _ in range(20)]
    want = set()
    for r in range(16):
        for j, k in enumerate((-1, 0, 1)):
            b = 3 * r + j
            n = 16 - r + k if 16 - r + k > 0 else 32 - r + k
            pa = b % 18
            if r:
                pieces[pa].append((b, r, None))
            pieces[pa + 1].append((b, n, None))
            if (-(r + n)) % 16:
                pieces[19].append((b, (-(r + n)) % 16, None))
            want.add((r, k % 16))
    prods = [_spread(rng, 2, 1, 22, pc) for pc in pieces]
    return build("first_piece", 22, 48, 1, 2, prods, seed=8, facts={"pieces": want})


PRODUCER_COUNTS = [1, 63, 64, 65, 128, 130]


def producers(n_prod):
    """k_bin_rowscan takes a bin's producers in chunks of 64 lanes and carries the sum from chunk to chunk: n_prod on both sides of one chunk
    and of two, a few records each, some producers with none"""
    rng = np.random.default_rng(900 + n_prod)
    prods = []
    for p in range(n_prod):
        n = 0 if p % 7 == 3 else int(rng.integers(1, 24))
        prods.append([[[(int(b), 1, None) for b in rng.integers(0, 9, n)]] if n else []])
    return build(f"producers_{n_prod}", 16, 9, 1, 1, prods, seed=900 + n_prod, facts={"n_prod": n_prod})


BINS_LINES = [1, 2, 63, 64, 65, 255, 256]
BINS_EITHER = [511, 512, 513, 1024, 1025, 1536, 1537, 3071, 3072]
BINS_LAYOUT = [477, 478]          # bin_layout_of's LINES_BINS, the most bins a pass gives k_part_lines, and one more


def bins(n_bins, dense):
    """n_bins on both sides of the wave's 64 lanes, of one, two and three bins per thread, of what k_part_lines takes (and of what the bin layout
    gives it at most) and of BIN_MAX; dense:
    every bin holds records; sparse: only the first, the last and every 97th"""
    rng = np.random.default_rng(2000 + n_bins + (5000 if dense else 0))
    which = list(range(n_bins)) if dense else sorted(set([0, n_bins - 1] + list(range(0, n_bins, 97))))
    hi = max(3, min(40, 60000 // len(which)))
    prods = [_spread(rng, 3, 1, 16, _some(rng, n_bins, 0 if dense else 1, hi, which)) for _ in range(3)]
    if dense:                                                             # (a seeded count may be 0: one more record each from a fourth producer)
        prods.append(_spread(rng, 3, 1, 16, [(b, 1, None) for b in which]))
    return build(f"bins_{n_bins}_{'dense' if dense else 'sparse'}", 16, n_bins, 1, 3, prods, seed=2000 + n_bins,
                 facts={"non_empty": which})


def _edge_offsets(rng, n, bin_shift):
    """n offsets: 0 and all-ones first, seeded ones behind"""
    off = rng.integers(0, 1 << bin_shift, n, dtype=np.int64)
    off[:2] = [0, (1 << bin_shift) - 1]
    return off


SUB_REGIONS = {"2_25": (2, 25, 200, 4), "3_20": (3, 20, 3000, 4), "3_23": (3, 23, 1300, 4), "8_25": (8, 25, 1000, 16), "8_25_low": (8, 25, 400, 16)}


def sub_regions(key):
    """tables of several sub-regions: a segment's sub-region is the high part of its records' cells, and a mixed tile's groups carry it in their
    meta words.  "2_25": 200 bins; "8_25": prod_waves 16 -- 128 segments, all the kernels' segment table holds -- and 1000 bins; "3_23": 1300 bins
    in three sub-regions.  "3_20": at bin_shift 20 the bins of sub-regions 1 and 2 start at 4096 and 8192, beyond BIN_MAX: three sub-regions of
    which only the first can hold records, so two of every three segments are empty.  "8_25_low": 128 segments again, with 400 bins -- few enough
    for k_part_lines, which the 1000 bins of "8_25" are not --, so that sub-regions 4 .. 7 hold nothing.  Every bin's first records have the offsets 0 and all-ones."""
    n_sub, sh, n_bins, pw = SUB_REGIONS[key]
    rng = np.random.default_rng(3000 + n_sub + sh + n_bins)
    prods = []
    for p in range(3):
        pieces = []
        for b in rng.permutation(n_bins)[:n_bins * 2 // 3].tolist():
            n = int(rng.integers(2, 12))
            pieces.append((b, n, _edge_offsets(rng, n, sh)))
        prods.append(_spread(rng, pw * n_sub, n_sub, sh, pieces))
    return build(f"sub_regions_{key}", sh, n_bins, n_sub, pw, prods, seed=3000 + n_sub + sh + n_bins, facts={"n_sub": n_sub, "segments": pw * n_sub})


PROD_WAVES = [1, 4, 6, 8, 12, 16]


def prod_waves(pw):
    """one small shape -- 3 producers, two sub-regions, 150 bins, a few thousand records -- at 1, 4, 6, 8, 12 and 16 waves per producer"""
    rng = np.random.default_rng(4000)
    prods = [_spread(rng, pw * 2, 2, 25, _some(rng, 150, 0, 30)) for _ in range(3)]
    return build(f"prod_waves_{pw}", 25, 150, 2, pw, prods, seed=4000 + pw, facts={"prod_waves": pw})


def offsets(bin_shift):
    """the narrowest and the widest bins; in every bin, the top one included, records with the offsets 0 and all-ones.  bin_shift 25: the top bin
    of a sub-region is 127, and its all-ones record is 0xFFFFFFFF -- the same word as the pool's filling"""
    rng = np.random.default_rng(5000 + bin_shift)
    n_bins = 128 if bin_shift == 25 else 200
    prods = []
    for p in range(2):
        pieces = []
        for b in range(n_bins):
            n = int(rng.integers(2, 9))
            pieces.append((b, n, _edge_offsets(rng, n, bin_shift)))
        prods.append(_spread(rng, 2, 1, bin_shift, pieces))
    return build(f"offsets_{bin_shift}", bin_shift, n_bins, 1, 2, prods, seed=5000 + bin_shift, facts={"top_bin": n_bins - 1})


FUZZ_SEEDS = list(range(12))
FUZZ_POOL_WORDS = 2 << 20             # a fuzz pool holds at most 8 MB


def fuzz(seed):
    """a seeded shape: n_prod <= 6, prod_waves, n_sub, bin_shift, n_bins <= 600, segment counts 0 .. 20000 with a bias to 0 and to multiples of
    8192 +- 2 (as far as a pool of 8 MB allows: many segments are short ones)"""
    rng = np.random.default_rng(7000 + seed)
    n_prod = int(rng.integers(1, 7))
    pw = int(rng.choice([1, 2, 3, 4, 8, 16]))
    n_sub = int(rng.choice([1, 1, 2, 3, 5]))
    shifts = [sh for sh in range(REGION_SHIFT, BIN_SHIFT_MAX + 1) if (n_sub - 1) * bins_per_sub(sh) < 600]
    sh = int(rng.choice(shifts))
    bps = bins_per_sub(sh)
    n_bins = int(rng.integers((n_sub - 1) * bps + 1, min(600, n_sub * bps) + 1))
    n_seg = pw * n_sub
    top = min(20000, (FUZZ_POOL_WORDS // (n_prod * n_seg) - 16) & ~15)
    prods = []
    for p in range(n_prod):
        segs = []
        for i in range(n_seg):
            s = i % n_sub
            lo, hi = s * bps, min(n_bins, (s + 1) * bps)
            u = rng.random()
            if u < 0.3:
                n = 0
            elif u < 0.6:
                n = int(rng.integers(1, 3)) * PART_TILE + int(rng.integers(-2, 3))
            else:
                n = int(rng.integers(1, top + 1))
            n = max(0, min(n, top))
            if not n:
                segs.append([])
                continue
            live = rng.permutation(np.arange(lo, hi))[:int(rng.integers(1, hi - lo + 1))]
            c = rng.multinomial(n, rng.dirichlet(np.full(len(live), 0.3)))
            segs.append([[(int(b), int(k), None) for b, k in zip(live, c) if k]])
        prods.append(segs)
    return build(f"fuzz_{seed}", sh, n_bins, n_sub, pw, prods, seed=7000 + seed, facts={"seed": seed})


# name -> (n_bins, generator): the GPU tests know a case's bins without building anything
CASES = {
    "empty": (3, empty), "one_record": (130, one_record), "pad_mod4": (7, pad_mod4), "tile_edges": (37, tile_edges),
    "tile_straddle": (50, tile_straddle), "one_bin_full_tiles": (64, one_bin_full_tiles), "carry_trickle": (24, carry_trickle),
    "first_piece": (48, first_piece),
    **{f"producers_{n}": (9, (lambda n=n: producers(n))) for n in PRODUCER_COUNTS},
    **{f"bins_{n}_{d}": (n, (lambda n=n, d=d: bins(n, d == "dense"))) for n in BINS_LINES + BINS_EITHER + BINS_LAYOUT for d in ("dense", "sparse")},
    **{f"sub_regions_{k}": (v[2], (lambda k=k: sub_regions(k))) for k, v in SUB_REGIONS.items()},
    **{f"prod_waves_{pw}": (150, (lambda pw=pw: prod_waves(pw))) for pw in PROD_WAVES},
    "offsets_16": (200, lambda: offsets(16)), "offsets_25": (128, lambda: offsets(25)),
}
FUZZ = [f"fuzz_{s}" for s in FUZZ_SEEDS]           # (their n_bins is seeded: at most 600, so between the two kernels' certain grounds or below)


def make(name):
    case = fuzz(int(name[5:])) if name.startswith("fuzz_") else CASES[name][1]()
    assert case.name == name and (name.startswith("fuzz_") or case.n_bins == CASES[name][0])
    for a in (case.pool, case.wave_cnt):
        a.setflags(write=False)
    return case
