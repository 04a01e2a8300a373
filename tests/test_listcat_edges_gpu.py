"""lime_lists_concat_dev at its edges: the lists of column shards of one device table (lime_choose_lists_dev with beta -1 on column
slices), concatenated with the real beta, against lime_choose_lists_dev of the whole table: row_max, row_off and the pairs exactly
equal (and equal to the numpy model of tests/shard_cases.py).  Row counts around the wave and through k_lc_copy's grid stride (8192
one-wave workgroups: 16 384 + 5 rows), 1 / 2 / 3 / 7 parts of 1 .. 300 genomes, rows of 0 / 1 / 63 / 64 / 65 / 200 pairs, a part
without pairs, no passing row, the 21 / 22 threshold of norm 85 and beta 0.25, id_base up to 2^32 - 1 - n, a side stream, accumulation
in steps, 200 seeded cases, and every refusal with its text and device memory back where it was."""
import gc

import numpy as np
import pytest

from tests import shard_cases as HC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


def _lists(ctx, table, norm, beta, stream=None):
    """lime_choose_lists_dev of a host table"""
    import torch
    from lime_amd import api
    nr, ng = table.shape
    t = torch.zeros(api.sim_bytes(nr, ng), dtype=torch.uint8, device="cuda")
    t[:nr * ng] = torch.from_numpy(np.ascontiguousarray(table).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return ctx.choose_lists_dev(t, nr, ng, norm, beta, stream)


def _check(ctx, table, col_cuts, norm=HC.NORM, beta=HC.BETA, stream=None, what=None):
    """-> the concatenated list's host copies, after comparing them with the whole table's list and with the model"""
    parts = [_lists(ctx, t, norm, -1.0) for t in HC.split(table, col_cuts)]
    widths = np.diff(col_cuts)
    got_l = ctx.lists_concat(parts, col_cuts[:-1], widths, beta, stream)
    want_l = _lists(ctx, table, norm, beta)
    got, want = got_l.get(), want_l.get()
    assert HC.same_lists(got, want), what
    assert HC.same_lists(got, HC.choose(table, norm, beta)), what
    assert got_l.info() == want_l.info() == (table.shape[0], len(want[2]), norm, float(np.float32(beta))), what
    for li in parts + [got_l, want_l]:
        li.close()
    return got


def _widths(n_parts, rng, top):
    w = [int(x) for x in rng.choice([1, 2, 3, 17, 63, 64, 65, 129, 300], size=n_parts)]
    w[int(rng.integers(0, n_parts))] = top           # the widest part the case may hold
    return w


@pytest.mark.parametrize("n_parts", [1, 2, 3, 7])
@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 257, 16384 + 5])
def test_row_counts_and_part_counts(ctx, n_reads, n_parts):
    rng = np.random.default_rng([HC.SEED, 21, n_reads, n_parts])
    big = n_reads > 1000
    widths = _widths(n_parts, rng, 40 if big else 300)
    if big:
        widths = [min(w, 40) for w in widths]
    col_cuts = [0] + [int(x) for x in np.cumsum(widths)]
    table = HC.sparse_table(n_reads, col_cuts[-1], rng, density=0.03 if big else 0.1)
    table[n_reads - 1, col_cuts[-1] - 1] = 200       # the last row's last cell: the end of every array
    got = _check(ctx, table, col_cuts, what=(n_reads, widths))
    assert len(got[2]) > 0 and got[1][-1] == len(got[2])


def test_rows_of_every_length_across_the_parts(ctx):
    rng = np.random.default_rng([HC.SEED, 22])
    table = HC.rows_of_lengths(300, rng)
    for col_cuts in ([0, 300], [0, 1, 300], [0, 64, 128, 300], [0, 100, 101, 299, 300], [0, 30, 60, 90, 120, 150, 180, 300]):
        got = _check(ctx, table, col_cuts, what=col_cuts)
        assert tuple(np.diff(got[1].astype(np.int64))) == HC.ROW_LENGTHS


def test_threshold_rows_an_empty_part_and_no_passing_row(ctx):
    col_cuts = [0, 3, 5, 9, 11]
    table, names = HC.handmade(col_cuts)
    got = _check(ctx, table, col_cuts)
    lens = dict(zip(names, np.diff(got[1].astype(np.int64))))
    assert lens["21 in every part: fails"] == 0 and lens["21 and 22: passes, the 21s listed too"] == 3
    assert lens["passes only through another part's maximum"] == 3 and lens["22 alone in the last part"] == 1
    wide = np.concatenate([table[:, :5], np.zeros((len(table), 4), np.uint8), table[:, 5:]], axis=1)      # a part without any pair
    _check(ctx, wide, [0, 3, 5, 9, 13, 15])
    _check(ctx, np.zeros((70, 12), np.uint8), [0, 4, 12])                                                  # no pair at all
    none = _check(ctx, table, col_cuts, beta=5.0)                                                          # no row passes
    assert len(none[2]) == 0 and not none[1].any() and none[0].max() == 255
    every = _check(ctx, table, col_cuts, beta=-1.0)
    assert len(every[2]) == int((table != 0).sum())


def test_id_base_up_to_the_last_id_and_one_past_it(ctx):
    from lime_amd import _lib, api
    rng = np.random.default_rng([HC.SEED, 23])
    n = 9
    table = HC.sparse_table(66, n, rng, density=0.4)
    part = _lists(ctx, table, HC.NORM, -1.0)
    top = 2 ** 32 - 1 - n
    li = ctx.lists_concat([part], [top], [n], HC.BETA)
    got, want = li.get(), HC.choose(table, HC.NORM, HC.BETA)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2][:, 0].astype(np.uint64), want[2][:, 0].astype(np.uint64) + np.uint64(top)) and np.array_equal(got[2][:, 1], want[2][:, 1])
    assert int(got[2][:, 0].max()) <= 2 ** 32 - 2 and len(got[2]) > 0
    li.close()
    with pytest.raises(api.LimeError) as e:
        ctx.lists_concat([part], [top + 1], [n], HC.BETA)
    assert e.value.code == _lib.ERR_ARG and "2^32 - 1" in str(e.value)
    part.close()


def test_a_side_stream(ctx):
    import torch
    rng = np.random.default_rng([HC.SEED, 24])
    table = HC.sparse_table(300, 90, rng, density=0.2)
    s = torch.cuda.Stream()
    _check(ctx, table, [0, 20, 50, 90], stream=s.cuda_stream)
    torch.cuda.synchronize()


def test_accumulate_then_filter(ctx):
    rng = np.random.default_rng([HC.SEED, 25])
    table = HC.sparse_table(130, 70, rng, density=0.05, top=30)          # (few cells, most below 22: the filter drops rows)
    col_cuts = [0, 10, 11, 40, 70]
    parts = [_lists(ctx, t, HC.NORM, -1.0) for t in HC.split(table, col_cuts)]
    acc, width = ctx.lists_concat(parts[:1], [0], [col_cuts[1]], -1.0), col_cuts[1]
    for p, a, b in zip(parts[1:], col_cuts[1:], col_cuts[2:]):
        nxt = ctx.lists_concat([acc, p], [0, a], [width, b - a], -1.0)
        acc.close()
        acc, width = nxt, b
    assert HC.same_lists(acc.get(), HC.choose(table, HC.NORM, -1.0))
    filtered = ctx.lists_concat([acc], [0], [width], HC.BETA)
    one = ctx.lists_concat(parts, col_cuts[:-1], np.diff(col_cuts), HC.BETA)
    want = HC.choose(table, HC.NORM, HC.BETA)
    assert HC.same_lists(filtered.get(), want) and HC.same_lists(one.get(), want) and 0 < len(want[2]) < int((table != 0).sum())
    for li in parts + [acc, filtered, one]:
        li.close()


def test_200_seeded_cases(ctx):
    for case in range(200):
        rng = np.random.default_rng([HC.SEED, 26, case])
        n_parts = int(rng.choice([1, 2, 3, 7]))
        widths = [int(x) for x in rng.integers(1, 31, size=n_parts)]
        if case % 10 == 0:
            widths[int(rng.integers(0, n_parts))] = 300
        col_cuts = [0] + [int(x) for x in np.cumsum(widths)]
        table = HC.sparse_table(int(rng.integers(1, 200)), col_cuts[-1], rng, density=float(rng.choice([0.0, 0.02, 0.1, 0.6])))
        beta = float(rng.choice([HC.BETA, 0.0, -1.0, 0.5]))
        _check(ctx, table, col_cuts, beta=beta, what=(case, widths, beta))


def _free_bytes():
    import torch
    from lime_amd import api
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


def test_refusals(ctx):
    import torch
    from lime_amd import _lib, api
    rng = np.random.default_rng([HC.SEED, 27])
    table = HC.sparse_table(40, 12, rng, density=0.3)
    a, b = (_lists(ctx, t, HC.NORM, -1.0) for t in HC.split(table, [0, 5, 12]))
    short = _lists(ctx, table[:39, :5], HC.NORM, -1.0)
    other_norm = _lists(ctx, table[:, :5], HC.NORM + 1, -1.0)
    ctx2 = api.Context(0)
    foreign = _lists(ctx2, table[:, 5:], HC.NORM, -1.0)
    ctx.lists_concat([a, b], [0, 5], [5, 7], HC.BETA).close()              # a whole call first: what the runtime allocates on first launches
    before = _free_bytes()
    bad = {"no part": ([], [], [], "n_parts is 0"),
           "a NULL part": ([a, None], [0, 5], [5, 7], "part 1 is NULL"),
           "a part of another context": ([a, foreign], [0, 5], [5, 7], "another context"),
           "different n_reads": ([short, b], [0, 5], [5, 7], "different numbers of reads"),
           "different norm": ([other_norm, b], [0, 5], [5, 7], "different norms"),
           "id_base descending": ([a, b], [7, 0], [5, 7], "id_base must ascend"),
           "id ranges that overlap": ([a, b], [0, 4], [5, 7], "id_base must ascend"),
           "ids past 2^32 - 1": ([a, b], [0, 2 ** 32 - 7], [5, 7], "2^32 - 1")}
    for name, (parts, base, cnt, text) in bad.items():
        with pytest.raises(api.LimeError) as e:
            ctx.lists_concat(parts, base, cnt, HC.BETA)
        assert e.value.code == _lib.ERR_ARG and text in str(e.value), (name, e.value)
    assert _free_bytes() == before
    ok = ctx.lists_concat([a, b], [0, 2 ** 32 - 8], [5, 7], HC.BETA)        # ... and one genome less is legal
    assert int(ok.get()[2][:, 0].max()) <= 2 ** 32 - 2
    for li in (ok, a, b, short, other_norm):
        li.close()
    ctx2.close()
    torch.cuda.synchronize()
