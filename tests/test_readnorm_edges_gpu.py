"""Every read normalised by its own length, on the device at its edges: k_rn_norms (lime_docs_norms_dev), k_rn_rows
(lime_lists_concat_norms_dev) and k_classify_norms (lime_classify_lists_dev over lists with per-read norms).  The oracle throughout is the
fixed-norm path: the numpy models of tests/readnorm_cases.py, which stand on those of shard_cases / classify_cases, and the existing
device calls run once per group of equal norms on the whole input, every read taken from its group's run.  No tolerance anywhere."""
import gc

import numpy as np
import pytest

from tests import classify_cases as CC
from tests import readnorm_cases as RN
from tests import shard_cases as HC

pytestmark = pytest.mark.gpu

RN_LANES = 1024 * 256                               # launch_rn_norms: at most 1024 workgroups of 256 lanes, the rest by grid stride


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


# ---- k_rn_norms --------------------------------------------------------------------------------------------------------------------
def _docs_of_lengths(ctx, lengths, shift=0):
    """documents of the given lengths (the symbols do not matter); shift: doc_off handed over as a view `shift` words into its tensor"""
    import torch
    off = RN.doc_off_of(lengths)
    n_text = int(off[-1])
    text = torch.full((max(n_text, 1),), 65, dtype=torch.uint8, device="cuda")
    buf = torch.zeros(len(off) + shift, dtype=torch.int64, device="cuda")
    buf[shift:] = torch.from_numpy(off).cuda()
    view = buf[shift:]
    assert view.data_ptr() % 16 == (8 * shift) % 16
    return ctx.docs_from_arrays_dev(text, view, len(lengths), n_text)


@pytest.mark.parametrize("n_docs", [1, 63, 64, 65, 257, RN_LANES + 5])
def test_norms_of_lengths_around_alpha(ctx, n_docs):
    for alpha in (1, 16, 255):
        rng = np.random.default_rng([RN.SEED, 11, n_docs, alpha])
        edge = [0, 1, alpha - 1, alpha, min(alpha + 1, 255), 255]
        lengths = rng.choice(edge + [100, 75], size=n_docs)
        lengths[:min(n_docs, 6)] = edge[:min(n_docs, 6)]
        lengths[-1] = 255 if n_docs > 1 else lengths[-1]              # the last read: the end of both arrays
        d = _docs_of_lengths(ctx, lengths, shift=alpha % 2)           # (alpha 1 and 255: a doc_off view 8 bytes off a 16-byte boundary)
        got = ctx.docs_norms(d, alpha).cpu().numpy()
        want, long_ = RN.norms_of(lengths, alpha)
        assert len(long_) == 0 and np.array_equal(got, want), (n_docs, alpha, np.nonzero(got != want)[0][:5])
        assert got.min() >= 1
        d.close()


def test_norms_of_documents_from_the_device_fastq_parser(ctx):
    rng = np.random.default_rng([RN.SEED, 12])
    lengths = [int(x) for x in rng.choice([0, 1, 15, 16, 17, 60, 100, 255], size=300)]
    reads = [bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8)) for n in lengths]
    d = ctx.docs_from_fastq_bytes(RN.fastq_of(reads))
    assert d.info() == (300, sum(lengths))
    got = ctx.docs_norms(d, 16).cpu().numpy()
    assert np.array_equal(got, RN.norms_of(lengths, 16)[0])
    rc = d.revcomp()
    assert np.array_equal(ctx.docs_norms(rc, 16).cpu().numpy(), got)      # a reverse complement has its read's length
    d.close(); rc.close()


def test_reads_longer_than_255_are_refused_with_the_lowest_index(ctx):
    from lime_amd import _lib, api
    lengths = np.full(3000, 100)
    lengths[[2999, 1037, 2001, 1500]] = [256, 256, 300, 256]
    d = _docs_of_lengths(ctx, lengths)
    with pytest.raises(api.LimeError) as e:
        ctx.docs_norms(d, 16)
    assert e.value.code == _lib.ERR_ARG and "read 1037 holds 256 symbols" in str(e.value), e.value
    lengths[1037] = 255
    lengths[0] = 70000                                                # a length no byte and no 16 bits hold
    d2 = _docs_of_lengths(ctx, lengths)
    with pytest.raises(api.LimeError) as e:
        ctx.docs_norms(d2, 16)
    assert "read 0 holds 70000 symbols" in str(e.value), e.value
    with pytest.raises(api.LimeError) as e:
        ctx.docs_norms(d, 0)
    assert e.value.code == _lib.ERR_ARG and "alpha is 0" in str(e.value)
    d.close(); d2.close()


# ---- lime_lists_concat_norms_dev -----------------------------------------------------------------------------------------------------
def _lists(ctx, table, norm, beta, stream=None):
    import torch
    from lime_amd import api
    nr, ng = table.shape
    t = torch.zeros(api.sim_bytes(nr, ng), dtype=torch.uint8, device="cuda")
    t[:nr * ng] = torch.from_numpy(np.ascontiguousarray(table).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return ctx.choose_lists_dev(t, nr, ng, norm, beta, stream)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    return t


def _check(ctx, table, col_cuts, norms, beta, stream=None, what=None):
    """the column shards' unfiltered lists, concatenated with the test per read, against the model and against the fixed-norm model by groups"""
    parts = [_lists(ctx, t, HC.NORM, -1.0) for t in HC.split(table, col_cuts)]
    li = ctx.lists_concat_norms(parts, col_cuts[:-1], np.diff(col_cuts), _dev(norms), beta, stream)
    got = li.get()
    assert HC.same_lists(got, RN.choose_norms(table, norms, beta)), what
    assert HC.same_lists(got, RN.choose_by_groups(table, norms, beta)), what
    assert li.info() == (table.shape[0], len(got[2]), 0, float(np.float32(beta))), what
    assert np.array_equal(li.norms(), norms), what
    for x in parts + [li]:
        x.close()
    return got


@pytest.mark.parametrize("n_parts", [1, 2, 3, 7])
@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 257, 16384 + 5])
def test_row_counts_and_part_counts(ctx, n_reads, n_parts):
    rng = np.random.default_rng([RN.SEED, 21, n_reads, n_parts])
    big = n_reads > 1000
    widths = [int(x) for x in rng.choice([1, 2, 3, 17, 40] if big else [1, 2, 3, 17, 63, 64, 65, 129, 300], size=n_parts)]
    col_cuts = [0] + [int(x) for x in np.cumsum(widths)]
    table = HC.sparse_table(n_reads, col_cuts[-1], rng, density=0.03 if big else 0.1)
    table[n_reads - 1, col_cuts[-1] - 1] = 200
    norms = rng.choice([1, 17, 50, 85, 100, 240, 255], size=n_reads).astype(np.uint8)
    norms[-1] = 85                                                    # (the last row passes: the end of every array)
    got = _check(ctx, table, col_cuts, norms, HC.BETA, what=(n_reads, widths))
    assert len(got[2]) > 0 and got[1][-1] == len(got[2])


def test_rows_of_every_length_across_the_parts(ctx):
    rng = np.random.default_rng([RN.SEED, 22])
    table = HC.rows_of_lengths(300, rng)                              # every row's maximum is 30 or more: it passes under each of these norms
    norms = np.array([85, 1, 100, 50, 85, 100], dtype=np.uint8)
    for col_cuts in ([0, 300], [0, 64, 128, 300], [0, 30, 60, 90, 120, 150, 180, 300]):
        got = _check(ctx, table, col_cuts, norms, HC.BETA, what=col_cuts)
        assert tuple(np.diff(got[1].astype(np.int64))) == HC.ROW_LENGTHS


@pytest.mark.parametrize("beta", RN.BETAS)
def test_both_sides_of_the_threshold_for_every_norm(ctx, beta):
    table, norms, want = RN.threshold_rows(beta)
    assert set(int(x) for x in norms) == set(range(1, 256))
    got = _check(ctx, table, [0, 1, 3], norms, beta)                  # (the maximum alone in the first part)
    assert np.array_equal(np.diff(got[1].astype(np.int64)) > 0, want)


def test_constant_norms_give_the_fixed_norm_lists(ctx):
    rng = np.random.default_rng([RN.SEED, 23])
    table = HC.sparse_table(300, 90, rng, density=0.1)
    cuts = [0, 20, 50, 90]
    parts = [_lists(ctx, t, HC.NORM, -1.0) for t in HC.split(table, cuts)]
    for beta in (HC.BETA, 0.0, -1.0, 0.5):
        fixed = ctx.lists_concat(parts, cuts[:-1], np.diff(cuts), beta)
        per = ctx.lists_concat_norms(parts, cuts[:-1], np.diff(cuts), _dev(np.full(300, HC.NORM, np.uint8)), beta)
        assert HC.same_lists(per.get(), fixed.get()), beta
        assert HC.same_lists(per.get(), _lists(ctx, table, HC.NORM, beta).get()), beta
        fixed.close(); per.close()


def test_accumulate_then_filter(ctx):
    rng = np.random.default_rng([RN.SEED, 25])
    table = HC.sparse_table(130, 70, rng, density=0.05, top=30)
    norms = rng.choice([50, 85, 100], size=130).astype(np.uint8)
    col_cuts = [0, 10, 11, 40, 70]
    parts = [_lists(ctx, t, HC.NORM, -1.0) for t in HC.split(table, col_cuts)]
    acc, width = ctx.lists_concat(parts[:1], [0], [col_cuts[1]], -1.0), col_cuts[1]
    for p, a, b in zip(parts[1:], col_cuts[1:], col_cuts[2:]):
        nxt = ctx.lists_concat([acc, p], [0, a], [width, b - a], -1.0)
        acc.close()
        acc, width = nxt, b
    every = ctx.lists_concat_norms([acc], [0], [width], _dev(norms), -1.0)       # a negative beta keeps every non-zero row
    assert HC.same_lists(every.get(), HC.choose(table, HC.NORM, -1.0))
    filtered = ctx.lists_concat_norms([acc], [0], [width], _dev(norms), HC.BETA)
    again = ctx.lists_concat_norms([every], [0], [width], _dev(norms), HC.BETA)  # (a part with norms of its own: they play no part)
    one = ctx.lists_concat_norms(parts, col_cuts[:-1], np.diff(col_cuts), _dev(norms), HC.BETA)
    want = RN.choose_norms(table, norms, HC.BETA)
    assert HC.same_lists(filtered.get(), want) and HC.same_lists(one.get(), want) and HC.same_lists(again.get(), want)
    assert 0 < len(want[2]) < int((table != 0).sum())
    for li in parts + [acc, every, filtered, again, one]:
        li.close()


def test_a_side_stream(ctx):
    import torch
    rng = np.random.default_rng([RN.SEED, 24])
    table = HC.sparse_table(300, 90, rng, density=0.2)
    norms = rng.choice(RN.MATE_NORMS, size=300).astype(np.uint8)
    s = torch.cuda.Stream()
    _check(ctx, table, [0, 20, 50, 90], norms, HC.BETA, stream=s.cuda_stream)
    torch.cuda.synchronize()


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
    rng = np.random.default_rng([RN.SEED, 27])
    table = HC.sparse_table(40, 12, rng, density=0.3)
    a, b = (_lists(ctx, t, HC.NORM, -1.0) for t in HC.split(table, [0, 5, 12]))
    short = _lists(ctx, table[:39, :5], HC.NORM, -1.0)
    other_norm = _lists(ctx, table[:, :5], HC.NORM + 1, -1.0)
    ctx2 = api.Context(0)
    foreign = _lists(ctx2, table[:, 5:], HC.NORM, -1.0)
    norms = _dev(np.full(40, 85, np.uint8))
    per = ctx.lists_concat_norms([a, b], [0, 5], [5, 7], norms, HC.BETA)    # a whole call first: what the runtime allocates on first launches
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
            ctx.lists_concat_norms(parts, base, cnt, norms, HC.BETA)
        assert e.value.code == _lib.ERR_ARG and text in str(e.value) and "lime_lists_concat_norms_dev" in str(e.value), (name, e.value)
    with pytest.raises(api.LimeError) as e:
        ctx.lists_concat_norms([a, b], [0, 5], [5, 7], None, HC.BETA)
    assert e.value.code == _lib.ERR_ARG and "d_norms is NULL" in str(e.value)
    with pytest.raises(api.LimeError) as e:                                 # the fixed-norm call takes no per-read part
        ctx.lists_concat([per], [0], [12], HC.BETA)
    assert e.value.code == _lib.ERR_ARG and "norm per read" in str(e.value)
    with pytest.raises(api.LimeError) as e:                                 # and a list with one norm has no norms to copy out
        a.norms()
    assert e.value.code == _lib.ERR_ARG and "one norm" in str(e.value)
    for call in (lambda: ctx.choose_lists_dev(torch.zeros(16, dtype=torch.uint8, device="cuda"), 1, 1, api.NORM_PER_READ, 0.25),
                 lambda: ctx.choose_pairs_dev(torch.zeros(16, dtype=torch.uint8, device="cuda"), 1, 1, api.NORM_PER_READ, 0.25)):
        with pytest.raises(api.LimeError) as e:                             # LIME_NORM_PER_READ is the sample calls' alone
            call()
        assert e.value.code == _lib.ERR_ARG and "LIME_NORM_PER_READ" in str(e.value)
    assert _free_bytes() == before
    for li in (per, a, b, short, other_norm):
        li.close()
    ctx2.close()
    torch.cuda.synchronize()


# ---- Classify over lists with per-read norms ---------------------------------------------------------------------------------------
def _upload(sim):
    import torch
    from lime_amd import api
    nr, ng = sim.shape
    t = torch.zeros(api.sim_bytes(nr, ng), dtype=torch.uint8, device="cuda")
    t[:nr * ng] = torch.from_numpy(np.ascontiguousarray(sim).reshape(-1)).cuda()
    return t


def _per_read_lists(ctx, col, tables, read_norms, stream=None):
    """per list: the unfiltered list of its table (beta -1), then the per-read filter (one part, id_base 0)"""
    n_reads, n_targ = col["sims"][0].shape
    out = []
    for t, nm in zip(tables, read_norms):
        raw = ctx.choose_lists_dev(t, n_reads, n_targ, 1, -1.0, stream)
        out.append(ctx.lists_concat_norms([raw], [0], [n_targ], _dev(nm), col["beta"], stream))
        raw.close()
    return out


def run(ctx, col, read_norms, combos, tmp_path, stream=None, fixed=None):
    """the collection with per-read norms through the device path for every (binary, higher, rank) of combos, against the fixed-norm device
    path by groups (whole input per group), lime_classify_mem_norms and the model by groups.  fixed: {list: norm} of the lists that are
    made with that one norm instead (a call that mixes both kinds); read_norms holds the same norm for them"""
    import torch
    from lime_amd import api
    n_files, n_targ, beta = len(col["sims"]), col["n_targ"], col["beta"]
    n_reads = col["sims"][0].shape[0]
    fixed = fixed or {}
    tables = [_upload(s) for s in col["sims"]]
    torch.cuda.synchronize()
    dev = _per_read_lists(ctx, col, tables, read_norms, stream)
    for i, n in fixed.items():
        dev[i].close()
        dev[i] = ctx.choose_lists_dev(tables[i], n_reads, n_targ, n, beta, stream)
    host = RN.lists_norms(col, read_norms)
    for li, want in zip(dev, host):
        assert HC.same_lists(li.get(), want), (col["name"], "lists")
    groups = RN.groups_of(read_norms)
    group_lists = {key: [ctx.choose_lists_dev(t, n_reads, n_targ, n, beta, stream) for t, n in zip(tables, key)] for key in groups}
    tax = str(tmp_path / "lineage.csv")
    open(tax, "wb").write(col["tax"])
    for binary, higher, rank in combos:
        where = (col["name"], binary, higher, rank)
        tx = api.load_taxonomy(tax, rank, higher, n_targ)
        v, counts = ctx.classify_lists_dev(dev, n_targ, tx, binary, stream)
        want = np.zeros(n_reads, dtype=api.VERDICT)
        for key, reads in groups.items():                            # the existing kernel, once per group on the whole input
            gv, _ = ctx.classify_lists_dev(group_lists[key], n_targ, tx, binary, stream)
            want[reads] = gv[reads]
        assert v.tobytes() == want.tobytes(), (where, "against the fixed-norm device path", np.nonzero(v != want)[0][:5])
        vm, cm = api.classify_mem(host, [fixed.get(i, 0) for i in range(n_files)], [beta] * n_files, n_targ, tx, binary,
                                  read_norms=[None if i in fixed else read_norms[i] for i in range(n_files)])
        assert v.tobytes() == vm.tobytes() and counts == cm, (where, "against lime_classify_mem_norms")
        rep = RN.model_by_groups(col, read_norms, rank, higher, binary, subset=True)
        assert CC.same_verdicts(rep, v) is None, (where, "against model_decide", CC.same_verdicts(rep, v))
        tx.close()
    for li in dev + [x for ls in group_lists.values() for x in ls]:
        li.close()


def _cols():
    return {"near_tie": lambda n_files: CC.near_tie_tables(n_files, 60, 130 if n_files == 2 else 200, seed=30 + n_files),
            "beta0": lambda n_files: CC.beta0_tables(n_files, 45, 129, seed=35)}


@pytest.mark.parametrize("n_files", (2, 4))
@pytest.mark.parametrize("kind", ("near_tie", "beta0"))
def test_norms_drawn_per_mate_every_combo(ctx, kind, n_files, tmp_path):
    col = _cols()[kind](n_files)
    rng = np.random.default_rng([RN.SEED, 31, n_files])
    read_norms = RN.draw_norms(n_files, col["sims"][0].shape[0], rng)
    if n_files == 4:
        assert (read_norms[0] != read_norms[2]).any()                 # mates of one read differ
    assert {int(x) for x in read_norms[0]} == set(RN.MATE_NORMS)
    run(ctx, col, read_norms, CC.COMBOS, tmp_path)


@pytest.mark.parametrize("n_files", (2, 4))
def test_norms_50_and_100_in_one_launch_on_the_tolerance(ctx, n_files, tmp_path):
    col, read_norms = RN.mixed_tolerance(n_files, 90, 70, seed=33 + n_files)
    run(ctx, col, read_norms, CC.COMBOS, tmp_path)


def test_per_read_lists_next_to_lists_with_one_norm(ctx, tmp_path):
    col = CC.near_tie_tables(4, 60, 200, seed=32)
    rng = np.random.default_rng([RN.SEED, 32])
    per = rng.choice(RN.MATE_NORMS, size=60).astype(np.uint8)
    one = np.full(60, col["norm"], np.uint8)
    run(ctx, col, [per, per, one, one], ((1, 1, 1), (0, 0, 1), (1, 0, 0)), tmp_path, fixed={2: col["norm"], 3: col["norm"]})
    run(ctx, col, [one, per, one, per], ((1, 1, 2),), tmp_path, fixed={0: col["norm"], 2: col["norm"]})


def test_grid_stride(ctx, tmp_path):
    col = CC.stride_case()
    n = CC.STRIDE_READS
    nm = np.where(np.arange(n) % 3 == 0, 100, 85).astype(np.uint8)
    nm[[0, 4, 16384, n - 1]] = [50, 255, 50, 1]
    run(ctx, col, [nm, nm], ((1, 1, 1), (0, 0, 0)), tmp_path)


def test_a_side_stream_for_classify(ctx, tmp_path):
    import torch
    col = CC.near_tie_tables(2, 60, 130, seed=31)
    read_norms = RN.draw_norms(2, 60, np.random.default_rng([RN.SEED, 33]))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        run(ctx, col, read_norms, ((1, 1, 1),), tmp_path, stream=s.cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()


def test_zz_the_fixed_norm_kernel_still_gives_the_references_bytes(ctx, tmp_path):
    """last in the module: after the per-read launches the same context gives the reference's bytes on classify_paired.npz through k_classify"""
    import os
    from lime_amd import api
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classify_paired.npz"))
    norm, beta = int(g["norm"]), float(g["beta"])
    _, n_reads, n_targ = g["sims"].shape
    tax = str(tmp_path / "lineage.csv")
    open(tax, "wb").write(g["tax"].tobytes())
    tx = api.load_taxonomy(tax, 1, 1, n_targ)
    tables = [_upload(s) for s in g["sims"]]
    fixed = [ctx.choose_lists_dev(t, n_reads, n_targ, norm, beta) for t in tables]
    per = _per_read_lists(ctx, dict(sims=list(g["sims"]), beta=beta), tables, [np.full(n_reads, norm, np.uint8)] * 4)
    for lists in (fixed, per):
        v, _ = ctx.classify_lists_dev(lists, n_targ, tx, True)
        outp = str(tmp_path / "after.txt")
        api.write_classification(outp, v)
        assert open(outp, "rb").read() == g["out_b1_h1_r1"].tobytes()
    tx.close()
