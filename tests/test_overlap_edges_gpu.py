"""The device overlap cut (lime_docs_trim_overlap_dev, lime_seq_reader_set_overlap / _next_pair; lime_overlap_kernel.hip) against
lime_pair_overlap_trim and the models of tests/overlap_cases.py: both texts, both doc_off, the inserts and every info field exactly equal.
Mate lengths around the kernel's word (64), its multiples and the 512 symbols whose words it keeps, equal and unequal; every insert of a
130 / 100 pair; hits at the edges of the candidate steps; the mismatch thresholds; collections around a workgroup's 4 pairs and past the grid
cap; documents of every origin; the refusals; the readers in batches and the chain of all four stages.
tests/test_overlap_cases_cpu.py holds lime_pair_overlap_trim against the models."""
import gc

import numpy as np
import pytest

from tests import adapter_cases as A
from tests import filter_cases as F
from tests import overlap_cases as V
from tests import trim_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


def _docs(ctx, reads, stream=None):
    import torch
    text, off = V.records(reads)
    t = torch.from_numpy(text).cuda() if len(text) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    return ctx.docs_from_arrays_dev(t, torch.from_numpy(off.astype(np.int64)).cuda(), len(reads), len(text), stream=stream)


def _check(ctx, r1, r2, params, what, d=None, stream=None, model=True):
    """the documents `d` (default: made from r1, r2 as arrays) cut with every (O, E) of params: against lime_pair_overlap_trim, and
    (model=True) against the numpy model -> the last inserts"""
    from lime_amd import api
    own = d is None
    if own:
        d = (_docs(ctx, r1, stream), _docs(ctx, r2, stream))
    ins = None
    for O, E in params:
        w1, f1, w2, f2, w_ins, w_info = api.overlap_trim(*V.records(r1), *V.records(r2), O, E)
        if model:
            m1, m2, m_ins, m_info = V.cut_model(r1, r2, O, E, insert=V.insert_masks)
            assert m_info == w_info and m_ins == w_ins.tolist() and np.array_equal(V.records(m1)[1], f1) and np.array_equal(V.records(m2)[1], f2), (what, O, E)
        o1, o2, info, ins = ctx.docs_trim_overlap(d[0], d[1], O, E, want_insert=True, stream=stream)
        if not np.array_equal(ins, w_ins):
            bad = int(np.nonzero(ins != w_ins)[0][0])
            raise AssertionError(f"{what}, overlap {O} error {E}: pair {bad} of {len(r1[bad])} / {len(r2[bad])} symbols has insert {int(ins[bad])}, not {int(w_ins[bad])}")
        for out, w_text, w_off, r in ((o1, w1, f1, r1), (o2, w2, f2, r2)):
            o_text, o_off = out.get()
            assert not out.has_qual and out.info() == (len(r), int(w_off[-1])), (what, O, E)
            assert np.array_equal(o_off, w_off) and np.array_equal(o_text, w_text), (what, O, E)
            out.close()
        assert info == w_info, (what, O, E, info, w_info)
        p1, p2, info2 = ctx.docs_trim_overlap(d[0], d[1], O, E, stream=stream)          # without the inserts: the same documents
        assert info2 == w_info and np.array_equal(p1.get()[1], f1) and np.array_equal(p2.get()[0], w2)
        p1.close(); p2.close()
    if own:
        d[0].close(); d[1].close()
    return ins


def _pairs_at(rng, lengths, O):
    """per (La, Lb): an unrelated pair, and a planted one at the insert lengths where the candidates begin and end and the mates end"""
    r1, r2 = [], []
    for La in lengths:
        for Lb in lengths:
            r1.append(V.bases(rng, La)); r2.append(V.bases(rng, Lb))
            for I in sorted({O, min(La, Lb), max(La, Lb), La + Lb - O, (La + Lb) // 2}):
                if O <= I <= La + Lb - O and min(La, Lb) > 0:
                    a, b = V.plant(rng, V.bases(rng, I), I, La=La, Lb=Lb)
                    r1.append(a); r2.append(b)
    return r1, r2


@pytest.mark.parametrize("O", [30, 1])
def test_mate_lengths_equal_and_unequal(ctx, O):
    rng = np.random.default_rng([V.SEED, 10, O])
    lengths = V.LENGTHS(30)
    assert {0, 1, 29, 30, 63, 64, 65, 255, 256, 257, 1000} <= set(lengths)
    r1, r2 = _pairs_at(rng, lengths, O)
    ins = _check(ctx, r1, r2, ((O, 0), (O, 10)), f"mate lengths, overlap {O}", model=False)
    assert np.count_nonzero(ins) > len(lengths) ** 2
    few = slice(0, len(r1), 17)                                               # the numpy model on every 17th pair
    m_ins = V.cut_model(r1[few], r2[few], O, 10, insert=V.insert_masks)[2]
    assert m_ins == ins[few].tolist()


def test_one_pair_of_5000_symbols(ctx):
    rng = np.random.default_rng([V.SEED, 11])
    r1, r2 = [], []
    for I in (4000, 5000, 7000, 9970):
        a, b = V.plant(rng, V.bases(rng, I), I, n_err=20 if I < 9000 else 0, La=5000, Lb=5000)
        r1.append(a); r2.append(b)
    a, b = V.bases(rng, 5000), V.bases(rng, 5000)
    ins = _check(ctx, r1 + [a, r1[0][:100]], r2 + [b, r2[0][:90]], ((30, 10),), "5000 symbols", model=False)
    assert ins.tolist()[:5] == [4000, 5000, 7000, 9970, 0]
    assert V.insert_masks(r1[0], r2[0], 30, 10) == 4000


@pytest.mark.parametrize("name", sorted(V.hand_cases()))
def test_the_hand_made_cases(ctx, name):
    r1, r2, O, E = V.hand_cases()[name]
    _check(ctx, r1, r2, ((O, E),), name)


def test_the_mismatch_thresholds_and_the_trap(ctx):
    cases = V.threshold_cases()
    for E in (0, 10, 50):
        sel = [c for c in cases.values() if c[3] == E]
        assert len(sel) == 8
        ins = _check(ctx, [c[0] for c in sel], [c[1] for c in sel], ((30, E),), f"thresholds at {E} percent")
        assert [(int(i) == c[4]) for i, c in zip(ins, sel)] == [c[5] <= (c[4] * E) // 100 for c in sel]
    for n_err, want in ((5, 150), (6, 60)):
        a, b, O, E, _, _ = V.trap(n_err)
        assert _check(ctx, [a], [b], ((O, E),), f"the trap with {n_err} mismatches").tolist() == [want]


def _collection(seed, n, top=130, O=30, errs=4, kit=True):
    """n pairs of mates of top - 30 .. top - 1 symbols: half read-through with fewer than `errs` errors, a quarter long fragments, a quarter
    unrelated.  kit=False: behind the fragment come adapters of the pair's own, which no adapter trim knows"""
    rng = np.random.default_rng([V.SEED, 12, seed])
    r1, r2 = [], []
    for _ in range(n):
        La, Lb = int(rng.integers(top - 30, top)), int(rng.integers(top - 30, top))
        u = rng.random()
        if u < 0.5:
            I = int(rng.integers(O, min(La, Lb)))
        elif u < 0.75:
            I = int(rng.integers(max(La, Lb), La + Lb - O + 1))
        else:
            I = La + Lb + 5
        ad = (V.TRUSEQ_R1, V.TRUSEQ_R2) if kit or rng.random() < 0.3 else (V.bases(rng, 33), V.bases(rng, 33))
        a, b = V.plant(rng, V.bases(rng, I), I, ad[0], ad[1], n_err=int(rng.integers(0, errs)), La=La, Lb=Lb)
        r1.append(a); r2.append(b)
    return r1, r2


@pytest.mark.parametrize("n", list(range(1, 66)))
def test_collections_of_1_to_65_pairs(ctx, n):
    r1, r2 = _collection(n, n)
    _check(ctx, r1, r2, ((30, 10),), f"{n} pairs")


@pytest.mark.parametrize("n", [V.PAIRS_PER_TRIP + 1, V.PAIRS_PER_TRIP + 2], ids=["one over a trip", "two over a trip"])
def test_past_the_grids_pairs_per_trip(ctx, n):
    """whoever changes RD_BLOCKS or RD_WAVES in lime_reads.h changes overlap_cases.PAIRS_PER_TRIP: the last one or two pairs are
    a wave's second.  The numpy model on the first and last 200 pairs, lime_pair_overlap_trim on all"""
    assert V.PAIRS_PER_TRIP == 8192
    r1, r2 = _collection(n, n, top=50, O=8, errs=1)                           # (no errors: three in four pairs are planted within the candidates)
    ins = _check(ctx, r1, r2, ((8, 10),), f"{n} pairs", model=False)
    for sl in (slice(0, 200), slice(n - 200, n)):
        assert V.cut_model(r1[sl], r2[sl], 8, 10, insert=V.insert_masks)[2] == ins[sl].tolist()
    assert np.count_nonzero(ins) > n // 2


def test_every_pair_empty_and_no_pair(ctx):
    _check(ctx, [b""] * 70, [b""] * 70, ((30, 10),), "70 empty pairs")
    _check(ctx, [], [], ((30, 10),), "no pair")


def test_documents_of_every_origin(ctx):
    """FASTA and FASTQ parses without and with qualities, the quality trim's, the adapter trim's and the filter's output, arrays: the cut takes
    each, mixed, and its output holds no qualities"""
    r1, r2 = _collection(101, 300, top=150)
    rng = np.random.default_rng([V.SEED, 13])
    q1, q2 = [T.sample_quals(rng, len(r)) for r in r1], [T.sample_quals(rng, len(r)) for r in r2]
    params = ((30, 10), (20, 0))
    for d in ((ctx.docs_from_bytes(V.fasta_of(r1)), ctx.docs_from_fastq_bytes(T.fastq_of(r2, q2))),
              (ctx.docs_from_fastq_qual_bytes(T.fastq_of(r1, q1)), _docs(ctx, r2))):
        _check(ctx, r1, r2, params, "parsed documents", d=d)
        d[0].close(); d[1].close()
    raw = [ctx.docs_from_fastq_qual_bytes(T.fastq_of(r, q)) for r, q in ((r1, q1), (r2, q2))]
    cut = [ctx.docs_trim(x, 0, 20)[0] for x in raw]
    _check(ctx, T.trim_model(r1, q1, 0, 20)[0], T.trim_model(r2, q2, 0, 20)[0], params, "the quality trim's output", d=cut)
    ad = [ctx.docs_trim_adapter(x, a, 3, 10)[0] for x, a in zip(raw, (V.TRUSEQ_R1, V.TRUSEQ_R2))]
    _check(ctx, A.trim_model(r1, V.TRUSEQ_R1, 3, 10)[0], A.trim_model(r2, V.TRUSEQ_R2, 3, 10)[0], params, "the adapter trim's output", d=ad)
    p = F.params(max_len=110, min_len=100)
    fl = [ctx.docs_filter(x, max_len=110, min_len=100)[0] for x in raw]
    _check(ctx, F.filter_model(r1, p)[0], F.filter_model(r2, p)[0], params, "the filter's output", d=fl)
    for x in raw + cut + ad + fl:
        x.close()


def test_text_at_offsets_that_are_no_multiples_of_64(ctx):
    """a first pair of 1 .. 63 symbols pushes every later read off the 64-byte lines, and the arrays themselves come from views at odd addresses"""
    import torch
    rng = np.random.default_rng([V.SEED, 14])
    for shift in (1, 7, 63):
        r1, r2 = _collection(200 + shift, 64)
        r1, r2 = [V.bases(rng, shift)] + r1, [V.bases(rng, 64 - shift)] + r2
        d = []
        for r in (r1, r2):
            text, off = V.records(r)
            raw = torch.zeros(len(text) + 128, dtype=torch.uint8, device="cuda")
            view = raw[shift:shift + len(text)]
            view.copy_(torch.from_numpy(text))
            d.append(ctx.docs_from_arrays_dev(view, torch.from_numpy(off.astype(np.int64)).cuda(), len(r), len(text)))
        _check(ctx, r1, r2, ((30, 10),), f"shift {shift}", d=d)
        d[0].close(); d[1].close()


def test_side_stream(ctx):
    import torch
    r1, r2 = _collection(102, 2000)
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _check(ctx, r1, r2, ((30, 10),), "side stream", stream=s.cuda_stream, model=False)
    s.synchronize()
    torch.cuda.synchronize()


def test_seeded_collections(ctx):
    for case in range(0, V.FUZZ_CASES, 2):
        r1, r2, O, E = V.fuzz_collection(V.SEED, case)
        _check(ctx, r1, r2, ((O, E),), f"fuzz_collection({V.SEED}, {case})", model=case % 8 == 0)


def _free_bytes():
    import torch
    from lime_amd import api
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


def test_refusals_and_device_memory_comes_back(ctx):
    """every refusal comes before any launch, with a text; after cuts and refusals of each kind and lime_trim_cache the device's free memory is
    what it was"""
    import ctypes as C
    from lime_amd import _lib, api
    r1, r2 = _collection(103, 1000)
    other = api.Context(0)

    def cycle():
        d1, d2, d3 = _docs(ctx, r1), _docs(ctx, r2), _docs(ctx, r2[:-1])
        o1, o2, info = ctx.docs_trim_overlap(d1, d2)
        assert info["n_cut"] > 0
        for O, E, word in ((0, 10, "overlap"), (30, 51, "0 .. 50")):
            with pytest.raises(api.LimeError) as e:
                ctx.docs_trim_overlap(d1, d2, O, E)
            assert e.value.code == _lib.ERR_ARG and word in str(e.value) and "lime_docs_trim_overlap_dev:" in str(e.value)
        with pytest.raises(api.LimeError) as e:
            ctx.docs_trim_overlap(d1, d3)
        assert e.value.code == _lib.ERR_ARG and "different numbers of reads" in str(e.value)
        with pytest.raises(api.LimeError) as e:
            other.docs_trim_overlap(d1, d2)
        assert e.value.code == _lib.ERR_ARG and "another context" in str(e.value)
        for args in ((None, d1.h, d2.h), (ctx.h, None, d2.h), (ctx.h, d1.h, None)):
            h1, h2, oi = C.c_void_p(1), C.c_void_p(1), _lib.OverlapInfo(7, 7, 7, 7, 7)
            assert ctx.lib.lime_docs_trim_overlap_dev(*args, 30, 10, None, None, C.byref(h1), C.byref(h2), C.byref(oi)) == _lib.ERR_ARG
            assert h1.value is None and h2.value is None and oi.n_pairs == 0 and "NULL" in ctx.lib.lime_last_error().decode()
        assert ctx.lib.lime_docs_trim_overlap_dev(ctx.h, d1.h, d2.h, 30, 10, None, None, None, None, None) == _lib.ERR_ARG
        for x in (d1, d2, d3, o1, o2):
            x.close()

    try:
        cycle()
        before = _free_bytes()
        cycle()
        assert _free_bytes() == before
    finally:
        other.close()


# ---- the readers ----
def _pair_batches(ra, rb, batch):
    texts, lens, first = ([], []), ([], []), 0
    while True:
        got = ra.next_pair(rb, batch)
        if got is None:
            break
        d1, d2, f = got
        assert f == first and not d1.has_qual and not d2.has_qual and d1.info()[0] == d2.info()[0]
        for m, d in enumerate((d1, d2)):
            t, o = d.get()
            texts[m].append(t); lens[m].extend(np.diff(o.astype(np.int64)).tolist())
        first += d1.info()[0]
        d1.close(); d2.close()
    return [np.concatenate(t).tobytes() if t else b"" for t in texts], lens, first


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_next_pair_in_batches_against_the_whole_file(ctx, fmt):
    from lime_amd import _lib, api
    r1, r2 = _collection(104, 300)
    data = {"fasta": V.fasta_of, "fastq": V.fastq_of}[fmt]
    w1, w2, _, w_info = V.cut_model(r1, r2, 30, 10, insert=V.insert_masks)
    parse = ctx.docs_from_bytes if fmt == "fasta" else ctx.docs_from_fastq_bytes
    whole = (parse(data(r1)), parse(data(r2)))
    o1, o2, info = ctx.docs_trim_overlap(*whole)
    assert info == w_info and o1.get()[0].tobytes() == b"".join(w1) and o2.get()[0].tobytes() == b"".join(w2)
    for x in whole + (o1, o2):
        x.close()
    for batch in (1, 7, 64):
        n = len(r1) if batch > 1 else 40
        ra, rb = ctx.seq_reader_bytes(data(r1[:n]), fmt, window_bytes=0 if batch > 1 else 700), ctx.seq_reader_bytes(data(r2[:n]), fmt)
        assert ra.overlap_info() == {k: 0 for k in V.INFO_KEYS}
        ra.set_overlap(rb)                                                    # (the defaults: 30, 10)
        texts, lens, first = _pair_batches(ra, rb, batch)
        assert first == n and lens[0] == [len(x) for x in w1[:n]] and lens[1] == [len(x) for x in w2[:n]]
        assert texts == [b"".join(w1[:n]), b"".join(w2[:n])]
        want = w_info if n == len(r1) else V.cut_model(r1[:n], r2[:n], 30, 10, insert=V.insert_masks)[3]
        assert ra.overlap_info() == want and rb.overlap_info() == want
        ra.close(); rb.close()


def test_set_overlap_refusals_and_next_on_a_linked_reader_alone(ctx):
    from lime_amd import _lib, api
    r1, r2 = _collection(105, 50)
    other = api.Context(0)
    try:
        ra, rb, rc = ctx.seq_reader_bytes(V.fastq_of(r1), "fastq"), ctx.seq_reader_bytes(V.fasta_of(r2), "fasta"), ctx.seq_reader_bytes(V.fasta_of(r2), "fasta")
        rd = other.seq_reader_bytes(V.fasta_of(r2), "fasta")
        for x, y, O, E, word in ((ra, rb, 0, 10, "overlap"), (ra, rb, 30, 51, "0 .. 50"), (ra, ra, 30, 10, "one reader"), (ra, rd, 30, 10, "different contexts")):
            with pytest.raises(api.LimeError) as e:
                x.set_overlap(y, O, E)
            assert e.value.code == _lib.ERR_ARG and word in str(e.value) and "lime_seq_reader_set_overlap:" in str(e.value)
        with pytest.raises(api.LimeError) as e:                                # not linked yet
            ra.next_pair(rb, 5)
        assert e.value.code == _lib.ERR_ARG and "not linked" in str(e.value)
        ra.set_overlap(rb, 30, 10)                                            # a FASTQ and a FASTA reader
        for x, y in ((ra, rc), (rc, rb)):
            with pytest.raises(api.LimeError) as e:
                x.set_overlap(y, 30, 10)
            assert e.value.code == _lib.ERR_ARG and "linked already" in str(e.value)
        with pytest.raises(api.LimeError) as e:
            ra.next_pair(rc, 5)
        assert e.value.code == _lib.ERR_ARG and "not linked" in str(e.value)
        b = ra.next(3)                                                        # alone: the uncut batch
        assert b[0].get()[0].tobytes() == b"".join(r1[:3])
        b[0].close()
        b = rb.next(3)
        b[0].close()
        w1, w2, _, _ = V.cut_model(r1[3:10], r2[3:10], 30, 10)
        d1, d2, first = rb.next_pair(ra, 7)                                   # (in either order: the rule is symmetric)
        assert first == 3 and d1.get()[0].tobytes() == b"".join(w2) and d2.get()[0].tobytes() == b"".join(w1)
        d1.close(); d2.close()
        re, rf = ctx.seq_reader_bytes(V.fasta_of(r1), "fasta"), ctx.seq_reader_bytes(V.fasta_of(r2), "fasta")
        x = re.next(2)
        x[0].close()
        with pytest.raises(api.LimeError) as e:                                # after a next of either
            rf.set_overlap(re, 30, 10)
        assert e.value.code == _lib.ERR_ARG and "before the first" in str(e.value)
        rg, rh = ctx.seq_reader_bytes(V.fasta_of(r1), "fasta"), ctx.seq_reader_bytes(V.fasta_of(r2), "fasta")
        rg.set_overlap(rh)
        rg.close()                                                            # closing one unlinks the other
        rh.set_overlap(rc)
        for r in (ra, rb, rc, re, rf, rh, rd):
            r.close()
    finally:
        other.close()


def test_readers_with_different_record_counts(ctx):
    from lime_amd import _lib, api
    r1, r2 = _collection(106, 20)
    ra, rb = ctx.seq_reader_bytes(V.fasta_of(r1), "fasta"), ctx.seq_reader_bytes(V.fasta_of(r2[:17]), "fasta")
    ra.set_overlap(rb, 30, 10)
    for _ in range(2):
        d1, d2, _ = ra.next_pair(rb, 7)
        d1.close(); d2.close()
    with pytest.raises(api.LimeError) as e:
        ra.next_pair(rb, 7)
    assert e.value.code == _lib.ERR_ARG and "different numbers of reads" in str(e.value) and "6" in str(e.value) and "3" in str(e.value)
    assert ra.overlap_info()["n_pairs"] == 14
    ra.close(); rb.close()


def test_the_chain_quality_adapter_filter_overlap(ctx):
    """set_trim + set_adapter + set_filter on each reader and set_overlap over both: the models composed in that order, in batches; the overlap
    cut is last, so --min-len has judged the reads before it"""
    r1, r2 = _collection(107, 400, top=140, kit=False)
    rng = np.random.default_rng([V.SEED, 15])
    quals = [[T.sample_quals(rng, len(r)) for r in rs] for rs in (r1, r2)]
    p = F.params(min_len=60, max_len=125)
    staged, infos = [], []
    for rs, q, ad in zip((r1, r2), quals, (V.TRUSEQ_R1, V.TRUSEQ_R2)):
        x, qi = T.trim_model(rs, q, 0, 20)
        x, ai = A.trim_model(x, ad, 3, 10)
        x, fi = F.filter_model(x, p)
        staged.append(x); infos.append((qi, ai, fi))
    w1, w2, w_ins, w_info = V.cut_model(staged[0], staged[1], 30, 10, insert=V.insert_masks)
    assert w_info["n_cut"] > 50 and infos[0][2]["n_short"] > 0 and infos[0][0]["n_changed"] > 50
    assert min(len(x) for x in w1 if x) < 60                                  # the floor behind the cut is O, not --min-len
    assert (w1, w2) != V.cut_model(r1, r2, 30, 10, insert=V.insert_masks)[:2]  # (the stages in front show)
    for batch in (7, 4096):
        readers = [ctx.seq_reader_bytes(T.fastq_of(rs, q), "fastq") for rs, q in zip((r1, r2), quals)]
        for r, ad in zip(readers, (V.TRUSEQ_R1, V.TRUSEQ_R2)):
            r.set_filter(min_len=60, max_len=125)
            r.set_adapter(ad, 3, 10)
            r.set_trim(0, 20)
        readers[0].set_overlap(readers[1], 30, 10)
        texts, lens, first = _pair_batches(readers[0], readers[1], batch)
        assert first == len(r1) and texts == [b"".join(w1), b"".join(w2)]
        assert lens[0] == [len(x) for x in w1] and lens[1] == [len(x) for x in w2]
        assert readers[0].overlap_info() == w_info
        for r, (qi, ai, fi) in zip(readers, infos):
            assert r.trim_info() == qi and r.adapter_info() == ai and r.filter_info() == fi
            r.close()
