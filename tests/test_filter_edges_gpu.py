"""The device read filter (lime_docs_filter_dev, lime_seq_reader_set_filter; lime_filter_kernel.hip) against lime_read_filter and the models
of tests/filter_cases.py: text, doc_off and every info field exactly equal.  Read lengths around the kernel's word (64) and its multiples,
every tail length of a read that spans three words, the mismatch thresholds, the cap, the N count and the complexity on and next to their
thresholds and on the word edges, collections around a workgroup's 4 reads and past the grid cap, documents of every origin, the reader in
batches and behind both trims.  tests/test_filter_cases_cpu.py holds lime_read_filter against the models."""
import gc

import numpy as np
import pytest

from tests import adapter_cases as A
from tests import filter_cases as F
from tests import trim_cases as T

pytestmark = pytest.mark.gpu

P = F.params
ALL = P(F.G_, max_len=200, min_len=20, max_n=3, min_complexity=30)          # every step at once


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
    text, off = F.records(reads)
    t = torch.from_numpy(text).cuda() if len(text) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    return ctx.docs_from_arrays_dev(t, torch.from_numpy(off.astype(np.int64)).cuda(), len(reads), len(text), stream=stream)


def _check(ctx, reads, plist, what, d=None, stream=None, model=True):
    """the documents `d` (default: made from `reads` as arrays) filtered with every parameter set of plist: against lime_read_filter, and
    (model=True) against both numpy models"""
    from lime_amd import api
    text, off = F.records(reads)
    own = d is None
    if own:
        d = _docs(ctx, reads, stream)
    for p in plist:
        w_text, w_off, w_info = api.read_filter(text, off, **p)
        if model:
            for keep in (F.keep_loop, F.keep_words):
                m_reads, m_info = F.filter_model(reads, p, keep=keep)
                assert m_info == w_info and np.array_equal(F.records(m_reads)[1], w_off), (what, p, keep.__name__)
        out, info = ctx.docs_filter(d, stream=stream, **p)
        o_text, o_off = out.get()
        assert not out.has_qual and out.info() == (len(reads), int(w_off[-1])), (what, p)
        if not np.array_equal(o_off, w_off):
            bad = int(np.nonzero(o_off != w_off)[0][0]) - 1
            raise AssertionError(f"{what}, {p}: read {bad} of {int(off[bad + 1] - off[bad])} symbols keeps {int(o_off[bad + 1] - o_off[bad])}, "
                                 f"not {int(w_off[bad + 1] - w_off[bad])}")
        assert np.array_equal(o_text, w_text), (what, p)
        assert info == w_info, (what, p, info, w_info)
        out.close()
    if own:
        d.close()


LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 130, 255, 256)


@pytest.mark.parametrize("Tmin", [1, 10, 64, 255])
def test_read_lengths(ctx, Tmin):
    """per length (T - 1, T and T + 1 among them): random bases, only G, only N, a G tail of T - 1, T and T + 1 behind G-free bases, one miss
    in the tail, lower case"""
    rng = np.random.default_rng([F.SEED, 5, Tmin])
    reads = []
    for L in sorted(set(LENGTHS) | {Tmin - 1, Tmin, Tmin + 1}):
        reads += [F.bases(rng, L), b"G" * L, b"N" * L, F.bases(rng, L).lower()]
        for t in (Tmin - 1, Tmin, Tmin + 1):
            if 0 < t <= L:
                reads.append(F.no_tail(rng, L - t) + b"G" * t)
                if t >= 9:
                    reads.append(F.no_tail(rng, L - t) + b"GGGGA" + b"G" * (t - 5))
    _check(ctx, reads, (P(F.G_, polyx_min=Tmin), P(15, polyx_min=Tmin), P(F.G_, polyx_min=Tmin, max_len=100, min_len=Tmin, max_n=0, min_complexity=20),
                        P(max_n=0), P(min_complexity=50), P(min_len=64), P(max_len=64)), f"lengths at T = {Tmin}")


def test_one_long_read_among_short_ones(ctx):
    """70 001 symbols are 1094 words, the last one from 69 952 on: random bases (the walk leaves after a few words), only G (it reaches word
    0), a G tail of 40 000 with one miss in nine and a shorter one in eight (the longest admissible tail is found words further down than
    the first inadmissible one); the forward pass over all of it for the N's and the complexity"""
    rng = np.random.default_rng([F.SEED, 6])
    body = F.no_tail(rng, F.LONG)
    ninth = bytearray(b"G" * 40_000)
    ninth[4::9] = b"A" * len(ninth[4::9])
    eighth = bytearray(b"G" * 40_000)
    eighth[7::8] = b"A" * len(eighth[7::8])                                  # exactly one in eight at every multiple of 8
    with_n = bytearray(body)
    with_n[0] = with_n[63] = with_n[64] = with_n[69_951] = with_n[69_952] = with_n[F.LONG - 1] = ord("N")
    short = [F.bases(rng, 5), b"", F.bases(rng, 300)]
    reads = [body, b"G" * F.LONG, body[:30_001] + bytes(ninth), body[:30_001] + bytes(eighth), bytes(with_n), b"AC" * 35_000 + b"A", b"A" * 35_000 + body[:35_001]]
    p = P(F.G_)
    assert [F.keep_loop(r, p)[0] for r in reads[:4]] == [F.LONG, 0, 30_001, 30_001]
    for k, r in enumerate(reads):
        _check(ctx, [r] + short + [r[:4097], r[-4097:]], (p, P(F.G_, max_n=5, min_complexity=50), P(max_n=6), P(min_complexity=51), P(15, polyx_min=255, max_len=70_000)),
               f"long read {k}", model=False)
    assert F.keep_words(reads[3], p) == F.keep_loop(reads[3], p) and F.keep_words(reads[4], P(max_n=5)) == (0, {"n_many_n"})
    assert F.keep_words(reads[4], P(max_n=6))[0] == F.LONG and F.keep_words(reads[6], P(min_complexity=51)) == F.keep_loop(reads[6], P(min_complexity=51))


@pytest.mark.parametrize("name", sorted(F.hand_cases()))
def test_the_hand_made_cases(ctx, name):
    reads, p = F.hand_cases()[name]
    _check(ctx, reads, (p,), name)


def test_the_trap(ctx):
    front = b"ACT" * 23 + b"AC"
    reads = [F.TRAP, b"ACTA" + F.TRAP, b"G" + front[:70] + F.TRAP, b"G" + front + F.TRAP, F.TRAP[::-1], F.TRAP + b"A"]
    assert [F.keep_loop(r, P(F.G_))[0] for r in reads] == [0, 4, 0, 72, 0, 0]            # (the last: the A at the end is one miss more)
    _check(ctx, reads, (P(F.G_), P(15), P(F.G_, polyx_min=255)), "the trap")


@pytest.mark.parametrize("mask", [F.A_, F.C_, F.G_, F.T_, 15])
def test_every_tail_length_on_a_read_of_130(ctx, mask):
    rng = np.random.default_rng([F.SEED, 7, mask])
    X = b"G" if mask == 15 else bytes([b"ACGT"[mask.bit_length() - 1]])
    reads = [F.no_tail(rng, 130 - t, X) + X * t for t in range(1, 131)]
    reads += [F.plant(rng, F.no_tail(rng, 130, X), t, X, 0.1) for t in range(1, 131)]
    p1 = P(mask, polyx_min=1)
    if mask != 15:
        assert [F.keep_loop(r, p1)[0] for r in reads[:130]] == [130 - t for t in range(1, 131)]
    _check(ctx, reads, (p1, P(mask), P(mask, polyx_min=64), P(mask, polyx_min=65)), f"every tail length, mask {mask}")


def test_the_mismatch_thresholds(ctx):
    cases = F.threshold_cases()
    assert len(cases) >= 100
    _check(ctx, [c[0] for c in cases], (P(F.G_, polyx_min=5), P(15, polyx_min=5), P(F.G_, polyx_min=5, max_n=0, min_complexity=10)), "thresholds")


def test_the_cap(ctx):
    """K = hi - 1, hi and hi + 1 for reads with and without a tail, hi on and next to the word edges"""
    rng = np.random.default_rng([F.SEED, 8])
    reads, plist = [], []
    for hi in (1, 2, 63, 64, 65, 127, 128, 129, 200):
        reads += [F.no_tail(rng, hi), F.no_tail(rng, hi) + b"G" * 30]
        plist += [P(F.G_, max_len=K) for K in (hi - 1, hi, hi + 1) if K]
    want = F.filter_model(reads, P(F.G_, max_len=64))[1]
    assert want["n_capped"] == 2 * 5 and want["n_polyx"] == 9            # hi of 65, 127, 128, 129, 200: one more than K and more
    _check(ctx, reads, plist + [P(max_len=1), P(max_len=64, min_len=64), P(max_len=63, min_len=64)], "the cap")


def test_n_counts(ctx):
    """max_n - 1, max_n and max_n + 1 N's; N's at bits 0 and 63 of a word; an N just below hi, which counts, and N's at hi and behind it (in
    the tail that is cut, behind the cap), which do not"""
    rng = np.random.default_rng([F.SEED, 9])

    def with_n(L, places):
        b = bytearray(F.no_tail(rng, L))
        for q in places:
            b[q] = ord("N") if q % 2 else ord("n")
        return bytes(b)

    reads = []
    for k in (2, 3, 4):
        reads += [with_n(150, range(10, 10 + k)), with_n(150, [0, 63, 64, 127, 128][:k]), with_n(150, [63, 64, 127, 128][:k]), with_n(150, [149 - 64 * i for i in range(k)])]
    edge = []
    for hi in (64, 100, 128, 129):
        edge += [with_n(hi, [1, 5, 9, hi - 1]) + b"G" * 30, with_n(hi, [1, 5, 9]) + b"GN" + b"G" * 28]       # the tail cut puts hi where the cap would
        edge += [with_n(hi + 22, [1, 5, 9, at]) for at in (hi - 1, hi, hi + 1)]
    p = P(F.G_, max_n=3)
    assert [F.keep_loop(r, p)[0] for r in edge[:2]] == [0, 64]              # an N at hi - 1 is the fourth; one inside the tail is cut with it
    assert [F.keep_loop(r, P(max_len=64, max_n=3))[0] for r in edge[2:5]] == [0, 64, 64]         # at hi and behind it: behind the cap
    _check(ctx, reads + edge, (p, P(max_n=3), P(max_n=2), P(max_n=4), P(max_n=0)) + tuple(P(max_len=hi, max_n=3) for hi in (64, 100, 128, 129)), "N counts")


def _with_d(rng, n, places):
    """n symbols that change class exactly behind each place j of `places` (s[j] != s[j + 1]) and nowhere else"""
    b, cur = bytearray(), 0
    for j in range(n):
        b.append(b"ACGTN"[cur])
        if j in places:
            cur = (cur + 1 + int(rng.integers(0, 4))) % 5
    return bytes(b)


def test_complexity(ctx):
    """100 d = C (n - 1) exactly and one pair fewer; the differing pairs on the word boundaries (63 | 64, 127 | 128); a differing pair at
    n - 1 | n, behind the cap or the tail cut, which does not count; N N is an equal pair"""
    rng = np.random.default_rng([F.SEED, 10])
    reads = []
    for n, C in ((101, 30), (129, 25), (65, 50), (201, 7), (2, 100), (3, 50)):
        d = C * (n - 1) // 100
        assert 100 * d == C * (n - 1)
        for k in (d, d - 1):
            edges = list(dict.fromkeys(q for q in (63, 127, 0, n - 2, 64, 62) if 0 <= q < n - 1))[:max(k, 0)]
            places = set(edges) | set(int(x) for x in rng.choice([q for q in range(n - 1) if q not in edges], size=k - len(edges), replace=False))
            r = _with_d(rng, n, places)
            assert sum(F.classes(r)[j] != F.classes(r)[j + 1] for j in range(n - 1)) == k
            assert (F.keep_loop(r, P(min_complexity=C))[0] == n) == (k == d), (n, C, k)
            reads.append(r)
            # the same kept part with another class behind it: the pair n - 1 | n differs and must not count (cap), and a G tail behind a
            # part that ends in another class
            last = F.classes(r)[-1]
            reads.append(r + b"ACGTN"[(last + 1) % 5:(last + 1) % 5 + 1] * 30)
            if last != 2:
                reads.append(r + b"G" * 30)
    reads += [b"N" * 100, b"NA" * 50, b"n" * 64 + b"N" * 64, b"-" * 64 + b"N" * 64 + b"A"]
    plist = [P(min_complexity=C) for C in (30, 25, 50, 7, 100, 1)]
    plist += [P(max_len=n, min_complexity=C) for n, C in ((101, 30), (129, 25), (65, 50), (201, 7), (2, 100), (3, 50), (64, 50), (128, 25))]
    plist += [P(F.G_, min_complexity=C) for C in (30, 25, 50, 7)]
    _check(ctx, reads, plist, "complexity")


def _collection(seed, n, top=130):
    rng = np.random.default_rng([F.SEED, 11, seed])
    return [F.fuzz_read(rng, int(L)) for L in rng.integers(0, top, size=n)]


@pytest.mark.parametrize("n", list(range(1, 66)))
def test_collections_of_1_to_65_reads(ctx, n):
    _check(ctx, _collection(n, n), (ALL,), f"{n} reads")


@pytest.mark.parametrize("n", [F.READS_PER_TRIP + 1, 2 * F.READS_PER_TRIP + 3], ids=["8193 reads", "16387 reads"])
def test_many_reads(ctx, n):
    """whoever changes RD_BLOCKS or RD_WAVES in lime_reads.h changes filter_cases.READS_PER_TRIP: one read more than a trip of the
    capped grid, and three more than two trips.  The numpy model on the first and last 300 reads, lime_read_filter on all"""
    from lime_amd import api
    assert F.READS_PER_TRIP == 8192
    reads = _collection(n, n, top=90)
    p = P(F.G_, min_len=15, max_n=2, min_complexity=30)
    _check(ctx, reads, (p, P(F.G_ | F.A_, polyx_min=5)), f"{n} reads", model=False)
    w_off = api.read_filter(*F.records(reads), **p)[1]
    for sl in (slice(0, 300), slice(n - 300, n)):
        m = F.filter_model(reads[sl], p, keep=F.keep_words)[0]
        assert [len(x) for x in m] == list(np.diff(w_off.astype(np.int64))[sl])


def test_every_read_empty_and_no_read(ctx):
    _check(ctx, [b""] * 70, (ALL, P(min_len=1)), "70 empty reads")
    _check(ctx, [], (ALL,), "no read")


def test_documents_of_every_origin(ctx):
    """a FASTA parse, a FASTQ parse without and with qualities, the output of either trim: the filter takes each, and its output holds no
    qualities"""
    reads = _collection(101, 900, top=150)
    rng = np.random.default_rng([F.SEED, 12])
    quals = [T.sample_quals(rng, len(r)) for r in reads]
    fq = T.fastq_of(reads, quals)
    plist = (ALL, P(F.G_))
    for d in (ctx.docs_from_bytes(F.fasta_of(reads)), ctx.docs_from_fastq_bytes(fq), ctx.docs_from_fastq_qual_bytes(fq)):
        _check(ctx, reads, plist, "parsed documents", d=d)
        d.close()
    d = ctx.docs_from_fastq_qual_bytes(fq)
    cut, _ = ctx.docs_trim(d, 5, 20)
    q_reads = T.trim_model(reads, quals, 5, 20)[0]
    _check(ctx, q_reads, plist, "the quality trim's output", d=cut)
    ad, _ = ctx.docs_trim_adapter(cut, A.TRUSEQ_R1[:20], 3, 10)
    _check(ctx, A.trim_model(q_reads, A.TRUSEQ_R1[:20], 3, 10)[0], plist, "the adapter trim's output", d=ad)
    ad.close(); cut.close(); d.close()


def test_text_at_offsets_that_are_no_multiples_of_64(ctx):
    """reads of 1 .. 63 symbols in front push every later read off the 64-byte lines, and the arrays themselves come from views at odd addresses"""
    import torch
    rng = np.random.default_rng([F.SEED, 13])
    for shift in (1, 7, 63):
        reads = [F.bases(rng, shift)] + [F.fuzz_read(rng, 100) for _ in range(64)] + [F.bases(rng, 200) + b"G" * 70]
        text, off = F.records(reads)
        raw = torch.zeros(len(text) + 128, dtype=torch.uint8, device="cuda")
        view = raw[shift:shift + len(text)]
        view.copy_(torch.from_numpy(text))
        d = ctx.docs_from_arrays_dev(view, torch.from_numpy(off.astype(np.int64)).cuda(), len(reads), len(text))
        _check(ctx, reads, (ALL,), f"shift {shift}", d=d)
        d.close()


def test_side_stream(ctx):
    import torch
    reads = _collection(102, 5000, top=120)
    text, off = F.records(reads)
    src = torch.from_numpy(text).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    late = torch.zeros(src.numel(), dtype=torch.uint8, device="cuda")       # not the input yet
    filler = torch.rand(8_000_000, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):                                              # best effort, as in tests/test_fastq_edges_gpu.py
        for _ in range(3):
            filler = torch.sort(filler.flip(0))[0]
        late.copy_(src.flip(0).flip(0))
        d = ctx.docs_from_arrays_dev(late, torch.from_numpy(off.astype(np.int64)).cuda(), len(reads), len(text), stream=s.cuda_stream)
        _check(ctx, reads, (ALL, P(15, polyx_min=5)), "side stream", d=d, stream=s.cuda_stream, model=False)
        d.close()
    s.synchronize()
    torch.cuda.synchronize()


def test_seeded_collections(ctx):
    for case in range(200):
        reads, p = F.fuzz_collection(F.SEED, case)
        _check(ctx, reads, (p,), f"fuzz_collection({F.SEED}, {case})", model=case % 4 == 0)


def _free_bytes():
    import torch
    from lime_amd import api
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


REFUSED = [(dict(polyx=16), "poly-X mask"), (dict(polyx=F.G_, polyx_min=0), "1 .. 255"), (dict(polyx=F.G_, polyx_min=256), "1 .. 255"),
           (dict(min_len=1, min_complexity=101), "0 .. 100"), (dict(), "nothing asked")]


def test_refusals_and_device_memory_comes_back(ctx):
    """every refusal comes before any launch, with a text; after filters and refusals of each kind and lime_trim_cache the device's free memory
    is what it was"""
    import ctypes as C
    from lime_amd import _lib, api
    reads = _collection(103, 3000, top=200)
    other = api.Context(0)

    def cycle():
        d = _docs(ctx, reads)
        out, info = ctx.docs_filter(d, **ALL)
        assert info["n_polyx"] > 0 and info["n_low_complexity"] > 0
        for kw, word in REFUSED:
            with pytest.raises(api.LimeError) as e:
                ctx.docs_filter(d, **P(**kw))
            assert e.value.code == _lib.ERR_ARG and word in str(e.value) and "lime_docs_filter_dev:" in str(e.value)
        with pytest.raises(api.LimeError) as e:
            other.docs_filter(d, **ALL)
        assert e.value.code == _lib.ERR_ARG and "another context" in str(e.value)
        f = _lib.Filter(4, 10, 0, 0, _lib.FILTER_OFF, 0)
        h, fi = C.c_void_p(1), _lib.FilterInfo(7, 7, 7, 7, 7, 7, 7, 7)
        for args in ((None, d.h, C.byref(f)), (ctx.h, None, C.byref(f)), (ctx.h, d.h, None)):
            assert ctx.lib.lime_docs_filter_dev(*args, None, C.byref(h), C.byref(fi)) == _lib.ERR_ARG
            assert h.value is None and fi.n_reads == 0 and "NULL" in ctx.lib.lime_last_error().decode()
            h, fi = C.c_void_p(1), _lib.FilterInfo(7, 7, 7, 7, 7, 7, 7, 7)
        assert ctx.lib.lime_docs_filter_dev(ctx.h, d.h, C.byref(f), None, None, None) == _lib.ERR_ARG
        for x in (d, out):
            x.close()

    try:
        cycle()
        before = _free_bytes()
        cycle()
        assert _free_bytes() == before
    finally:
        other.close()


# ---- the reader ----
def _batches(r, batch):
    texts, lens, first = [], [], 0
    while True:
        b = r.next(batch)
        if b is None:
            break
        d, f = b
        assert f == first and not d.has_qual
        t, o = d.get()
        texts.append(t); lens.extend(np.diff(o.astype(np.int64)).tolist())
        first += d.info()[0]
        d.close()
    return (np.concatenate(texts).tobytes() if texts else b""), lens, first


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_reader_batches_against_the_whole_file(ctx, fmt):
    from lime_amd import _lib, api
    reads = _collection(104, 5000)
    data = {"fasta": F.fasta_of, "fastq": F.fastq_of}[fmt]
    want, w_info = F.filter_model(reads, ALL)
    whole = ctx.docs_from_bytes(data(reads)) if fmt == "fasta" else ctx.docs_from_fastq_bytes(data(reads))
    assert whole.get()[0].tobytes() == b"".join(reads)                      # (the parser hands the symbols on as they are)
    out, info = ctx.docs_filter(whole, **ALL)
    assert info == w_info and out.get()[0].tobytes() == b"".join(want)
    out.close(); whole.close()
    for batch in (1, 7, 4096):
        n = len(reads) if batch > 1 else 40
        r = ctx.seq_reader_bytes(data(reads[:n]), fmt, window_bytes=0 if batch > 1 else 700)
        assert r.filter_info() == {k: 0 for k in w_info}
        r.set_filter(**ALL)
        text, lens, first = _batches(r, batch)
        assert first == n and lens == [len(x) for x in want[:n]] and text == b"".join(want[:n])
        assert r.filter_info() == (w_info if n == len(reads) else F.filter_model(reads[:n], ALL)[1])
        assert r.trim_info()["n_reads"] == 0 and r.adapter_info()["n_reads"] == 0
        with pytest.raises(api.LimeError) as e:                              # after the first batch: refused
            r.set_filter(**ALL)
        assert e.value.code == _lib.ERR_ARG and "before the first" in str(e.value)
        r.close()


def test_set_filter_after_the_first_next_and_with_bad_values_is_refused(ctx):
    from lime_amd import _lib, api
    reads = [F.bases(np.random.default_rng([F.SEED, 14, k]), 40 + k) for k in range(50)]
    r = ctx.seq_reader_bytes(F.fastq_of(reads), "fastq")
    for kw, word in REFUSED:
        with pytest.raises(api.LimeError) as e:
            r.set_filter(**P(**kw))
        assert e.value.code == _lib.ERR_ARG and word in str(e.value) and "lime_seq_reader_set_filter:" in str(e.value)
    b = r.next(3)
    assert b is not None and b[0].info()[0] == 3                            # (the refusals left the reader as it was)
    assert b[0].get()[0].tobytes() == b"".join(reads[:3])
    b[0].close()
    with pytest.raises(api.LimeError) as e:
        r.set_filter(**ALL)
    assert e.value.code == _lib.ERR_ARG and "before the first" in str(e.value)
    assert r.filter_info()["n_reads"] == 0
    r.close()


def test_quality_trim_then_adapter_trim_then_filter(ctx):
    """set_trim + set_adapter + set_filter: the quality model's output through the adapter model and that through the filter model, in batches"""
    rng = np.random.default_rng([F.SEED, 15])
    a20 = A.TRUSEQ_R1[:20]
    reads = []
    for k in range(3000):
        L = int(rng.integers(0, 140))
        r = F.fuzz_read(rng, L)
        if L > 40 and k % 3 == 0:                                           # read-through, then the instrument's G's
            r = (r[:int(rng.integers(10, L - 25))] + a20 + b"G" * L)[:L]
        reads.append(r)
    quals = [T.sample_quals(rng, len(r)) for r in reads]
    q_reads, q_info = T.trim_model(reads, quals, 5, 20)
    a_reads, a_info = A.trim_model(q_reads, a20, 3, 10)
    want, w_info = F.filter_model(a_reads, ALL)
    assert w_info["n_polyx"] > 100 and a_info["n_changed"] > 500 and q_info["n_changed"] > 500
    assert want != F.filter_model(reads, ALL)[0] and want != F.filter_model(q_reads, ALL)[0]       # (the order shows)
    for batch in (7, 4096):
        r = ctx.seq_reader_bytes(T.fastq_of(reads, quals), "fastq")
        r.set_filter(**ALL)                                                 # (in any order of the three calls)
        r.set_adapter(a20, 3, 10)
        r.set_trim(5, 20)
        text, lens, first = _batches(r, batch)
        assert first == len(reads) and lens == [len(x) for x in want] and text == b"".join(want)
        assert r.trim_info() == q_info and r.adapter_info() == a_info and r.filter_info() == w_info
        assert r.filter_info()["symbols_in"] == a_info["symbols_out"]
        r.close()
