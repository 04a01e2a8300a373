"""The device adapter trim (lime_docs_trim_adapter_dev, lime_seq_reader_set_adapter; lime_adapter_kernel.hip) against lime_adapter_trim and the
models of tests/adapter_cases.py: text, doc_off and every info field exactly equal.  Read lengths around the kernel's word (64) and its
multiples, every adapter length around 32 and 64, the adapter at every start of a read that spans three words, the mismatch thresholds,
collections around a workgroup's 4 reads and past the grid cap, documents of every origin, the reader in batches.
tests/test_adapter_cases_cpu.py holds lime_adapter_trim against the models."""
import gc

import numpy as np
import pytest

from tests import adapter_cases as A
from tests import trim_cases as T

pytestmark = pytest.mark.gpu

A20 = A.TRUSEQ_R1[:20]


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
    text, off = A.records(reads)
    t = torch.from_numpy(text).cuda() if len(text) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    return ctx.docs_from_arrays_dev(t, torch.from_numpy(off.astype(np.int64)).cuda(), len(reads), len(text), stream=stream)


def _check(ctx, reads, params, what, d=None, stream=None, model=True):
    """the documents `d` (default: made from `reads` as arrays) cut with every (adapter, O, E) of params: against lime_adapter_trim, and
    (model=True) against the numpy model"""
    from lime_amd import api
    text, off = A.records(reads)
    own = d is None
    if own:
        d = _docs(ctx, reads, stream)
    for adapter, O, E in params:
        w_text, w_off, w_info = api.adapter_trim(text, off, adapter, O, E)
        if model:
            m_reads, m_info = A.trim_model(reads, adapter, O, E)
            assert m_info == w_info and np.array_equal(A.records(m_reads)[1], w_off), (what, adapter, O, E)
        out, info = ctx.docs_trim_adapter(d, adapter, O, E, stream=stream)
        o_text, o_off = out.get()
        assert not out.has_qual and out.info() == (len(reads), int(w_off[-1])), (what, adapter, O, E)
        if not np.array_equal(o_off, w_off):
            bad = int(np.nonzero(o_off != w_off)[0][0]) - 1
            raise AssertionError(f"{what}, adapter {adapter} overlap {O} error {E}: read {bad} of {int(off[bad + 1] - off[bad])} symbols is cut to "
                                 f"{int(o_off[bad + 1] - o_off[bad])}, not {int(w_off[bad + 1] - w_off[bad])}")
        assert np.array_equal(o_text, w_text), (what, adapter, O, E)
        assert info == w_info, (what, adapter, O, E, info, w_info)
        out.close()
    if own:
        d.close()


def _lengths(M, O):
    return sorted({0, 1, max(O - 1, 0), O, M - 1, M, M + 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4097})


@pytest.mark.parametrize("M", A.ADAPTER_LENGTHS)
def test_read_lengths_at_each_adapter_length(ctx, M):
    """per length: a read without the adapter, one that ends in the whole adapter, one that ends in O of its symbols, one in O - 1, and one that
    is the adapter's start"""
    rng = np.random.default_rng([A.SEED, 5, M])
    a = A.bases(rng, M)
    for O in sorted({1, min(3, M), M}):
        reads = []
        for L in _lengths(M, O):
            reads.append(A.bases(rng, L))
            for k in (M, O, O - 1):
                if 0 < k <= L:
                    reads.append(A.bases(rng, L - k) + a[:k])
            reads.append((a + A.bases(rng, L))[:L])
        _check(ctx, reads, ((a, O, 0), (a, O, 10), (a, O, 50), (a.lower(), O, 10)), f"adapter of {M}, overlap {O}")


def test_one_long_read_among_short_ones(ctx):
    """70 001 symbols are 1094 words, the last one from 69 952 on; the adapter nowhere, in its last word, across its last word edge, and at its very end cut to O symbols"""
    rng = np.random.default_rng([A.SEED, 6])
    body = bytearray(A.bases(rng, A.LONG))
    for at in range(A.LONG - 2):                                      # no exact 3-symbol start of the adapter anywhere: no chance hit at E = 0
        if bytes(body[at:at + 3]) == A20[:3]:
            body[at + 2] = body[at + 2:at + 3].translate(A.COMP)[0]
    body = bytes(body)
    short = [A.bases(rng, 5), b"", A.bases(rng, 300)]
    assert A.keep_masks(body[-300:], A20, 3, 0) == 300
    for name, read in (("nowhere", body), ("in the last word", body[:A.LONG - 30] + A20 + body[:10]), ("across the last word edge", body[:69_947] + A20 + body[:34]),
                       ("cut to O at the end", body[:A.LONG - 3] + A20[:3]), ("at 64 000", body[:64_000] + A20 + body[64_020:])):
        assert len(read) == A.LONG
        _check(ctx, [read] + short + [read[:4097], read[-4097:]], ((A20, 3, 0),), f"a long read, the adapter {name}", model=False)
        want = {"nowhere": A.LONG, "in the last word": A.LONG - 30, "across the last word edge": 69_947, "cut to O at the end": A.LONG - 3, "at 64 000": 64_000}[name]
        from lime_amd import api
        assert int(api.adapter_trim(*A.records([read]), A20, 3, 0)[1][1]) == want, name


@pytest.mark.parametrize("name", sorted(A.hand_cases()))
def test_the_hand_made_cases(ctx, name):
    reads, adapter, O, E = A.hand_cases()[name]
    _check(ctx, reads, ((adapter, O, E),), name)


def test_every_start_of_130_at_other_adapter_lengths(ctx):
    rng = np.random.default_rng([A.SEED, 7])
    for M in (1, 33, 64):
        a = A.bases(rng, M)
        body = A.far_from(rng, 130, a, min(3, M), 0) if M > 1 else bytes(A.bases(rng, 130).replace(a, a.translate(A.COMP)))
        reads = [(body[:p] + a + A.bases(rng, 130))[:130] for p in range(130)]
        _check(ctx, reads, ((a, min(3, M), 0), (a, M, 0), (a, min(3, M), 10)), f"every start of 130, adapter of {M}")


def test_the_mismatch_thresholds(ctx):
    cases = A.threshold_cases()
    for E in (0, 10, 50):
        reads = [c[0] for c in cases.values() if c[3] == E]
        assert len(reads) >= 4
        _check(ctx, reads, ((A.TRUSEQ_R1[:30], 3, E),), f"thresholds at {E} percent")


def _collection(seed, n, top=130):
    """n reads of 0 .. top - 1 symbols, two thirds with A20 planted with up to 2 errors"""
    rng = np.random.default_rng([A.SEED, 8, seed])
    reads = []
    for L in rng.integers(0, top, size=n):
        r = A.bases(rng, int(L))
        if L and rng.random() < 0.67:
            r = A.plant(rng, r, int(rng.integers(0, L)), A20, int(rng.integers(0, 3)))
        reads.append(r)
    return reads


@pytest.mark.parametrize("n", list(range(1, 66)))
def test_collections_of_1_to_65_reads(ctx, n):
    _check(ctx, _collection(n, n), ((A20, 3, 10),), f"{n} reads")


@pytest.mark.parametrize("n", [16384 + 5, 6 * A.READS_PER_TRIP + 37], ids=["16389 reads", "49189 reads, past the grid cap"])
def test_many_reads(ctx, n):
    """whoever changes RD_BLOCKS or RD_WAVES in lime_reads.h changes adapter_cases.READS_PER_TRIP: the larger collection takes a
    seventh trip.  The numpy model on the first and last 300 reads, lime_adapter_trim on all"""
    from lime_amd import api
    assert A.READS_PER_TRIP == 8192 and 6 * A.READS_PER_TRIP + 37 == 49189
    reads = _collection(n, n, top=40)
    _check(ctx, reads, ((A20, 3, 10), (A20, 1, 0)), f"{n} reads", model=False)
    w_off = api.adapter_trim(*A.records(reads), A20, 3, 10)[1]
    for sl in (slice(0, 300), slice(n - 300, n)):
        m = A.trim_model(reads[sl], A20, 3, 10)[0]
        assert [len(x) for x in m] == list(np.diff(w_off.astype(np.int64))[sl])


def test_every_read_empty_and_no_read(ctx):
    _check(ctx, [b""] * 70, ((A20, 3, 10),), "70 empty reads")
    _check(ctx, [], ((A20, 3, 10),), "no read")


def test_documents_of_every_origin(ctx):
    """a FASTA parse, a FASTQ parse without and with qualities, the quality trim's output: the adapter trim takes each, and its output holds no
    qualities"""
    reads = _collection(101, 900, top=150)
    rng = np.random.default_rng([A.SEED, 9])
    quals = [T.sample_quals(rng, len(r)) for r in reads]
    fq = T.fastq_of(reads, quals)
    params = ((A20, 3, 10), (A20, 5, 0))
    for d in (ctx.docs_from_bytes(A.fasta_of(reads)), ctx.docs_from_fastq_bytes(fq), ctx.docs_from_fastq_qual_bytes(fq)):
        _check(ctx, reads, params, "parsed documents", d=d)
        d.close()
    d = ctx.docs_from_fastq_qual_bytes(fq)
    cut, _ = ctx.docs_trim(d, 5, 20)
    _check(ctx, T.trim_model(reads, quals, 5, 20)[0], params, "the quality trim's output", d=cut)
    cut.close(); d.close()


def test_text_at_offsets_that_are_no_multiples_of_64(ctx):
    """reads of 1 .. 9 symbols in front push every later read off the 64-byte lines, and the arrays themselves come from views at odd addresses"""
    import torch
    rng = np.random.default_rng([A.SEED, 10])
    for shift in (1, 7, 63):
        reads = [A.bases(rng, shift)] + [A.plant(rng, A.bases(rng, 100), int(rng.integers(20, 101)), A20, 1) for _ in range(64)] + [A.bases(rng, 200) + A20]
        text, off = A.records(reads)
        raw = torch.zeros(len(text) + 128, dtype=torch.uint8, device="cuda")
        view = raw[shift:shift + len(text)]
        view.copy_(torch.from_numpy(text))
        d = ctx.docs_from_arrays_dev(view, torch.from_numpy(off.astype(np.int64)).cuda(), len(reads), len(text))
        _check(ctx, reads, ((A20, 3, 10),), f"shift {shift}", d=d)
        d.close()


def test_side_stream(ctx):
    import torch
    reads = _collection(102, 5000, top=120)
    text, off = A.records(reads)
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
        _check(ctx, reads, ((A20, 3, 10), (A20, 8, 20)), "side stream", d=d, stream=s.cuda_stream)
        d.close()
    s.synchronize()
    torch.cuda.synchronize()


def test_seeded_collections(ctx):
    for case in range(200):
        reads, adapter, O, E = A.fuzz_collection(A.SEED, case)
        _check(ctx, reads, ((adapter, O, E),), f"fuzz_collection({A.SEED}, {case})", model=case % 4 == 0)


def _free_bytes():
    import torch
    from lime_amd import api
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


REFUSED = [(b"", 1, 10, "1 .. 64"), (b"A" * 65, 3, 10, "1 .. 64"), (b"ACGN", 3, 10, "A, C, G and T"), (b"ACGT", 0, 10, "overlap"), (b"ACGT", 5, 10, "overlap"),
           (b"ACGT", 3, 51, "0 .. 50")]


def test_refusals_and_device_memory_comes_back(ctx):
    """every refusal comes before any launch, with a text; after trims and refusals of each kind and lime_trim_cache the device's free memory is
    what it was"""
    import ctypes as C
    import torch
    from lime_amd import _lib, api
    reads = _collection(103, 3000, top=200)
    other = api.Context(0)

    def cycle():
        d = _docs(ctx, reads)
        out, info = ctx.docs_trim_adapter(d, A20, 3, 10)
        assert info["n_changed"] > 0
        for adapter, O, E, word in REFUSED:
            with pytest.raises(api.LimeError) as e:
                ctx.docs_trim_adapter(d, adapter, O, E)
            assert e.value.code == _lib.ERR_ARG and word in str(e.value) and "lime_docs_trim_adapter_dev:" in str(e.value)
        with pytest.raises(api.LimeError) as e:
            other.docs_trim_adapter(d, A20, 3, 10)
        assert e.value.code == _lib.ERR_ARG and "another context" in str(e.value)
        h, ti = C.c_void_p(1), _lib.TrimInfo(7, 7, 7, 7, 7)
        for args in ((None, d.h, A20, 20), (ctx.h, None, A20, 20), (ctx.h, d.h, None, 20)):
            assert ctx.lib.lime_docs_trim_adapter_dev(*args, 3, 10, None, C.byref(h), C.byref(ti)) == _lib.ERR_ARG
            assert h.value is None and ti.n_reads == 0 and "NULL" in ctx.lib.lime_last_error().decode()
            h, ti = C.c_void_p(1), _lib.TrimInfo(7, 7, 7, 7, 7)
        assert ctx.lib.lime_docs_trim_adapter_dev(ctx.h, d.h, A20, 20, 3, 10, None, None, None) == _lib.ERR_ARG
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
    data = {"fasta": A.fasta_of, "fastq": A.fastq_of}[fmt]
    want, w_info = A.trim_model(reads, A20, 3, 10)
    whole = ctx.docs_from_bytes(data(reads)) if fmt == "fasta" else ctx.docs_from_fastq_bytes(data(reads))
    out, info = ctx.docs_trim_adapter(whole, A20, 3, 10)
    assert info == w_info and out.get()[0].tobytes() == b"".join(want)
    out.close(); whole.close()
    for batch in (1, 7, 4096):
        n = len(reads) if batch > 1 else 40
        r = ctx.seq_reader_bytes(data(reads[:n]), fmt, window_bytes=0 if batch > 1 else 700)
        assert r.adapter_info() == {k: 0 for k in w_info}
        r.set_adapter(A20, 3, 10)
        text, lens, first = _batches(r, batch)
        assert first == n and lens == [len(x) for x in want[:n]] and text == b"".join(want[:n])
        assert r.adapter_info() == (w_info if n == len(reads) else A.trim_model(reads[:n], A20, 3, 10)[1])
        assert r.trim_info() == {k: 0 for k in w_info}
        with pytest.raises(api.LimeError) as e:                              # after the first batch: refused
            r.set_adapter(A20, 3, 10)
        assert e.value.code == _lib.ERR_ARG and "before the first" in str(e.value)
        r.close()


def test_set_adapter_after_the_first_next_and_with_bad_values_is_refused(ctx):
    from lime_amd import _lib, api
    data = A.fastq_of(_collection(105, 50))
    r = ctx.seq_reader_bytes(data, "fastq")
    for adapter, O, E, word in REFUSED:
        with pytest.raises(api.LimeError) as e:
            r.set_adapter(adapter, O, E)
        assert e.value.code == _lib.ERR_ARG and word in str(e.value) and "lime_seq_reader_set_adapter:" in str(e.value)
    b = r.next(3)
    assert b is not None and b[0].info()[0] == 3                            # (the refusals left the reader as it was)
    assert b[0].get()[0].tobytes() == b"".join(_collection(105, 50)[:3])
    b[0].close()
    with pytest.raises(api.LimeError) as e:
        r.set_adapter(A20, 3, 10)
    assert e.value.code == _lib.ERR_ARG and "before the first" in str(e.value)
    r.close()


def test_quality_trim_first_and_adapter_trim_second(ctx):
    """set_trim + set_adapter: the quality model's output through the adapter model, in batches"""
    reads = _collection(106, 3000, top=140)
    rng = np.random.default_rng([A.SEED, 11])
    quals = [T.sample_quals(rng, len(r)) for r in reads]
    q_reads, q_info = T.trim_model(reads, quals, 5, 20)
    want, w_info = A.trim_model(q_reads, A20, 3, 10)
    assert w_info["n_changed"] > 500 and q_info["n_changed"] > 500
    assert want != A.trim_model(reads, A20, 3, 10)[0]                       # (the order shows)
    for batch in (7, 4096):
        r = ctx.seq_reader_bytes(T.fastq_of(reads, quals), "fastq")
        r.set_adapter(A20, 3, 10)                                           # (in either order of the two calls)
        r.set_trim(5, 20)
        text, lens, first = _batches(r, batch)
        assert first == len(reads) and lens == [len(x) for x in want] and text == b"".join(want)
        assert r.trim_info() == q_info and r.adapter_info() == w_info
        assert r.adapter_info()["symbols_in"] == q_info["symbols_out"]
        r.close()
