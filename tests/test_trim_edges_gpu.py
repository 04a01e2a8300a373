"""The device quality trim (lime_docs_from_fastq_qual_bytes_dev, lime_docs_trim_dev, lime_seq_reader_set_trim; lime_fqtrim_kernel.hip) against
lime_quality_trim and the models of tests/trim_cases.py: text, doc_off and every info field exactly equal.  Read lengths around the
kernel's lane (16), row step (256) and their multiples, hand-made quality patterns at each, collections around a wave's 4 and a
workgroup's 16 reads and past the grid cap, the quality writer against lime_fastq_read_qual on every input of tests/fastq_cases.py, the
reader in batches.  tests/test_trim_cases_cpu.py holds lime_quality_trim against the models."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import fasta_cases as FC
from tests import fastq_cases as QC
from tests import trim_cases as T

pytestmark = pytest.mark.gpu

PAIRS = ((20, 20), (0, 20), (20, 0), (1, 1), (93, 93), (1, 93), (93, 0), (0, 0))


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


def _to_dev(data):
    import torch
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if len(data) else torch.zeros(0, dtype=torch.uint8, device="cuda")


def _check(ctx, reads, quals, pairs, what, eol=b"\n", t=None, stream=None, model=True):
    """the FASTQ of (reads, quals) parsed with qualities on the device, then trimmed with every cutoff pair: against lime_quality_trim, and
    (model=True) against the numpy model"""
    from lime_amd import api
    text, off = T.records(reads)
    qual, _ = T.records(quals)
    if t is None:
        t = _to_dev(T.fastq_of(reads, quals, eol))
    d = ctx.docs_from_fastq_qual_bytes_dev(t, stream=stream)
    g_text, g_off = d.get()
    assert d.has_qual and d.info() == (len(reads), len(text)), what
    assert np.array_equal(g_off, off) and np.array_equal(g_text, text) and np.array_equal(d.qual, qual), what
    for q5, q3 in pairs:
        w_text, w_off, w_info = api.quality_trim(text, qual, off, q5, q3)
        if model:
            m_reads, m_info = T.trim_model(reads, quals, q5, q3)
            assert m_info == w_info and np.array_equal(T.records(m_reads)[1], w_off), (what, q5, q3)
        out, info = ctx.docs_trim(d, q5, q3, stream=stream)
        o_text, o_off = out.get()
        assert not out.has_qual and out.info() == (len(reads), int(w_off[-1])), (what, q5, q3)
        if not np.array_equal(o_off, w_off):
            bad = int(np.nonzero(o_off != w_off)[0][0]) - 1
            raise AssertionError(f"{what}, cutoffs {q5},{q3}: read {bad} of {int(off[bad + 1] - off[bad])} symbols is cut to "
                                 f"{int(o_off[bad + 1] - o_off[bad])}, not {int(w_off[bad + 1] - w_off[bad])}")
        assert np.array_equal(o_text, w_text), (what, q5, q3)
        assert info == w_info, (what, q5, q3, info, w_info)
        out.close()
    d.close()


@pytest.mark.parametrize("L", T.LENGTHS)
def test_patterns_at_each_length(ctx, L):
    rng = np.random.default_rng([T.SEED, 7, L])
    for cut in (1, 20):
        pats = T.patterns(L, cut)
        names = sorted(pats)
        reads = [T.bases(rng, L) for _ in names]
        _check(ctx, reads, [pats[k] for k in names], ((cut, cut), (0, cut), (cut, 0), (93, 93), (1, 93), (93, 0), (0, 0)), f"patterns of {L} around {cut}")


def test_one_long_read_among_short_ones(ctx):
    """70 001 symbols are 274 steps; the short reads of its wave are done after one.  The long read under every pattern"""
    rng = np.random.default_rng([T.SEED, 8])
    pats = T.patterns(T.LONG, 20)
    for names in (sorted(pats)[0::3], sorted(pats)[1::3], sorted(pats)[2::3]):
        reads, quals = [], []
        for k in names:
            for L in (T.LONG, 5, 0, 300):
                reads.append(T.bases(rng, L))
                quals.append(pats[k] if L == T.LONG else T.fuzz_read(rng, L))
        _check(ctx, reads, quals, ((20, 20), (0, 20), (20, 0)), "a long read")
    noise = rng.integers(T.Q(15), T.Q(26), size=T.LONG, dtype=np.uint8).tobytes()       # sums that wander around 0 for thousands of symbols
    _check(ctx, [T.bases(rng, T.LONG)], [noise], ((20, 20), (21, 19), (19, 21)), "a long noisy read")


def _short_collection(seed, n, top=24):
    """n reads of 0 .. top - 1 symbols over a tie-heavy quality alphabet"""
    rng = np.random.default_rng([T.SEED, 9, seed])
    lens = rng.integers(0, top, size=n)
    offs = np.concatenate([[0], np.cumsum(lens)])
    flat_q = np.array([T.Q(2), T.Q(19), T.Q(20), T.Q(21), T.Q(38)], np.uint8)[rng.integers(0, 5, size=int(offs[-1]))].tobytes()
    flat_r = T.bases(rng, int(offs[-1]))
    return [flat_r[offs[i]:offs[i + 1]] for i in range(n)], [flat_q[offs[i]:offs[i + 1]] for i in range(n)]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65])
def test_collections_around_a_waves_and_a_workgroups_reads(ctx, n):
    reads, quals = _short_collection(n, n, top=40)
    _check(ctx, reads, quals, PAIRS, f"{n} reads")


@pytest.mark.parametrize("n", [16384 + 5, 2 * T.READS_PER_TRIP + 37], ids=["16389 reads", "past the grid cap"])
def test_many_reads(ctx, n):
    """whoever changes TR_BLOCKS or TR_READS in lime_fqtrim_kernel.hip changes trim_cases.READS_PER_TRIP: the larger collection takes a third trip.
    The numpy model on the first and last 300 reads, lime_quality_trim on all"""
    from lime_amd import api
    assert T.READS_PER_TRIP == 24576
    reads, quals = _short_collection(n, n)
    _check(ctx, reads, quals, ((20, 20), (0, 21)), f"{n} reads", model=False)
    text, off = T.records(reads); qual, _ = T.records(quals)
    w_text, w_off, _ = api.quality_trim(text, qual, off, 20, 20)
    for sl in (slice(0, 300), slice(n - 300, n)):
        m = T.trim_model(reads[sl], quals[sl], 20, 20)[0]
        assert [len(x) for x in m] == list(np.diff(w_off.astype(np.int64))[sl])


def test_every_read_empty_and_no_read(ctx):
    _check(ctx, [b""] * 70, [b""] * 70, PAIRS, "70 empty reads")
    _check(ctx, [], [], PAIRS, "no read")


def test_a_crlf_file(ctx):
    reads, quals = _short_collection(1, 200, top=300)
    _check(ctx, reads, quals, PAIRS, "CRLF", eol=b"\r\n")


def test_input_at_every_offset(ctx):
    """the file's bytes at device offsets 0 .. 15 from an aligned allocation, reads long enough for 16-byte loads of qualities at every alignment"""
    import torch
    reads, quals = _short_collection(2, 40, top=90)
    data = T.fastq_of(reads, quals)
    for shift in range(16):
        raw = torch.full((64 + len(data) + 64,), ord("I"), dtype=torch.uint8, device="cuda")
        start = 16 + (-raw.data_ptr()) % 16 + shift
        view = raw[start:start + len(data)]
        view.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
        assert view.data_ptr() % 16 == shift
        _check(ctx, reads, quals, ((20, 20),), f"offset {shift}", t=view)


def test_side_stream(ctx):
    import torch
    reads, quals = _short_collection(3, 5000, top=120)
    src = _to_dev(T.fastq_of(reads, quals))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    late = torch.full((src.numel(),), ord("@"), dtype=torch.uint8, device="cuda")          # not the input yet
    filler = torch.rand(8_000_000, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):                                              # best effort, as in tests/test_fastq_edges_gpu.py
        for _ in range(3):
            filler = torch.sort(filler.flip(0))[0]
        late.copy_(src.flip(0).flip(0))
        _check(ctx, reads, quals, ((20, 20), (5, 30)), "side stream", t=late, stream=s.cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()


def test_seeded_collections(ctx):
    for case in range(200):
        reads, quals, q5, q3 = T.fuzz_collection(T.SEED, case)
        _check(ctx, reads, quals, ((q5, q3), (20, 20)), f"fuzz_collection({T.SEED}, {case})")


# ---- the quality writer ----
def _parse_qual_dev(ctx, t, who="lime_docs_from_fastq_qual_bytes_dev"):
    from lime_amd import _lib
    h = C.c_void_p(1)
    code = ctx.lib.lime_docs_from_fastq_qual_bytes_dev(ctx.h, C.c_void_p(t.data_ptr()), int(t.numel()), None, C.byref(h))
    if code != 0:
        msg = ctx.lib.lime_last_error().decode()
        assert code == _lib.ERR_ARG and h.value is None and msg.startswith(who + ": line "), (code, h.value, msg)
        return QC.refusal_of(msg)
    d = ctx._docs_of(h)
    out = d.get() + (d.qual,)
    d.close()
    return out


def _longer_qualities(api):
    """records whose quality lines hold ten times their sequences' bytes, over several blocks: more quality bytes than the handle has room for"""
    return QC.rec(seq=b"ACGT", qual=b"I" * 40) * (3 * api.FASTA_BLOCK // 50 + 7)


def test_the_quality_writer_on_every_case(ctx, tmp_path):
    """Docs.qual is lime_fastq_read_qual's on every valid input of tests/fastq_cases.py, with the text and doc_off of the plain parse; every
    malformed one is refused with lime_fastq_read's line and reason through the new parse too"""
    from lime_amd import api
    cases = dict(QC.cases(api.FASTA_BLOCK))
    cases["quality lines ten times as long as the sequences"] = _longer_qualities(api)
    for case in range(100):
        cases[f"fuzz_mutated {case}"] = QC.fuzz_mutated(QC.SEED, case, api.FASTA_BLOCK)
    valid = 0
    for name, data in cases.items():
        want = QC.host_read(tmp_path, data)
        got = _parse_qual_dev(ctx, _to_dev(data))
        assert QC.is_refusal(got) == QC.is_refusal(want), (name, got[:2], want)
        if QC.is_refusal(want):
            assert tuple(got) == tuple(want), (name, got, want)
            continue
        text, qual, off = api.fastq_read_qual(str(tmp_path / "in.fastq"))
        assert np.array_equal(got[0], text) and np.array_equal(got[1], off) and np.array_equal(got[2], qual), name
        valid += 1
    assert QC.host_read(tmp_path, cases["quality lines ten times as long as the sequences"]) == (4, 2)
    assert 40 <= valid < len(cases)


def test_front_ends_and_documents_without_qualities(ctx, tmp_path):
    import torch
    from lime_amd import _lib, api
    reads, quals = _short_collection(4, 900, top=150)
    data = T.fastq_of(reads, quals)
    p = str(tmp_path / "in.fastq")
    open(p, "wb").write(data)
    want = T.records(T.trim_model(reads, quals, 20, 20)[0])
    for d in (ctx.docs_from_fastq_qual(p), ctx.docs_from_fastq_qual_bytes(data), ctx.docs_from_fastq_qual_bytes(np.frombuffer(data, np.uint8))):
        assert d.has_qual and np.array_equal(d.qual, T.records(quals)[0])
        out, _ = ctx.docs_trim(d, 20, 20)
        assert np.array_equal(out.get()[0], want[0]) and np.array_equal(out.get()[1], want[1])
        plain = ctx.docs_from_fastq(p)
        rc = d.revcomp()
        again = ctx.docs_from_arrays_dev(torch.from_numpy(T.records(reads)[0]).cuda(), torch.from_numpy(T.records(reads)[1].astype(np.int64)).cuda(),
                                         len(reads), sum(len(r) for r in reads))
        for x in (plain, rc, again, out):                                     # documents without qualities: NULL, and the trim refuses them
            assert not x.has_qual and x.qual_device() is None
            with pytest.raises(api.LimeError) as e:
                ctx.docs_trim(x, 20, 20)
            assert e.value.code == _lib.ERR_ARG and "no qualities" in str(e.value)
            with pytest.raises(api.LimeError) as e:
                x.qual
            assert e.value.code == _lib.ERR_ARG
            x.close()
        for q5, q3 in ((94, 0), (0, 94)):
            with pytest.raises(api.LimeError) as e:
                ctx.docs_trim(d, q5, q3)
            assert e.value.code == _lib.ERR_ARG and "0 .. 93" in str(e.value)
        d.close()
    fa = str(tmp_path / "in.fasta")
    open(fa, "wb").write(FC.cases(api.FASTA_BLOCK)["a header line from block 0 into block 3"])
    d = ctx.docs_from_fasta(fa)
    assert not d.has_qual
    d.close()
    with pytest.raises(api.LimeError) as e:
        ctx.docs_from_fastq_qual(str(tmp_path / "no_such_file"))
    assert e.value.code == _lib.ERR_IO


def _free_bytes():
    import torch
    from lime_amd import api
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


def test_device_memory_comes_back(ctx, tmp_path):
    """parses with qualities, trims and refusals of each kind: after lime_trim_cache the device's free memory is what it was"""
    from lime_amd import api
    cases = QC.cases(api.FASTA_BLOCK)
    reads, quals = _short_collection(5, 3000, top=200)
    good = T.fastq_of(reads, quals)
    refused = [cases[f"reason {r} in a record in block 2"] for r in (0, 1, 2)] + [cases["reason 3 in block 2"], _longer_qualities(api)]

    def cycle():
        d = ctx.docs_from_fastq_qual_bytes(good)
        out, info = ctx.docs_trim(d, 20, 20)
        assert info["n_changed"] > 0
        plain = ctx.docs_from_fastq_bytes(good)
        for call in [lambda: ctx.docs_trim(plain, 20, 20), lambda: ctx.docs_trim(d, 94, 1)] + [lambda x=x: ctx.docs_from_fastq_qual_bytes(x) for x in refused]:
            with pytest.raises(api.LimeError):
                call()
        for x in (d, out, plain):
            x.close()

    cycle()
    before = _free_bytes()
    cycle()
    assert _free_bytes() == before


# ---- the reader ----
def test_reader_batches_against_the_whole_file(ctx, tmp_path):
    from lime_amd import _lib, api
    reads, quals = _short_collection(6, 5000, top=130)
    data = T.fastq_of(reads, quals)
    want, w_info = T.trim_model(reads, quals, 7, 20)
    w_text, w_off = T.records(want)
    for batch in (1, 7, 4096):
        n = len(reads) if batch > 1 else 40
        r = ctx.seq_reader_bytes(T.fastq_of(reads[:n], quals[:n]) if batch == 1 else data, "fastq", window_bytes=0 if batch > 1 else 700)
        assert r.trim_info() == {k: 0 for k in w_info}
        r.set_trim(7, 20)
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
        assert first == n and lens == [len(x) for x in want[:n]]
        assert np.concatenate(texts).tobytes() == b"".join(want[:n])
        assert r.trim_info() == (w_info if n == len(reads) else T.trim_model(reads[:n], quals[:n], 7, 20)[1])
        with pytest.raises(api.LimeError) as e:                              # after the first batch: refused
            r.set_trim(7, 20)
        assert e.value.code == _lib.ERR_ARG and "before the first" in str(e.value)
        r.close()
    r = ctx.seq_reader_bytes(data, "fastq")
    assert r.next(3) is not None
    with pytest.raises(api.LimeError) as e:
        r.set_trim(1, 1)
    assert e.value.code == _lib.ERR_ARG
    r.close()
    r = ctx.seq_reader_bytes(data, "fastq")
    with pytest.raises(api.LimeError) as e:
        r.set_trim(94, 1)
    assert e.value.code == _lib.ERR_ARG and "0 .. 93" in str(e.value)
    r.close()
    r = ctx.seq_reader_bytes(b">r\nACGT\n>s\nTT\n", "fasta")
    with pytest.raises(api.LimeError) as e:
        r.set_trim(20, 20)
    assert e.value.code == _lib.ERR_ARG and "FASTA" in str(e.value)
    assert r.next(5)[0].info() == (2, 6)                                    # and the reader goes on untrimmed
    r.close()


def test_a_malformed_batch_through_a_trimming_reader(ctx, tmp_path):
    """the refusal names the line in the FILE, as without the trim"""
    from lime_amd import _lib, api
    data = QC.fixed_records(50).tobytes() + b"@r\nACGT\n+\nIII\n" + QC.rec()
    want = QC.host_read(tmp_path, data)
    assert want == (204, 2)
    r = ctx.seq_reader_bytes(data, "fastq")
    r.set_trim(20, 20)
    for _ in range(5):
        assert r.next(10)[0].info()[0] == 10
    with pytest.raises(api.LimeError) as e:
        r.next(10)
    assert e.value.code == _lib.ERR_ARG and QC.refusal_of(str(e.value)) == want
    r.close()
