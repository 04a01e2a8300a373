"""The per-position read statistics on the device (lime_docs_qc_dev, lime_seq_reader_set_qc; lime_qc_kernel.hip) against lime_read_qc and the
models of tests/qc_cases.py: every word of the tables equal.  Read lengths around the kernel's word (64) and its multiples at every n_pos, so
that the pooled row begins inside a word, at a word edge and at position 1; every class and the quality thresholds in every lane;
collections around a workgroup's 4 reads and past the grid cap; documents of every origin; one record whose pooled quality sum passes 2^32;
the reader in batches, behind every stage and behind the overlap cut.  tests/test_qc_cases_cpu.py holds lime_read_qc against the models."""
import gc

import numpy as np
import pytest

from tests import adapter_cases as A
from tests import filter_cases as F
from tests import overlap_cases as V
from tests import qc_cases as Q
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


def _docs(ctx, reads, quals=None, stream=None):
    """documents from arrays; with qualities from the bytes of a FASTQ file (no byte of which is LF or CR)"""
    import torch
    if quals is not None:
        assert reads
        d = ctx.docs_from_fastq_qual_bytes(Q.fastq_of(reads, quals))
        assert d.has_qual
        return d
    text, off = Q.records(reads)
    t = torch.from_numpy(text).cuda() if len(text) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    return ctx.docs_from_arrays_dev(t, torch.from_numpy(off.astype(np.int64)).cuda(), len(reads), len(text), stream=stream)


def _differ(got, want, n_pos):
    k = int(np.nonzero(got != want)[0][0])
    n = n_pos + 1
    where = f"row {k // 8} counter {k % 8}" if k < 8 * n else f"len_hist[{k - 8 * n}]" if k < 9 * n else f"gc_hist[{k - 9 * n}]" if k < 9 * n + 101 else f"mq_hist[{k - 9 * n - 101}]"
    return f"{int((got != want).sum())} words differ, the first at {where}: {int(got[k])}, not {int(want[k])}"


def _check(ctx, reads, quals, n_pos_list, what, d=None, stream=None, model="vector", with_qual=None):
    """the documents `d` (default: made from reads / quals) at every n_pos: against lime_read_qc and the model(s)"""
    from lime_amd import api
    own = d is None
    if not reads:
        quals = None                            # (no record: a FASTQ file of no bytes)
    if own:
        d = _docs(ctx, reads, quals, stream)
    if with_qual is None:
        with_qual = quals is not None
    assert d.has_qual == with_qual, what
    text, q, off = Q.flat(reads, quals if with_qual else None)
    for n_pos in n_pos_list:
        want = api.read_qc(text, off, n_pos, qual=q)["tables"]
        if model == "both":
            assert np.array_equal(Q.model(reads, quals if with_qual else None, n_pos), want), (what, n_pos)
        elif model == "vector":
            assert np.array_equal(Q.qc_vector(reads, quals if with_qual else None, n_pos), want), (what, n_pos)
        got = ctx.docs_qc(d, n_pos, stream=stream)
        assert got["tables"].shape == (Q.words(n_pos),)
        if not np.array_equal(got["tables"], want):
            raise AssertionError(f"{what}, n_pos {n_pos}: " + _differ(got["tables"], want, n_pos))
        for k in Q.KEYS:
            assert np.array_equal(got[k], Q.split(want, n_pos)[k])
    if own:
        d.close()


def _bases(rng, L):
    return rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L).tobytes()


def _collection(seed, n, top=150):
    rng = np.random.default_rng([Q.SEED, 3, seed])
    reads = [Q.fuzz_read(rng, int(rng.integers(0, top))) for _ in range(n)]
    return reads, [Q.fuzz_qual(rng, len(r)) for r in reads]


@pytest.mark.parametrize("n_pos", Q.N_POS)
def test_read_lengths(ctx, n_pos):
    """every length with mixed content and qualities, with one class alone, and n_pos - 1, n_pos, n_pos + 1 besides; with and without qualities"""
    rng = np.random.default_rng([Q.SEED, 5, n_pos])
    reads = []
    for L in sorted(set(Q.LENGTHS) | {n_pos - 1, n_pos, n_pos + 1}):
        reads += [Q.fuzz_read(rng, L), _bases(rng, L), b"N" * L, _bases(rng, L).lower()]
    quals = [Q.fuzz_qual(rng, len(r)) for r in reads]
    _check(ctx, reads, quals, (n_pos,), "lengths with qualities")
    _check(ctx, reads, None, (n_pos,), "lengths without qualities")


def test_the_pooled_row_at_every_n_pos_of_three_words(ctx):
    """n_pos = 1 .. 130 and around 512 on reads of up to four words: the pool begins in every lane of words 0, 1 and 2"""
    rng = np.random.default_rng([Q.SEED, 6])
    reads = [Q.fuzz_read(rng, L) for L in (0, 1, 64, 65, 129, 130, 131, 192, 200, 256, 600)]
    quals = [Q.fuzz_qual(rng, len(r)) for r in reads]
    d = _docs(ctx, reads, quals)
    _check(ctx, reads, quals, tuple(range(1, 131)) + (191, 192, 193, 510, 511, 512), "n_pos sweep", d=d)
    d.close()


def test_every_class_and_lower_case_in_every_lane(ctx):
    """one read per lane and symbol: the symbol alone among N's at that lane of words 0, 1 and 2"""
    reads = []
    for sym in b"ACGTacgtN" + bytes([0, 255, ord("R")]):
        for lane in range(64):
            r = bytearray(b"N" * 192 if sym != ord("N") else b"A" * 192)
            for w in range(3):
                r[64 * w + lane] = sym
            reads.append(bytes(r))
    _check(ctx, reads, None, (64, 100, 192, 512, 1), "classes in every lane")


def test_qualities_on_the_thresholds_in_lane_0_lane_63_and_the_pools_first_lane(ctx):
    reads, quals = [], []
    for n_pos in Q.N_POS:
        for at in {0, 63, n_pos - 1, n_pos, min(n_pos + 1, 599), 64, 127, 128}:
            for q in (0, 32, 52, 53, 62, 63, 255):
                b = bytearray([40] * 600)
                b[at] = q
                reads.append(b"ACGT" * 150); quals.append(bytes(b))
    _check(ctx, reads, quals, Q.N_POS, "thresholds")
    # the cases of the host test, on the device
    for name, r, q in Q.threshold_cases():
        _check(ctx, r, q, (1, 64, 100, 512), name, model="both")


@pytest.mark.parametrize("name", [c[0] for c in Q.hand_cases()])
def test_the_hand_made_cases(ctx, name):
    _, reads, quals, n_pos, want = next(c for c in Q.hand_cases() if c[0] == name)
    _check(ctx, reads, quals, (n_pos,) + Q.N_POS, name, model="both")
    d = _docs(ctx, reads, quals)
    assert np.array_equal(ctx.docs_qc(d, n_pos)["tables"], want)
    d.close()


def test_collection_sizes(ctx):
    """1 .. 9 reads (a workgroup holds 4), one and two reads over the grid's reads per trip, three trips + 1"""
    trip = Q.READS_PER_TRIP
    reads, quals = _collection(7, 3 * trip + 1, top=90)
    for n in list(range(1, 10)) + [trip - 1, trip, trip + 1, trip + 2, 2 * trip + 1, 3 * trip + 1]:
        _check(ctx, reads[:n], quals[:n], (64, 100), f"{n} reads")
    _check(ctx, reads, None, (1, 512), "three trips + 1, no qualities")
    assert np.array_equal(Q.qc_vector(reads[:trip + 2], quals[:trip + 2], 100), Q.qc_loop(reads[:trip + 2], quals[:trip + 2], 100))


def test_every_read_empty_and_no_read(ctx):
    _check(ctx, [b""] * 70, [b""] * 70, Q.N_POS, "70 empty reads", model="both")
    _check(ctx, [b""] * 70, None, (1, 512), "70 empty reads, no qualities", model="both")
    _check(ctx, [], None, (1, 64, 512), "no read", model="both")
    from lime_amd import api
    d = _docs(ctx, [], None)
    t = np.arange(Q.words(5), dtype=np.uint64)
    assert np.array_equal(ctx.docs_qc(d, 5, tables=t)["tables"], np.arange(Q.words(5), dtype=np.uint64))       # no read adds nothing
    d.close()
    assert api.qc_words(5) == len(t)


def test_the_call_adds_to_the_callers_tables(ctx):
    a, qa = _collection(8, 300)
    b, qb = _collection(9, 200)
    da, db = _docs(ctx, a, qa), _docs(ctx, b, None)
    t = np.zeros(Q.words(100), dtype=np.uint64)
    out = ctx.docs_qc(da, 100, tables=t)
    assert out["tables"] is t
    ctx.docs_qc(db, 100, tables=t)
    ctx.docs_qc(da, 100, tables=t)
    assert np.array_equal(t, 2 * Q.qc_vector(a, qa, 100) + Q.qc_vector(b, None, 100))
    da.close(); db.close()


def test_documents_of_every_origin(ctx):
    """a FASTA parse, a FASTQ parse without and with qualities, arrays, reverse complements, the output of each trim"""
    rng = np.random.default_rng([Q.SEED, 12])
    reads = [F.fuzz_read(rng, int(rng.integers(0, 150))) for _ in range(900)]
    for k in range(0, 900, 3):                                              # read-through and the instrument's G's, for the trims to cut
        L = len(reads[k])
        if L > 60:
            reads[k] = (reads[k][:L - 40] + A.TRUSEQ_R1[:20] + b"G" * 40)[:L]
    quals = [T.sample_quals(rng, len(r)) for r in reads]
    fq = T.fastq_of(reads, quals)
    n_pos = (64, 100, 256)
    for d, wq in ((ctx.docs_from_bytes(Q.fasta_of(reads)), False), (ctx.docs_from_fastq_bytes(fq), False), (ctx.docs_from_fastq_qual_bytes(fq), True),
                  (_docs(ctx, reads), False)):
        _check(ctx, reads, quals, n_pos, "parsed documents", d=d, with_qual=wq)
        d.close()
    d = ctx.docs_from_fastq_qual_bytes(fq)
    rc = d.revcomp()
    rc_text, rc_off = rc.get()
    rc_reads = [rc_text[int(a):int(b)].tobytes() for a, b in zip(rc_off[:-1], rc_off[1:])]
    assert [len(r) for r in rc_reads] == [len(r) for r in reads] and rc_reads != reads
    _check(ctx, rc_reads, None, n_pos, "reverse complements", d=rc, with_qual=False)
    cut, _ = ctx.docs_trim(d, 5, 20)
    q_reads = T.trim_model(reads, quals, 5, 20)[0]
    _check(ctx, q_reads, None, n_pos, "the quality trim's output", d=cut)
    ad, _ = ctx.docs_trim_adapter(cut, A.TRUSEQ_R1[:20], 3, 10)
    a_reads = A.trim_model(q_reads, A.TRUSEQ_R1[:20], 3, 10)[0]
    _check(ctx, a_reads, None, n_pos, "the adapter trim's output", d=ad)
    p = F.params(F.G_, max_len=120, min_len=20, max_n=3, min_complexity=30)
    fl, _ = ctx.docs_filter(ad, **p)
    f_reads = F.filter_model(a_reads, p)[0]
    _check(ctx, f_reads, None, n_pos, "the filter's output", d=fl)
    assert q_reads != reads and a_reads != q_reads and f_reads != a_reads
    half = 100
    m1, m2 = _docs(ctx, reads[:half]), _docs(ctx, [V.revcomp(r) for r in reads[:half]])
    o1, o2, info = ctx.docs_trim_overlap(m1, m2, 30, 10)
    c1, c2, _, w_info = V.cut_model(reads[:half], [V.revcomp(r) for r in reads[:half]], 30, 10, insert=V.insert_masks)
    assert info == w_info
    _check(ctx, c1, None, n_pos, "the overlap cut's first output", d=o1)
    _check(ctx, c2, None, n_pos, "the overlap cut's second output", d=o2)
    for x in (o1, o2, m1, m2, fl, ad, cut, rc, d):
        x.close()


def test_text_at_offsets_that_are_no_multiples_of_64(ctx):
    """reads of 1 .. 63 symbols in front push every later read off the 64-byte lines, and the arrays themselves come from views at odd addresses"""
    import torch
    rng = np.random.default_rng([Q.SEED, 13])
    for shift in (1, 7, 63):
        reads = [_bases(rng, shift)] + [Q.fuzz_read(rng, 100) for _ in range(64)] + [_bases(rng, 700)]
        text, off = Q.records(reads)
        raw = torch.zeros(len(text) + 128, dtype=torch.uint8, device="cuda")
        view = raw[shift:shift + len(text)]
        view.copy_(torch.from_numpy(text))
        d = ctx.docs_from_arrays_dev(view, torch.from_numpy(off.astype(np.int64)).cuda(), len(reads), len(text))
        _check(ctx, reads, None, (63, 64, 100), f"shift {shift}", d=d)
        d.close()
        quals = [Q.fuzz_qual(rng, len(r)) for r in reads]
        _check(ctx, reads, quals, (63, 64, 100), f"shift {shift} with qualities")


def test_side_stream(ctx):
    import torch
    reads, _ = _collection(102, 5000, top=120)
    text, off = Q.records(reads)
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
        _check(ctx, reads, None, (100, 512), "side stream", d=d, stream=s.cuda_stream)
        d.close()
    s.synchronize()
    torch.cuda.synchronize()


def test_seeded_collections(ctx):
    for case in range(200):
        reads, quals, n_pos = Q.fuzz_collection(Q.SEED, case)
        _check(ctx, reads, quals, (n_pos,), f"fuzz_collection({Q.SEED}, {case})", model="both" if case % 4 == 0 else "vector")


def test_one_record_whose_pooled_quality_sum_passes_2_to_the_32(ctx):
    """17 000 000 symbols of quality byte 255 at n_pos = 64: the pooled qsum is 255 * (17 000 000 - 64) > 2^32, and every word is exact"""
    from lime_amd import api
    L, n_pos = 17_000_000, 64
    seq = np.frombuffer(b"ACGTN" * (L // 5), dtype=np.uint8)
    fq = np.concatenate([np.frombuffer(b"@r\n", dtype=np.uint8), seq, np.frombuffer(b"\n+\n", dtype=np.uint8), np.full(L, 255, dtype=np.uint8),
                         np.frombuffer(b"\n", dtype=np.uint8)])
    d = ctx.docs_from_fastq_qual_bytes(fq)
    assert d.info() == (1, L) and d.has_qual
    got = ctx.docs_qc(d, n_pos)
    d.close()
    want = np.zeros(Q.words(n_pos), dtype=np.uint64)
    s = Q.split(want, n_pos)
    for p in range(n_pos):
        s["rows"][p, p % 5] = 1
        s["rows"][p, 5:] = (255, 1, 1)
    pooled = L - n_pos
    assert 255 * pooled > 2 ** 32
    for c in range(5):
        s["rows"][n_pos, c] = L // 5 - len([p for p in range(n_pos) if p % 5 == c])
    s["rows"][n_pos, 5:] = (255 * pooled, pooled, pooled)
    s["len_hist"][n_pos] = 1
    s["gc_hist"][50] = 1                                                    # C + G are 2 of the 4 bases in 5 symbols
    s["mq_hist"][255] = 1
    if not np.array_equal(got["tables"], want):
        raise AssertionError(_differ(got["tables"], want, n_pos))
    assert int(got["rows"][n_pos, 5]) == 255 * (L - 64)
    oracle = api.read_qc(seq, np.array([0, L], dtype=np.uint64), n_pos, qual=np.full(L, 255, dtype=np.uint8))
    assert np.array_equal(oracle["tables"], want)


def _free_bytes():
    import torch
    from lime_amd import api
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


def test_refusals_and_device_memory_comes_back(ctx):
    """every refusal comes before any launch, with a text; after calls and refusals of each kind and lime_trim_cache the device's free memory
    is what it was"""
    from lime_amd import _lib, api
    reads, quals = _collection(103, 3000, top=200)
    other = api.Context(0)

    def cycle():
        d = _docs(ctx, reads, quals)
        assert ctx.docs_qc(d, 512)["rows"][:, 5].any()
        t = np.zeros(Q.words(512), dtype=np.uint64)
        for n_pos in (0, 513, 1 << 20):
            assert ctx.lib.lime_docs_qc_dev(ctx.h, d.h, n_pos, None, t.ctypes.data) == _lib.ERR_ARG
            msg = ctx.lib.lime_last_error().decode()
            assert "positions" in msg and "1 .. 512" in msg and "lime_docs_qc_dev:" in msg
            with pytest.raises(ValueError):
                ctx.docs_qc(d, n_pos)
        with pytest.raises(api.LimeError) as e:
            other.docs_qc(d, 64)
        assert e.value.code == _lib.ERR_ARG and "another context" in str(e.value)
        for args in ((None, d.h, 64, None, t.ctypes.data), (ctx.h, None, 64, None, t.ctypes.data), (ctx.h, d.h, 64, None, None)):
            assert ctx.lib.lime_docs_qc_dev(*args) == _lib.ERR_ARG and "NULL" in ctx.lib.lime_last_error().decode()
        assert not t.any()
        d.close()

    try:
        cycle()
        before = _free_bytes()
        cycle()
        assert _free_bytes() == before
    finally:
        other.close()


# ---- the reader ----
def _batches(r, batch, other=None):
    """every batch of the reader -> [(text bytes, lengths, has_qual)] per batch"""
    out, first = [], 0
    while True:
        b = r.next(batch)
        if b is None:
            break
        d, f = b
        assert f == first
        t, o = d.get()
        out.append((t[:d.info()[1]].tobytes(), np.diff(o.astype(np.int64)).tolist(), d.has_qual))
        first += d.info()[0]
        d.close()
    return out


def _reader_set(r, stages):
    for name, args in stages:
        getattr(r, name)(*args[0], **args[1])


ALL = F.params(F.G_, max_len=120, min_len=20, max_n=3, min_complexity=30)
A20 = A.TRUSEQ_R1[:20]


def _stage_sample():
    rng = np.random.default_rng([Q.SEED, 15])
    reads = []
    for k in range(400):
        L = int(rng.integers(0, 140))
        r = F.fuzz_read(rng, L)
        if L > 40 and k % 3 == 0:                                           # read-through, then the instrument's G's
            r = (r[:int(rng.integers(10, L - 25))] + A20 + b"G" * L)[:L]
        reads.append(r)
    quals = [T.sample_quals(rng, len(r)) for r in reads]
    return reads, quals


STAGES = {
    "none": ([], lambda reads, quals: reads),
    "quality trim": ([("set_trim", ((5, 20), {}))], lambda reads, quals: T.trim_model(reads, quals, 5, 20)[0]),
    "adapter": ([("set_adapter", ((A20, 3, 10), {}))], lambda reads, quals: A.trim_model(reads, A20, 3, 10)[0]),
    "filter": ([("set_filter", ((), ALL))], lambda reads, quals: F.filter_model(reads, ALL)[0]),
    "chain": ([("set_filter", ((), ALL)), ("set_adapter", ((A20, 3, 10), {})), ("set_trim", ((5, 20), {}))],
              lambda reads, quals: F.filter_model(A.trim_model(T.trim_model(reads, quals, 5, 20)[0], A20, 3, 10)[0], ALL)[0]),
}


@pytest.mark.parametrize("fmt,stage", [(f, s) for f in ("fasta", "fastq") for s in sorted(STAGES) if f == "fastq" or s not in ("quality trim", "chain")])
def test_reader_raw_and_out_against_the_whole_file(ctx, fmt, stage):
    """set_qc in batches of 1, 7 and 64: RAW is the file as parsed (with the quality tables for FASTQ), OUT the batches as handed out; the
    batches themselves are those of a reader without set_qc
    (a FASTA file holds no qualities to trim by: the quality trim and the chain run on FASTQ alone)"""
    reads, quals = _stage_sample()
    setters, stage_model = STAGES[stage]
    n_pos = 100
    data = Q.fasta_of(reads) if fmt == "fasta" else T.fastq_of(reads, quals)
    for batch in (1, 7, 64):
        n = len(reads) if batch > 1 else 40
        part = Q.fasta_of(reads[:n]) if fmt == "fasta" else T.fastq_of(reads[:n], quals[:n])
        plain = ctx.seq_reader_bytes(part if n < len(reads) else data, fmt)
        r = ctx.seq_reader_bytes(part if n < len(reads) else data, fmt)
        for k in ("raw", "out"):
            z = r.qc(k)
            assert z["tables"].shape == (Q.words(1),) and not z["tables"].any()      # zeros without set_qc
        _reader_set(plain, setters)
        _reader_set(r, setters)
        r.set_qc(n_pos)
        got, want = _batches(r, batch), _batches(plain, batch)
        assert got == want and len(got) == (n + batch - 1) // batch
        assert not any(b[2] for b in got)
        done = stage_model(reads[:n], quals[:n])
        assert b"".join(b[0] for b in got) == b"".join(done)
        raw = Q.qc_vector(reads[:n], quals[:n] if fmt == "fastq" else None, n_pos)
        out = Q.qc_vector(done, None, n_pos)
        for k, w in (("raw", raw), (0, raw), ("out", out), (1, out)):
            t = r.qc(k)["tables"]
            if not np.array_equal(t, w):
                raise AssertionError(f"{fmt}, {stage}, batches of {batch}, {k}: " + _differ(t, w, n_pos))
        if stage == "none":
            assert np.array_equal(out, Q.qc_vector(reads[:n], None, n_pos))
        else:
            assert not np.array_equal(out[:8 * (n_pos + 1)].reshape(-1, 8)[:, :5], raw[:8 * (n_pos + 1)].reshape(-1, 8)[:, :5])      # (the stage shows)
        r.close(); plain.close()


def test_next_pair_counts_each_batch_once_behind_the_overlap_cut(ctx):
    """two linked readers with a quality trim and a filter each: RAW is each file as parsed, OUT what next_pair hands out -- the four models
    composed -- and each batch is counted once"""
    rng = np.random.default_rng([Q.SEED, 16])
    r1, r2 = [], []
    for k in range(150):
        read = _bases(rng, 100)
        I = int(rng.integers(35, 141))
        a, b = V.plant(rng, read, I, V.TRUSEQ_R1, V.TRUSEQ_R2, int(rng.integers(0, 3)))
        r1.append(a); r2.append(b)
    q1, q2 = [T.sample_quals(rng, len(r)) for r in r1], [T.sample_quals(rng, len(r)) for r in r2]
    p = F.params(F.G_, min_len=20, max_n=3)
    s1 = F.filter_model(T.trim_model(r1, q1, 0, 20)[0], p)[0]
    s2 = F.filter_model(T.trim_model(r2, q2, 0, 20)[0], p)[0]
    ins = [V.insert_masks(x, y, 30, 10) for x, y in zip(s1, s2)]              # once, shared by the batch sizes

    def cut(n):
        return V.cut_model(s1[:n], s2[:n], 30, 10, insert=lambda x, y, O, E, it=iter(ins): next(it))

    assert cut(len(r1))[3]["n_cut"] > 30 and s1 != r1
    n_pos = 64
    for batch in (1, 7, 64):
        n = len(r1) if batch > 1 else 30
        w1, w2, _, w_info = cut(n)
        a, b = ctx.seq_reader_bytes(T.fastq_of(r1[:n], q1[:n]), "fastq"), ctx.seq_reader_bytes(T.fastq_of(r2[:n], q2[:n]), "fastq")
        for r in (a, b):
            r.set_trim(0, 20); r.set_filter(**p); r.set_qc(n_pos)
        a.set_overlap(b, 30, 10)
        t1, t2, n_batches = b"", b"", 0
        while True:
            got = a.next_pair(b, batch)
            if got is None:
                break
            d1, d2, _ = got
            assert not d1.has_qual and not d2.has_qual
            t1 += d1.get()[0][:d1.info()[1]].tobytes(); t2 += d2.get()[0][:d2.info()[1]].tobytes()
            d1.close(); d2.close()
            n_batches += 1
        assert t1 == b"".join(w1) and t2 == b"".join(w2) and n_batches == (n + batch - 1) // batch and a.overlap_info() == w_info
        for r, raw, q, kept in ((a, r1, q1, w1), (b, r2, q2, w2)):
            assert np.array_equal(r.qc("raw")["tables"], Q.qc_vector(raw[:n], q[:n], n_pos))
            out = r.qc("out")["tables"]
            want = Q.qc_vector(kept, None, n_pos)
            if not np.array_equal(out, want):
                raise AssertionError(f"batches of {batch}: " + _differ(out, want, n_pos))
            assert int(Q.split(out, n_pos)["len_hist"].sum()) == n          # once, not twice
        a.close(); b.close()


def test_set_qc_after_the_first_next_and_with_bad_values_is_refused(ctx):
    from lime_amd import _lib, api
    reads = [_bases(np.random.default_rng([Q.SEED, 14, k]), 40 + k) for k in range(50)]
    r = ctx.seq_reader_bytes(Q.fastq_of(reads), "fastq")
    for n_pos in (0, 513):
        with pytest.raises(api.LimeError) as e:
            r.set_qc(n_pos)
        assert e.value.code == _lib.ERR_ARG and "1 .. 512" in str(e.value) and "lime_seq_reader_set_qc:" in str(e.value)
    t = np.zeros(Q.words(1), dtype=np.uint64)
    assert ctx.lib.lime_seq_reader_qc(r.h, 2, t.ctypes.data) == _lib.ERR_ARG and ctx.lib.lime_seq_reader_qc(r.h, 0, None) == _lib.ERR_ARG
    b = r.next(3)
    assert b is not None and b[0].info()[0] == 3 and not b[0].has_qual      # (the refusals left the reader as it was)
    assert b[0].get()[0][:b[0].info()[1]].tobytes() == b"".join(reads[:3])
    b[0].close()
    with pytest.raises(api.LimeError) as e:
        r.set_qc(64)
    assert e.value.code == _lib.ERR_ARG and "before the first" in str(e.value)
    assert not r.qc("raw")["tables"].any() and not r.qc("out")["tables"].any()
    r.close()
