"""The device FASTA parser (lime_docs_from_bytes_dev and its host front ends) against lime_fasta_read on the same bytes, and the device
reverse complement (lime_docs_revcomp, fed through lime_docs_from_arrays_dev) against the numpy model of tests/fasta_cases.py, which
tests/test_fasta_cases_cpu.py holds against lime_fasta_read.  Every comparison is np.array_equal on text and doc_off; no tolerance."""
import gc
import os

import numpy as np
import pytest

from tests import fasta_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


def _oracle(tmp_path, data):
    from lime_amd import api
    p = str(tmp_path / "in.fasta")
    with open(p, "wb") as f:
        f.write(data)
    return FC.records(api.fasta_read(p))


def _parse_dev(ctx, data, stream=None):
    import torch
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if len(data) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    d = ctx.docs_from_bytes_dev(t, stream=stream)
    got = d.get(), d.info()
    d.close()
    return got


def _same(got, want, what):
    (text, off), (n_docs, n_text) = got
    w_text, w_off = want
    assert n_docs == len(w_off) - 1 and n_text == len(w_text), (what, n_docs, n_text, len(w_off) - 1, len(w_text))
    assert np.array_equal(off, w_off), (what, off[:8], w_off[:8])
    if not np.array_equal(text, w_text):
        bad = np.nonzero(text != w_text)[0]
        raise AssertionError(f"{what}: text differs at {len(bad)} of {len(text)} bytes, first {bad[:5].tolist()}")


def _case_names():
    return sorted(FC.cases(4096))


def test_block_is_what_the_cases_assume():
    from lime_amd import api
    assert sorted(FC.cases(api.FASTA_BLOCK)) == _case_names()


@pytest.mark.parametrize("name", _case_names())
def test_parser_case(ctx, tmp_path, name):
    from lime_amd import api
    data = FC.cases(api.FASTA_BLOCK)[name]
    _same(_parse_dev(ctx, data), _oracle(tmp_path, data), name)


def test_parser_host_front_ends(ctx, tmp_path):
    """lime_docs_from_bytes and lime_docs_from_fasta on a multi-block case; an unreadable file is LIME_ERR_IO"""
    from lime_amd import _lib, api
    data = FC.cases(api.FASTA_BLOCK)["a header line from block 0 into block 3"] + FC.fuzz_bytes(FC.SEED, 24, api.FASTA_BLOCK)
    want = _oracle(tmp_path, data)
    for d in (ctx.docs_from_bytes(data), ctx.docs_from_fasta(str(tmp_path / "in.fasta")), ctx.docs_from_bytes(b"")):
        _same((d.get(), d.info()), want if d.info()[1] else (np.zeros(0, np.uint8), np.zeros(1, np.uint64)), "host front end")
        d.close()
    with pytest.raises(api.LimeError) as e:
        ctx.docs_from_fasta(str(tmp_path / "no_such_file"))
    assert e.value.code == _lib.ERR_IO


def test_parser_views_at_every_offset(ctx, tmp_path):
    """the input as a view at every offset mod 16 of a larger buffer, '\\n>' right in front of it and '\\n>x' right behind: the result is
    that of the view alone (byte 0's line-first test reads nothing; no 16-byte load reaches past the end)"""
    import torch
    from lime_amd import api
    for data in (b">h\nACGT\nAC\n>b\nTTGA\nGG", FC.two_line_records(api.FASTA_BLOCK + 7)[:-1] + b"A"):
        want = _oracle(tmp_path, data)
        assert want[1][-1] > 0 and not data.endswith(b"\n")
        n = len(data)
        for shift in range(16):
            raw = torch.full((64 + n + 64,), ord("A"), dtype=torch.uint8, device="cuda")
            start = 16 + (-raw.data_ptr()) % 16 + shift
            raw[start - 2:start] = torch.tensor(list(b"\n>"), dtype=torch.uint8, device="cuda")
            raw[start + n:start + n + 3] = torch.tensor(list(b"\n>x"), dtype=torch.uint8, device="cuda")
            view = raw[start:start + n]
            view.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
            assert view.data_ptr() % 16 == shift
            d = ctx.docs_from_bytes_dev(view)
            _same((d.get(), d.info()), want, f"{n} bytes at offset {shift}")
            d.close()


def test_parser_past_the_grid_cap(ctx):
    """The launchers of lime_fasta_kernel.hip cap their grids at BY_BLOCKS = 8192 workgroups (lime_bytes.h), one block of FASTA_BLOCK bytes per trip; whoever
    changes that changes this.  4 480 000 records '>r' / 'ACGTACGTACG' of 15 bytes are 16 407 blocks: a third trip.  doc_off[k] = 11 k."""
    import torch
    from lime_amd import api
    rec, n_rec = b">r\nACGTACGTACG\n", 4_480_000
    assert len(rec) * n_rec > 2 * 8192 * api.FASTA_BLOCK
    t = torch.from_numpy(np.frombuffer(rec, dtype=np.uint8).copy()).cuda().repeat(n_rec)
    d = ctx.docs_from_bytes_dev(t)
    assert d.info() == (n_rec, 11 * n_rec)
    text, off = d.get()
    d.close()
    assert np.array_equal(off, np.arange(n_rec + 1, dtype=np.uint64) * 11)
    assert np.array_equal(text.reshape(n_rec, 11), np.broadcast_to(np.frombuffer(b"ACGTACGTACG", np.uint8), (n_rec, 11)))


def test_parser_side_stream(ctx, tmp_path):
    import torch
    from lime_amd import api
    data = FC.two_line_records(40 * api.FASTA_BLOCK + 5)
    want = _oracle(tmp_path, data)
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    late = torch.full((len(data),), ord(">"), dtype=torch.uint8, device="cuda")            # not the input yet
    filler = torch.rand(16_000_000, device="cuda")
    torch.cuda.synchronize()
    # best effort, as in tests/test_merge_edges_gpu.py::test_side_stream: sorts stand in front of the write of the input on the side stream
    with torch.cuda.stream(s):
        for _ in range(4):
            filler = torch.sort(filler.flip(0))[0]
        late.copy_(src.flip(0).flip(0))
        d = ctx.docs_from_bytes_dev(late, stream=s.cuda_stream)
        r = d.revcomp(stream=s.cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()
    _same((d.get(), d.info()), want, "side stream")
    assert np.array_equal(r.get()[0], FC.model_revcomp(*want))
    d.close(); r.close()


def test_parser_seeded_fuzz(ctx, tmp_path):
    from lime_amd import api
    for case in range(FC.FUZZ_CASES):
        data = FC.fuzz_bytes(FC.SEED, case, api.FASTA_BLOCK)
        _same(_parse_dev(ctx, data), _oracle(tmp_path, data), f"fuzz_bytes({FC.SEED}, {case})")
    assert FC.FUZZ_CASES == 200


# ---- reverse complement ----
def _arrays_dev(ctx, text, off, shift=0):
    """Docs from arrays on the device; the text as a view `shift` bytes into a 16-byte aligned buffer"""
    import torch
    n = len(text)
    raw = torch.full((32 + shift + n + 48,), 0x41, dtype=torch.uint8, device="cuda")
    buf = raw[16 + (-raw.data_ptr()) % 16:]
    view = buf[shift:shift + n]
    if n:
        view.copy_(torch.from_numpy(np.ascontiguousarray(text)))
    off_t = torch.from_numpy(np.asarray(off).astype(np.int64)).cuda()
    return ctx.docs_from_arrays_dev(view, off_t, len(off) - 1, n)


def _revcomp_check(ctx, text, off, what, shift=0):
    d = _arrays_dev(ctx, text, off, shift)
    assert d.info() == (len(off) - 1, len(text))
    g_text, g_off = d.get()
    assert np.array_equal(g_text, text) and np.array_equal(g_off, off), what
    r = d.revcomp()
    r_text, r_off = r.get()
    d.close(); r.close()
    assert np.array_equal(r_off, off), what
    want = FC.model_revcomp(text, off)
    if not np.array_equal(r_text, want):
        bad = np.nonzero(r_text != want)[0]
        raise AssertionError(f"{what}: differs at {len(bad)} of {len(want)} bytes, first {bad[:5].tolist()}: got {r_text[bad[:5]].tolist()}, want {want[bad[:5]].tolist()}")


@pytest.mark.parametrize("name", sorted(FC.revcomp_collections(4096)))
def test_revcomp_collection(ctx, name):
    from lime_amd import api
    text, off = FC.records(FC.revcomp_collections(api.FASTA_BLOCK)[name])
    _revcomp_check(ctx, text, off, name)


def test_revcomp_no_documents_and_empty_documents(ctx):
    _revcomp_check(ctx, np.zeros(0, np.uint8), np.zeros(1, np.uint64), "no documents")
    _revcomp_check(ctx, np.zeros(0, np.uint8), np.zeros(4, np.uint64), "three empty documents")
    _revcomp_check(ctx, *FC.records([b"", b"", b"A", b"", b"CG", b""]), "empty documents around short ones")


def test_revcomp_views_at_every_offset(ctx):
    text, off = FC.records(FC.revcomp_collections(4096)["every length 0 .. 130"][:70])
    for shift in range(16):
        _revcomp_check(ctx, text, off, f"offset {shift}", shift)


def test_revcomp_many_short_documents(ctx):
    """2 * 10^6 documents of 1 .. 3 symbols, 4 * 10^6 symbols: 250 000 lane pieces of 16 bytes, beyond the 512 x 256 lanes of the capped grid,
    every piece crossing several documents"""
    rng = np.random.default_rng([FC.SEED, 9])
    lens = rng.integers(1, 4, size=2_000_000)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    text = np.frombuffer(b"ACGTNacgtn", np.uint8)[rng.integers(0, 10, size=int(off[-1]))]
    assert (int(off[-1]) + 15) // 16 > 512 * 256
    _revcomp_check(ctx, text, off, "2e6 short documents")


def test_revcomp_twice_is_the_identity(ctx):
    rng = np.random.default_rng([FC.SEED, 10])
    docs = [np.frombuffer(b"ACGTRYKMBVDHSWNacgtrykmbvdhswn", np.uint8)[rng.integers(0, 30, size=int(n))].tobytes() for n in rng.integers(0, 300, size=500)]
    text, off = FC.records(docs)
    d = _arrays_dev(ctx, text, off)
    r = d.revcomp()
    rr = r.revcomp()
    assert not np.array_equal(r.get()[0], text) and np.array_equal(rr.get()[0], text) and np.array_equal(rr.get()[1], off)
    for x in (d, r, rr):
        x.close()


# ---- refusals, memory ----
def test_refusals(ctx):
    import torch
    from lime_amd import _lib, api
    small = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for n in (2 ** 32, 2 ** 32 + 5, 2 ** 40):                               # by argument only: nothing that large exists or is read
        with pytest.raises(api.LimeError) as e:
            ctx.docs_from_bytes_dev(small, n=n)
        assert e.value.code == _lib.ERR_ARG and str(n) in str(e.value)
    text = torch.zeros(10, dtype=torch.uint8, device="cuda")
    for off in ([0, 6, 4, 10], [1, 4, 6, 10], [0, 4, 6, 9], [0, 4, 6, 11]):
        with pytest.raises(api.LimeError) as e:
            ctx.docs_from_arrays_dev(text, torch.tensor(off, dtype=torch.int64, device="cuda"), 3, 10)
        assert e.value.code == _lib.ERR_ARG, off
    with pytest.raises(api.LimeError) as e:
        ctx.docs_from_arrays_dev(text, torch.tensor([0], dtype=torch.int64, device="cuda"), 0, 10)
    assert e.value.code == _lib.ERR_ARG


def _free_bytes():
    import torch
    from lime_amd import api
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


def test_device_memory_comes_back(ctx, tmp_path):
    """parses, reverse complements and refusals, host front ends included: after lime_trim_cache the device's free memory is what it was"""
    from lime_amd import api
    big = FC.two_line_records(70 * 1024 * 1024)                              # raw bytes and documents beyond the block cache's 64 MB threshold
    small = FC.cases(api.FASTA_BLOCK)["a header line from block 0 into block 3"]
    p = str(tmp_path / "in.fasta")
    open(p, "wb").write(big)

    def cycle():
        for d in (ctx.docs_from_bytes(small), ctx.docs_from_bytes(big), ctx.docs_from_fasta(p)):
            r = d.revcomp()
            assert r.info() == d.info()
            r.close(); d.close()
        with pytest.raises(api.LimeError):
            ctx.docs_from_fasta(str(tmp_path / "no_such_file"))
        with pytest.raises(api.LimeError):
            ctx.docs_from_bytes_dev(_Null(), n=2 ** 32)

    cycle()                                                                 # what the runtime allocates on first launches is there before the reading
    before = _free_bytes()
    cycle()
    assert _free_bytes() == before


class _Null:
    """stands for a device tensor that is never read"""
    def data_ptr(self):
        return 0

    def numel(self):
        return 0
