"""The device FASTQ parser (lime_docs_from_fastq_bytes_dev and its host and file front ends, lime_docs_from_file) against lime_fastq_read on
the same bytes: valid inputs by np.array_equal on text and doc_off, refused ones by code, line and reason, with *out NULL and the
device's memory back.  tests/test_fastq_cases_cpu.py holds lime_fastq_read against the two models of tests/fastq_cases.py."""
import ctypes as C
import gc
import os

import numpy as np
import pytest

from tests import fasta_cases as FC
from tests import fastq_cases as QC

pytestmark = pytest.mark.gpu


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


def _parse_dev(ctx, t, stream=None, who="lime_docs_from_fastq_bytes_dev"):
    """the C call itself -> (text, doc_off), or (line, reason) of a LIME_ERR_ARG refusal that left *out NULL"""
    from lime_amd import _lib
    h = C.c_void_p(1)
    code = ctx.lib.lime_docs_from_fastq_bytes_dev(ctx.h, C.c_void_p(t.data_ptr()), int(t.numel()), stream, C.byref(h))
    if code != 0:
        msg = ctx.lib.lime_last_error().decode()
        assert code == _lib.ERR_ARG and h.value is None and msg.startswith(who + ": line "), (code, h.value, msg)
        return QC.refusal_of(msg)
    d = ctx._docs_of(h)
    text, off = d.get()
    assert d.info() == (len(off) - 1, len(text))
    d.close()
    return text, off


def _same(got, want, what):
    assert QC.is_refusal(got) == QC.is_refusal(want), (what, got, want)
    if QC.is_refusal(want):
        assert tuple(got) == tuple(want), (what, got, want)
        return
    assert np.array_equal(got[1], want[1]), (what, got[1][:8], want[1][:8])
    if not np.array_equal(got[0], want[0]):
        bad = np.nonzero(got[0] != want[0])[0] if len(got[0]) == len(want[0]) else []
        raise AssertionError(f"{what}: text differs ({len(got[0])} and {len(want[0])} bytes), first at {list(bad[:5])}")


def _case_names():
    return sorted(QC.cases(4096))


def test_block_is_what_the_cases_assume():
    from lime_amd import api
    assert sorted(QC.cases(api.FASTA_BLOCK)) == _case_names()


@pytest.mark.parametrize("name", _case_names())
def test_parser_case(ctx, tmp_path, name):
    from lime_amd import api
    data = QC.cases(api.FASTA_BLOCK)[name]
    _same(_parse_dev(ctx, _to_dev(data)), QC.host_read(tmp_path, data), name)


def test_parser_random_strings(ctx, tmp_path):
    from lime_amd import api
    for case in range(QC.FUZZ_CASES):
        data = QC.fuzz_bytes(QC.SEED, case, api.FASTA_BLOCK)
        _same(_parse_dev(ctx, _to_dev(data)), QC.host_read(tmp_path, data), f"fuzz_bytes({QC.SEED}, {case})")
    assert QC.FUZZ_CASES == 400


def test_parser_mutated_records(ctx, tmp_path):
    from lime_amd import api
    valid = 0
    for case in range(QC.FUZZ_CASES):
        data = QC.fuzz_mutated(QC.SEED, case, api.FASTA_BLOCK)
        want = QC.host_read(tmp_path, data)
        valid += not QC.is_refusal(want)
        _same(_parse_dev(ctx, _to_dev(data)), want, f"fuzz_mutated({QC.SEED}, {case})")
    assert QC.FUZZ_CASES == 400 and 100 <= valid <= 300


def test_front_ends(ctx, tmp_path):
    """lime_docs_from_fastq_bytes, lime_docs_from_fastq and lime_docs_from_file on a multi-block input, valid and refused; lime_docs_from_file on
    a FASTA file is lime_docs_from_fasta; an unreadable file is LIME_ERR_IO"""
    from lime_amd import _lib, api
    cases = QC.cases(api.FASTA_BLOCK)
    data = cases["a sequence line from block 0 into block 3"] + cases["several blocks of valid records"]
    want = QC.host_read(tmp_path, data)
    p = str(tmp_path / "in.fastq")
    assert not QC.is_refusal(want) and api.seq_format(p) == "fastq"
    for d in (ctx.docs_from_fastq_bytes(data), ctx.docs_from_fastq_bytes(np.frombuffer(data, np.uint8)), ctx.docs_from_fastq(p), ctx.docs_from_file(p)):
        _same(d.get(), want, "front end")
        assert d.info() == (len(want[1]) - 1, len(want[0]))
        d.close()
    d = ctx.docs_from_fastq_bytes(b"")
    assert d.info() == (0, 0) and np.array_equal(d.get()[1], np.zeros(1, np.uint64))
    d.close()
    bad = data + cases["reason 1 in a record in block 2"]
    want = QC.host_read(tmp_path, bad)
    assert QC.is_refusal(want) and want[1] == 1
    for call, who in ((lambda: ctx.docs_from_fastq_bytes(bad), "lime_docs_from_fastq_bytes"), (lambda: ctx.docs_from_fastq(p), "lime_docs_from_fastq"),
                      (lambda: ctx.docs_from_file(p), "lime_docs_from_fastq")):
        with pytest.raises(api.LimeError) as e:
            call()
        assert e.value.code == _lib.ERR_ARG and who + ": line " in str(e.value) and QC.refusal_of(str(e.value)) == tuple(want)
    fa = FC.cases(api.FASTA_BLOCK)["a header line from block 0 into block 3"]
    q = str(tmp_path / "in.fasta")
    open(q, "wb").write(fa)
    d = ctx.docs_from_file(q)
    w_text, w_off = FC.records(api.fasta_read(q))
    assert api.seq_format(q) == "fasta" and np.array_equal(d.get()[0], w_text) and np.array_equal(d.get()[1], w_off) and len(w_off) > 2
    d.close()
    for call in (ctx.docs_from_fastq, ctx.docs_from_file):
        with pytest.raises(api.LimeError) as e:
            call(str(tmp_path / "no_such_file"))
        assert e.value.code == _lib.ERR_IO


def test_views_at_every_offset(ctx, tmp_path):
    """the input as a view at every offset mod 16 of a larger buffer, '\\n@' right in front of it and '\\n@x' right behind: the result is
    that of the view alone (byte 0's line-first test reads nothing; no 16-byte load reaches past the end)"""
    import torch
    from lime_amd import api
    for data in (QC.rec() + QC.rec(b"x", b"TTGAC")[:-1], QC.pad(api.FASTA_BLOCK + 8)[:-1], QC.rec() + b"@r\nACGT\n+\nIII"):
        want = QC.host_read(tmp_path, data)
        assert not data.endswith(b"\n")
        n = len(data)
        for shift in range(16):
            raw = torch.full((64 + n + 64,), ord("A"), dtype=torch.uint8, device="cuda")
            start = 16 + (-raw.data_ptr()) % 16 + shift
            raw[start - 2:start] = torch.tensor(list(b"\n@"), dtype=torch.uint8, device="cuda")
            raw[start + n:start + n + 3] = torch.tensor(list(b"\n@x"), dtype=torch.uint8, device="cuda")
            view = raw[start:start + n]
            view.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
            assert view.data_ptr() % 16 == shift
            _same(_parse_dev(ctx, view), want, f"{n} bytes at offset {shift}")


def test_past_the_grid_cap(ctx):
    """The launchers of lime_fastq_kernel.hip cap their grids at BY_BLOCKS = 8192 workgroups (lime_bytes.h), one block of FASTA_BLOCK bytes per trip; whoever
    changes that changes this.  4 200 100 records of 16 bytes are 16 407 blocks: a third trip.  doc_off[k] = 4 k.  Then one quality byte of a
    record in block 16 390, which the third trip handles, becomes a CR: its line, reason 2."""
    import torch
    from lime_amd import api
    n_rec = 4_200_100
    assert len(QC.REC16) == 16 and 16 * n_rec > 2 * 8192 * api.FASTA_BLOCK and (16 * n_rec + api.FASTA_BLOCK - 1) // api.FASTA_BLOCK == 16407
    t = _to_dev(QC.REC16).repeat(n_rec)
    text, off = _parse_dev(ctx, t)
    assert np.array_equal(off, np.arange(n_rec + 1, dtype=np.uint64) * 4)
    assert np.array_equal(text.reshape(n_rec, 4), np.broadcast_to(np.frombuffer(b"ACGT", np.uint8), (n_rec, 4)))
    k = 16390 * (api.FASTA_BLOCK // 16) + 3
    assert 16 * k // api.FASTA_BLOCK == 16390 >= 2 * 8192
    t[16 * k + 13] = 13
    t[16 * (k + 1000)] = ord("X")                                           # a later line's reason 0 does not win
    assert _parse_dev(ctx, t) == (4 * k + 4, 2)


def test_side_stream(ctx, tmp_path):
    import torch
    from lime_amd import api
    data = QC.fixed_records(40 * api.FASTA_BLOCK // 16 + 3).tobytes()
    want = QC.host_read(tmp_path, data)
    src = _to_dev(data)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    late = torch.full((len(data),), ord("@"), dtype=torch.uint8, device="cuda")            # not the input yet
    filler = torch.rand(16_000_000, device="cuda")
    torch.cuda.synchronize()
    # best effort, as in tests/test_fasta_edges_gpu.py: sorts stand in front of the write of the input on the side stream
    with torch.cuda.stream(s):
        for _ in range(4):
            filler = torch.sort(filler.flip(0))[0]
        late.copy_(src.flip(0).flip(0))
        got = _parse_dev(ctx, late, stream=s.cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()
    _same(got, want, "side stream")


def test_revcomp_of_parsed_reads(ctx, tmp_path):
    from lime_amd import api
    data = QC.cases(api.FASTA_BLOCK)["several blocks of valid records"] + QC.cases(api.FASTA_BLOCK)["empty reads"] + QC.rec(seq=b"ACGTURYKMBVDHSWNacgtn-")
    want = QC.host_read(tmp_path, data, 1)
    d = ctx.docs_from_fastq(str(tmp_path / "in.fastq"))
    r = d.revcomp()
    _same(r.get(), want, "reverse complements")
    assert not np.array_equal(d.get()[0], want[0])
    d.close(); r.close()


class _Null:
    """stands for a device tensor that is never read"""
    def data_ptr(self):
        return 0

    def numel(self):
        return 0


def test_inputs_of_2_to_the_32_bytes_are_refused_before_any_launch(ctx):
    from lime_amd import _lib, api
    for n in (2 ** 32, 2 ** 32 + 5, 2 ** 40):                               # by argument only: nothing that large exists, and address 0 is never read
        with pytest.raises(api.LimeError) as e:
            ctx.docs_from_fastq_bytes_dev(_Null(), n=n)
        assert e.value.code == _lib.ERR_ARG and str(n) in str(e.value)


def _free_bytes():
    import torch
    from lime_amd import api
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


def test_device_memory_comes_back(ctx, tmp_path):
    """parses and refusals of each reason, host front ends included: after lime_trim_cache the device's free memory is what it was"""
    from lime_amd import api
    cases = QC.cases(api.FASTA_BLOCK)
    big = QC.fixed_records(70 * 1024 * 1024 // 16).tobytes()                 # raw bytes and documents beyond the block cache's 64 MB threshold
    p, q = str(tmp_path / "big.fastq"), str(tmp_path / "bad.fastq")
    open(p, "wb").write(big)
    open(q, "wb").write(big[:-20] + b"\r" + big[-19:])
    refused = [cases[f"reason {r} in a record in block 2"] for r in (0, 1, 2)] + [cases["reason 3 in block 2"]]

    def cycle():
        for d in (ctx.docs_from_fastq_bytes(cases["several blocks of valid records"]), ctx.docs_from_fastq_bytes(big), ctx.docs_from_file(p)):
            assert d.info()[0] > 0
            d.close()
        for call in [lambda: ctx.docs_from_fastq(q), lambda: ctx.docs_from_fastq(str(tmp_path / "no_such_file")),
                     lambda: ctx.docs_from_fastq_bytes_dev(_Null(), n=2 ** 32)] + [lambda x=x: ctx.docs_from_fastq_bytes(x) for x in refused]:
            with pytest.raises(api.LimeError):
                call()

    cycle()                                                                 # what the runtime allocates on first launches is there before the reading
    before = _free_bytes()
    cycle()
    assert _free_bytes() == before
