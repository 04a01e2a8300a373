"""The cut kernels (lime_seq_cut_dev, lime_amd/csrc/lime_seqcut_kernel.hip) against the numpy rule of tests/seqcut_cases.py (model_cut), which
tests/test_seqcut_cases_cpu.py holds against lime_fastq_read / lime_fasta_read: the wanted marker at the edges of a lane's 16 bytes, a
wave's 1024 and a block's 4096, windows around those sizes, eof 0 and 1 with the markers below, at and above max_reads, views at every
offset mod 16, a grid past the cap, a side stream and seeded windows."""
import numpy as np
import pytest

from tests import fasta_cases as FC
from tests import fastq_cases as QC
from tests import seqcut_cases as SC

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 1)


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


def _check(ctx, data, fmt, max_reads, eof, what="", t=None):
    got = ctx.seq_cut_dev(_to_dev(data) if t is None else t, fmt, max_reads, eof)
    want = SC.model_cut(data, fmt, max_reads, eof)
    assert got == want, (what, fmt, max_reads, eof, len(data), got, want)
    return got


def _all_modes(ctx, data, fmt, what):
    """eof 0 and 1, max_reads below, at and above the records the window holds, and 1"""
    full = SC.model_cut(data, fmt, 2 ** 32 - 1, True)[1]
    for eof in (False, True):
        for mr in sorted({1, max(full - 1, 1), max(full, 1), full + 1, 2 ** 32 - 1}):
            _check(ctx, data, fmt, mr, eof, what)


def test_block_is_what_the_sizes_assume():
    from lime_amd import api
    assert api.FASTA_BLOCK == 4096


def test_window_sizes(ctx):
    for n in SIZES:
        _all_modes(ctx, QC.pad(n) if n == 0 or n >= 6 else b"\n" * n, SC.FASTQ, f"pad({n})")
        _all_modes(ctx, b"\n" * n, SC.FASTQ, f"{n} LF")
        _all_modes(ctx, b"A" * n, SC.FASTQ, f"{n} bytes without LF")
        _all_modes(ctx, FC.two_line_records(n), SC.FASTA, f"two_line_records({n})")
        _all_modes(ctx, b">" * n, SC.FASTA, f"{n} '>'")
        _all_modes(ctx, b">\n" * (n // 2) + b">" * (n % 2), SC.FASTA, f"{n} bytes of empty records")


@pytest.mark.parametrize("width", [16, 1024, 4096])
def test_the_wanted_marker_at_the_edges_of_a_unit(ctx, width):
    """the LF that ends record 2 (FASTQ), the '>' that starts record 2 (FASTA), as the last and the first byte of a lane's, a wave's and a
    block's bytes, in the second and third block too, and as the window's last byte"""
    for base in (0, 4096, 2 * 4096):
        for at in (base + width - 1, base + width):
            if at < 31:
                continue
            # FASTQ: two records of at + 1 bytes in all, the last LF at `at`; one more record behind
            q = QC.rec() + b"@" + b"h" * (at + 1 - 15 - 14) + b"\nACGT\n+\nIIII\n"
            assert len(q) == at + 1 and q[at:at + 1] == b"\n"
            for tail in (b"", QC.rec(), QC.rec()[:-1], b"@x\nAC"):
                for eof in (False, True):
                    for mr in (1, 2, 3):
                        got = _check(ctx, q + tail, SC.FASTQ, mr, eof, f"LF at {at}")
                        if mr == 2 and (tail or not eof):
                            assert got[:2] == (at + 1, 2)
            # FASTA: '>' of record 2 at `at`, the LF in front of it the last byte of the unit before
            a = b">a\nAC\n>b\n" + b"A" * (at - 10) + b"\n" + b">c\nGG\n>d\nT"
            assert a[at:at + 1] == b">" and a[at - 1:at] == b"\n"
            for eof in (False, True):
                for mr in (1, 2, 3, 4, 5):
                    got = _check(ctx, a, SC.FASTA, mr, eof, f"'>' at {at}")
                    if mr == 2:
                        assert got[:2] == (at, 2)
            _check(ctx, a[:at + 1], SC.FASTA, 2, False, f"'>' at {at}, the window's last byte")
            assert _check(ctx, a[:at + 1], SC.FASTA, 5, True, f"'>' at {at}, the window's last byte")[:2] == (at + 1, 3)


def test_a_block_of_lfs_with_the_wanted_one_in_every_quarter(ctx):
    data = QC.rec() + b"\n" * 4096 + QC.rec()
    for quarter in range(4):
        for mr in (1 + quarter * 256, 1 + quarter * 256 + 255, 1 + quarter * 256 + 100):
            for eof in (False, True):
                got = _check(ctx, data, SC.FASTQ, mr, eof, f"quarter {quarter}")
                assert got[0] == 15 + 4 * (mr - 1)
    _all_modes(ctx, b"\n" * 4096, SC.FASTQ, "a block of LF")


def test_fasta_markers_are_line_first_only(ctx):
    cases = FC.cases(4096)
    for name in ("'>' in mid-line", "'>' right after a lone CR", "CRLF", "consecutive headers and empty records", "headers only",
                 "text in front of the first header", "text longer than a block in front of the first header", "no header", "only '>'"):
        _all_modes(ctx, cases[name], SC.FASTA, name)
    assert ctx.seq_cut_dev(_to_dev(b">a\nAC>GT\nA>\n\r>x\n"), "fasta", 5, True) == (16, 1, 1)
    lf_ends_block = b">a\n" + b"A" * (4096 - 4) + b"\n" + b">b\nCC\n>c\n"          # a '>' whose LF is the last byte of the block before
    assert ctx.seq_cut_dev(_to_dev(lf_ends_block), "fasta", 1, False) == (4096, 1, 3)
    _all_modes(ctx, lf_ends_block, SC.FASTA, "LF ends a block")
    unfinished = b">a\nACGT\nAC"                       # one unfinished record: nothing in front of the cut
    assert ctx.seq_cut_dev(_to_dev(unfinished), "fasta", 1, False) == (0, 0, 1)
    assert ctx.seq_cut_dev(_to_dev(b"@r\nACGT\n+\nII"), "fastq", 1, False) == (0, 0, 3)


def test_crlf_and_every_case(ctx):
    _all_modes(ctx, QC.rec(eol=b"\r\n") * 5, SC.FASTQ, "CRLF")
    for fmt in (SC.FASTQ, SC.FASTA):
        for name, data in (QC.cases(4096) if fmt == SC.FASTQ else FC.cases(4096)).items():
            for mr in (1, 3, 682):
                for eof in (False, True):
                    _check(ctx, data, fmt, mr, eof, name)


def test_views_at_every_offset(ctx):
    """the window as a view at every offset mod 16 of a larger buffer, with markers right in front of it and right behind"""
    import torch
    for fmt, data, mr in ((SC.FASTQ, QC.pad(4096 + 8)[:-1], 255), (SC.FASTQ, QC.rec() * 3 + b"@r\nAC", 3), (SC.FASTA, FC.two_line_records(4096 + 9), 300),
                          (SC.FASTA, b">a\nAC\n>b", 1)):
        n = len(data)
        for shift in range(16):
            raw = torch.full((64 + n + 64,), ord("A"), dtype=torch.uint8, device="cuda")
            start = 16 + (-raw.data_ptr()) % 16 + shift
            raw[start - 2:start] = torch.tensor(list(b">\n"), dtype=torch.uint8, device="cuda")
            raw[start + n:start + n + 3] = torch.tensor(list(b"\n>\n"), dtype=torch.uint8, device="cuda")
            view = raw[start:start + n]
            view.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
            assert view.data_ptr() % 16 == shift
            for eof in (False, True):
                _check(ctx, data, fmt, mr, eof, f"offset {shift}", t=view)


def test_past_the_grid_cap(ctx):
    """The launchers cap their grids at 8192 workgroups, one block of 4096 bytes per trip.  4 200 100 records of 16 bytes are 16 407
    blocks: a third trip.  Closed form: FASTQ cuts after record m at 16 m; FASTA (the same bytes with '>' for '@': every fourth line
    is a header) cuts in front of record m at 16 m."""
    n_rec = 4_200_100
    assert (16 * n_rec + 4095) // 4096 == 16407
    t = _to_dev(QC.REC16).repeat(n_rec)
    for m in (1, 8192 * 256, 16390 * 256 + 3, n_rec - 1, n_rec):
        assert ctx.seq_cut_dev(t, "fastq", m, False) == (16 * m, m, 4 * n_rec)
    assert ctx.seq_cut_dev(t, "fastq", n_rec + 1, False) == (16 * n_rec, n_rec, 4 * n_rec)
    assert ctx.seq_cut_dev(t[:-1], "fastq", n_rec, True) == (16 * n_rec - 1, n_rec, 4 * n_rec - 1)
    t[::16] = ord(">")
    for m in (1, 8192 * 256, 16390 * 256 + 3, n_rec - 1):
        assert ctx.seq_cut_dev(t, "fasta", m, False) == (16 * m, m, n_rec)
    assert ctx.seq_cut_dev(t, "fasta", n_rec, False) == (16 * (n_rec - 1), n_rec - 1, n_rec)
    assert ctx.seq_cut_dev(t, "fasta", n_rec, True) == (16 * n_rec, n_rec, n_rec)


def test_side_stream(ctx):
    import torch
    data = QC.fixed_records(40 * 4096 // 16 + 3).tobytes()
    src = _to_dev(data)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    late = torch.full((len(data),), ord("@"), dtype=torch.uint8, device="cuda")            # not the input yet
    filler = torch.rand(16_000_000, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):                       # best effort: sorts stand in front of the write of the input on the side stream
        for _ in range(4):
            filler = torch.sort(filler.flip(0))[0]
        late.copy_(src.flip(0).flip(0))
        got = ctx.seq_cut_dev(late, "fastq", 10_000, False, stream=s.cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()
    assert got == SC.model_cut(data, SC.FASTQ, 10_000, False) == (160_000, 10_000, 4 * (40 * 256 + 3))


@pytest.mark.parametrize("fmt", [SC.FASTQ, SC.FASTA], ids=["fastq", "fasta"])
def test_seeded_windows(ctx, fmt):
    rng = np.random.default_rng([SC.SEED, 5, fmt])
    for case in range(200):
        data = (QC.fuzz_bytes if fmt == SC.FASTQ else FC.fuzz_bytes)(SC.SEED, case, 4096)
        if case % 2:
            data = QC.fuzz_mutated(SC.SEED, case, 4096) if fmt == SC.FASTQ else SC.fuzz_fasta_records(SC.SEED, case, 4096)
        full = SC.model_cut(data, fmt, 2 ** 32 - 1, True)[1]
        for eof in (False, True):
            for mr in {1, int(rng.integers(1, full + 2)), full + 1}:
                _check(ctx, data, fmt, mr, eof, f"seeded window {case}")


def test_refusals(ctx):
    from lime_amd import _lib, api

    class Null:
        def data_ptr(self):
            return 0

        def numel(self):
            return 0
    for call in (lambda: ctx.seq_cut_dev(Null(), "fastq", 1, True, n=2 ** 32), lambda: ctx.seq_cut_dev(_to_dev(b"@r\n"), "fastq", 0, True),
                 lambda: ctx.seq_cut_dev(_to_dev(b"@r\n"), 2, 1, True)):
        with pytest.raises(api.LimeError) as e:
            call()
        assert e.value.code == _lib.ERR_ARG and "lime_seq_cut_dev" in str(e.value)
