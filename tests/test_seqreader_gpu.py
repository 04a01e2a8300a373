"""lime_seq_reader (Context.seq_reader / seq_reader_bytes) against api.fastq_read / api.fasta_read of the whole input: the batches' records,
concatenated, are the whole file's; every batch but the last holds max_reads; a malformed FASTQ is refused in the batch that meets it with
the whole file's line and reason, the batches before it handed out; the device's memory comes back.

The inputs are those of tests/seqcut_cases.py (every case of fastq_cases.py / fasta_cases.py and 400 seeded inputs per format) at its
max_reads and window values.  A batch costs several launches and read-backs, so the grid is walked, not crossed: every input is read
with ten of the forty (max_reads, window) pairs, the pairs rotating with the input's number, so that every pair is used about a hundred
times per format and every input meets every max_reads and every window value; an input of more than 64 records meets one of
max_reads 1, 2, 3 instead of all three.  tests/test_seqcut_cases_cpu.py runs the reader's model over the whole cross product."""
import gc

import pytest

from tests import fasta_cases as FC
from tests import fastq_cases as QC
from tests import seqcut_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


def _whole(tmp_path, fmt, data):
    """api.fastq_read / api.fasta_read of the bytes -> list of records, or (line, reason)"""
    from lime_amd import api
    p = str(tmp_path / "whole.seq")
    with open(p, "wb") as f:
        f.write(data)
    try:
        return (api.fastq_read if fmt == SC.FASTQ else api.fasta_read)(p)
    except api.LimeError as e:
        return QC.refusal_of(str(e))


def _records(docs):
    text, off = docs.get()
    raw = text.tobytes()
    return [raw[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]


def _read_all(reader, max_reads):
    """-> (records, batch sizes, (line, reason) or None)"""
    from lime_amd import _lib, api
    got, sizes = [], []
    while True:
        try:
            b = reader.next(max_reads)
        except api.LimeError as e:
            assert e.code == _lib.ERR_ARG and "lime_seq_reader_next: line " in str(e), str(e)
            return got, sizes, QC.refusal_of(str(e))
        if b is None:
            return got, sizes, None
        docs, first = b
        assert first == len(got)
        r = _records(docs)
        docs.close()
        got.extend(r)
        sizes.append(len(r))


def _check(ctx, fmt, data, whole, max_reads, window, what):
    r = ctx.seq_reader_bytes(data, fmt, window)
    got, sizes, failure = _read_all(r, max_reads)
    info = r.info()
    if isinstance(whole, tuple):
        assert failure == whole, (what, failure, whole)
        assert got == [ln.replace(b"\r", b"") for ln in data.split(b"\n")[1:4 * len(got):4]], what       # the batches before it, intact
        assert len(got) == (whole[0] - 1) // 4 // max_reads * max_reads, (what, len(got))
    else:
        assert failure is None and got == whole, (what, len(got), len(whole))
        assert info["bytes"] == len(data) or (fmt == SC.FASTA and not whole), what
        assert r.next(max_reads) is None and r.next(1) is None, what                                     # next after the end
    assert all(s == max_reads for s in sizes[:-1]) and all(1 <= s <= max_reads for s in sizes), (what, sizes[-3:])
    assert info["records"] == len(got) and info["format"] == ("fastq" if fmt == SC.FASTQ else "fasta")
    assert info["lines"] == (4 * len(got) if fmt == SC.FASTQ else 0)
    r.close()
    return info


@pytest.mark.parametrize("fmt", [SC.FASTQ, SC.FASTA], ids=["fastq", "fasta"])
def test_every_input_in_batches(ctx, tmp_path, fmt):
    from lime_amd import api
    used = {}
    for k, (name, data) in enumerate(SC.inputs(fmt, api.FASTA_BLOCK).items()):
        whole = _whole(tmp_path, fmt, data)
        n_rec = (data.count(b"\n") + 1) // 4 if isinstance(whole, tuple) else len(whole)
        grid = SC.grid(n_rec)
        for g, (max_reads, window) in enumerate(grid):
            i, j = divmod(g, len(SC.WINDOWS))
            if (i + j + k) % 4:
                continue
            if n_rec > 64 and i < 3 and i != k % 3:
                continue
            _check(ctx, fmt, data, whole, max_reads, window, (name, max_reads, window))
            used[(i, j)] = used.get((i, j), 0) + 1
    assert len(used) == 40 and min(used.values()) >= 50, used


def test_files_and_the_window_that_grows(ctx, tmp_path):
    """a record that spans three windows, growth from a 1-byte window, multi-line FASTA records cut between their lines, a preamble
    longer than the window: over files"""
    from lime_amd import api
    cases = FC.cases(api.FASTA_BLOCK)
    multi = b"".join(b">r%d\n" % k + b"ACGTNACGTT\n" * (k % 4) + b"GG\n" for k in range(300))
    inputs = {
        "a FASTQ record that spans three windows": (QC.rec() + QC.rec(b"h" * 40, b"ACGT" * 30) + QC.rec(), 64, 1),
        "FASTQ from a 1-byte window": (QC.fixed_records(300).tobytes(), 1, 7),
        "a FASTA record that spans three windows": (b">a\nAC\n>b\n" + b"ACGT\n" * 40 + b">c\nGG\n", 64, 1),
        "multi-line FASTA records cut between their lines": (multi, 50, 3),
        "FASTA from a 1-byte window": (multi, 1, 100),
        "a preamble longer than the window": (cases["text longer than a block in front of the first header"] + b">b\nTT\n", 4096, 1),
        "lines of two blocks in front of the first header": (cases["lines of two blocks in front of the first header"], 100, 2),
    }
    for name, (data, window, max_reads) in inputs.items():
        p = str(tmp_path / "in.seq")
        open(p, "wb").write(data)
        fmt = SC.FASTQ if api.seq_format(p) == "fastq" else SC.FASTA
        want = (api.fastq_read if fmt == SC.FASTQ else api.fasta_read)(p)
        r = ctx.seq_reader(p, window)
        assert r.info()["window_bytes"] == window
        got, sizes, failure = _read_all(r, max_reads)
        assert failure is None and got == want and len(want) >= 1, name
        assert r.info()["window_bytes"] == SC.model_reader(data, fmt, max_reads, window)[1] > window, name
        r.close()
    # the default window, iteration, and a file that cannot be read
    p = str(tmp_path / "default.fastq")
    open(p, "wb").write(QC.fixed_records(1000).tobytes())
    r = ctx.seq_reader(p)
    r.batch = 300
    sizes = []
    for d in r:
        sizes.append(d.info()[0])
        d.close()
    assert sizes == [300, 300, 300, 100] and r.info()["window_bytes"] == 16000
    r.close()
    from lime_amd import _lib
    with pytest.raises(api.LimeError) as e:
        ctx.seq_reader(str(tmp_path / "no_such_file"))
    assert e.value.code == _lib.ERR_IO


@pytest.mark.parametrize("reason", [0, 1, 2, 3])
def test_a_refusal_names_the_files_line(ctx, tmp_path, reason):
    """each reason in the first, a middle and the last batch of 100 records, through small and large windows"""
    n_rec, batch = 1000, 100
    for where, k in (("the first batch", 37), ("a middle batch", 537), ("the last batch", 999 if reason < 3 else 1000)):
        if reason == 3:
            data = QC.fixed_records(k).tobytes() + b"@r\nAC\n"
            want = (4 * k + 2, 3)
        else:
            data = QC._broken(n_rec, {k: reason})
            want = (4 * k + (1, 3, 4)[reason], reason)
        whole = _whole(tmp_path, SC.FASTQ, data)
        assert whole == want, (where, whole, want)
        for window in (100, 4096, 0):
            _check(ctx, SC.FASTQ, data, whole, batch, window, (where, reason, window))
        r = ctx.seq_reader_bytes(data, "fastq", 4096)
        got, sizes, failure = _read_all(r, batch)
        assert failure == want and sizes == [batch] * (k // batch), where
        from lime_amd import api
        with pytest.raises(api.LimeError) as e:      # the refusal is final
            r.next(batch)
        assert QC.refusal_of(str(e.value)) == want
        r.close()


def _free_bytes():
    import torch
    from lime_amd import api
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


def test_device_memory_comes_back(ctx, tmp_path):
    """after reading to the end, after a refusal and after closing half-way (and a reader left to lime_shutdown)"""
    from lime_amd import api
    good = QC.fixed_records(70 * 1024 * 1024 // 16).tobytes()                # beyond the block cache's 64 MB threshold
    bad = good[:-20] + b"\r" + good[-19:]
    p = str(tmp_path / "big.fastq")
    open(p, "wb").write(good)

    def cycle():
        r = ctx.seq_reader(p, 16 << 20)
        n = 0
        for d in r:
            n += d.info()[0]
            d.close()
        assert n == len(good) // 16
        r.close()
        r = ctx.seq_reader_bytes(bad, "fastq")
        with pytest.raises(api.LimeError):
            while r.next(1_000_000) is not None:
                pass
        r.close()
        r = ctx.seq_reader(p, 1 << 20)               # a window that has to grow, closed half-way
        d, _ = r.next(500_000)
        assert d.info()[0] == 500_000 and r.info()["window_bytes"] == 8 << 20
        d.close()
        r.close()

    cycle()
    before = _free_bytes()
    cycle()
    assert _free_bytes() == before
    c2 = api.Context(0)
    r = c2.seq_reader(p, 1 << 20)
    d, _ = r.next(1000)
    c2.close()                                       # lime_shutdown releases the open reader and the batch
    assert r.h is None and d.h is None
