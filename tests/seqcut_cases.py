"""The cut of a reads file's window into whole records, and the reader built on it (include/lime_hip.h states both at lime_seq_cut_dev and
lime_seq_reader; lime_amd/csrc/lime_seqcut_kernel.hip states the rule): model_cut is the rule in numpy, model_reader the reader's refill
loop over it (window, start, fill, the doubling), which yields the batches' bytes.  The inputs are every case of tests/fastq_cases.py and
tests/fasta_cases.py and 400 seeded inputs per format.  tests/test_seqcut_cases_cpu.py holds the models against lime_fastq_read /
lime_fasta_read without a GPU; tests/test_seqcut_edges_gpu.py holds the kernels against model_cut, tests/test_seqreader_gpu.py the reader
against the whole-file readers and against model_reader's batches."""
import numpy as np

from tests import fasta_cases as FC
from tests import fastq_cases as QC

SEED = 20271
FUZZ_CASES = 400
FASTA, FASTQ = 0, 1
MAX_READS = (1, 2, 3, 682, None)                  # None: more than the records
WINDOWS = (1, 15, 16, 17, 4095, 4096, 4097, None)  # None: the whole input
WINDOW_MAX = 0xFFFFFFFF


def markers_of(data, fmt):
    """positions of the markers of a window: FASTQ the LFs, FASTA the line-first '>'"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    if fmt == FASTQ:
        return np.flatnonzero(a == 10)
    first = np.ones(len(a), dtype=bool)
    first[1:] = a[:-1] == 10
    return np.flatnonzero(first & (a == ord(">")))


def cut_of(pos, n, last_is_lf, fmt, max_reads, eof):
    """the rule on a window of n bytes whose markers stand at pos -> (cut, m, markers)"""
    t = len(pos)
    if n == 0:
        return 0, 0, 0
    if fmt == FASTQ:
        if eof and t // 4 < max_reads:
            return n, (t + (0 if last_is_lf else 1)) // 4, t
        m = min(max_reads, t // 4)
        return (int(pos[4 * m - 1]) + 1 if m else 0), m, t
    m = min(max_reads, t if eof else max(t, 1) - 1)
    if eof and m == t:
        return n, m, t
    return (int(pos[m]) if t else 0), m, t


def model_cut(data, fmt, max_reads, eof):
    data = bytes(data)
    return cut_of(markers_of(data, fmt), len(data), data[-1:] == b"\n", fmt, max_reads, eof)


def model_reader(data, fmt, max_reads, window):
    """the reader's loop -> (list of the batches' bytes, the window size at the end).  A batch is data[a:b]: the cut is taken on
    data[start of the window .. its fill) with the file's own markers, which are the window's because a window begins at a line start"""
    data = bytes(data)
    size = len(data)
    every = markers_of(data, fmt)
    cap = window if window else min(64 << 20, max(size, 1))
    base = start = fill = 0                          # the window holds data[base .. base + fill), the unread part begins at start
    out = []
    while True:
        if start == fill:
            base, start, fill = base + fill, 0, 0
        if start == 0:
            fill = min(cap, size - base)
        eof = base + fill == size
        n = fill - start
        if n == 0 and eof:
            return out, cap
        lo = base + start
        assert lo == 0 or data[lo - 1:lo] == b"\n", "a window begins at a line start"
        pos = every[np.searchsorted(every, lo):np.searchsorted(every, lo + n)] - lo
        cut, m, _ = cut_of(pos, n, data[lo + n - 1:lo + n] == b"\n", fmt, max_reads, eof)
        if m < max_reads and not eof:
            if start == 0:
                assert cap < WINDOW_MAX
                cap = min(WINDOW_MAX, 2 * cap)
            base, fill, start = base + start, fill - start, 0
            fill = min(cap, size - base)
            continue
        if cut:
            out.append(data[lo:lo + cut])
        start += cut


def grid(n_records):
    """the (max_reads, window_bytes) pairs every input is read with; window 0 = the whole input"""
    return [(mr if mr else n_records + 1, w if w else 0) for mr in MAX_READS for w in WINDOWS]


def fastq_inputs(block):
    """name -> bytes: every case of fastq_cases.py and 400 seeded inputs (random strings, and valid records with one mutation)"""
    c = dict(QC.cases(block))
    for k in range(FUZZ_CASES // 2):
        c[f"fuzz_bytes({SEED}, {k})"] = QC.fuzz_bytes(SEED, k, block)
        c[f"fuzz_mutated({SEED}, {k})"] = QC.fuzz_mutated(SEED, k, block)
    return c


def fuzz_fasta_records(seed, case, block):
    """records of 0 .. 3 lines of 0 .. 12 symbols, 20 % of the lines with CR LF, a third with text in front of the first header, a
    quarter without a final LF; every 25th case is several blocks long"""
    rng = np.random.default_rng([seed, 3, case])
    eol = lambda: b"\r\n" if rng.random() < 0.2 else b"\n"
    pick = lambda alphabet, k: bytes(alphabet[i] for i in rng.integers(0, len(alphabet), size=int(k)))
    n_rec = int(rng.integers(0, 9)) if case % 25 != 24 else int(rng.integers(block // 16, block // 4))
    out = [pick(b"ACGT>\n", rng.integers(1, 30)).lstrip(b">") + b"\n"] if rng.random() < 0.33 else []
    for _ in range(n_rec):
        out.append(b">" + pick(b"r> ", rng.integers(0, 4)) + eol())
        for _ in range(int(rng.integers(0, 4))):
            out.append(pick(b"ACGTN", rng.integers(0, 13)) + pick(b">", rng.integers(0, 2)) + eol())
    data = b"".join(out)
    return data[:-1] if data and rng.random() < 0.25 else data


def fasta_inputs(block):
    """name -> bytes: every case of fasta_cases.py and 400 seeded inputs (random strings, and records of several lines)"""
    c = dict(FC.cases(block))
    for k in range(FUZZ_CASES // 2):
        c[f"fuzz_bytes({SEED}, {k})"] = FC.fuzz_bytes(SEED, k, block)
        c[f"fuzz_fasta_records({SEED}, {k})"] = fuzz_fasta_records(SEED, k, block)
    return c


def inputs(fmt, block):
    return fastq_inputs(block) if fmt == FASTQ else fasta_inputs(block)


def parse(fmt, data):
    """the format's rule per byte (fastq_cases / fasta_cases model_parse) -> (text, doc_off), or (line, reason) of a FASTQ refusal"""
    return QC.model_parse(data) if fmt == FASTQ else FC.model_parse(data)


def seeded_verdicts(n, seed=SEED):
    """a VERDICT array with every type, taxa and similarities of many widths"""
    from lime_amd import api
    rng = np.random.default_rng([seed, 9])
    v = np.zeros(n, dtype=api.VERDICT)
    v["type"] = np.frombuffer(b"CUAH", dtype=np.uint8)[rng.integers(0, 4, size=n)]
    v["taxon"] = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32) >> rng.integers(0, 32, size=n).astype(np.uint32)
    v["sim"] = (rng.integers(0, 1000, size=n) / np.float32(7.0)).astype(np.float32) * (rng.random(n) < 0.9)
    v["rule"] = rng.integers(0, 4, size=n)
    return v
