"""The device FASTA parser's and the device reverse complement's cases, with numpy models of both (lime_amd/csrc/lime_fasta_kernel.hip
states the rule per byte).  tests/test_fasta_cases_cpu.py holds the models against lime_fasta_read without a GPU;
tests/test_fasta_edges_gpu.py holds the kernels against lime_fasta_read (the parser) and against the model (the reverse complement,
whose inputs may hold 0x0A and 0x0D as symbols, which no FASTA file can say)."""
import numpy as np

SEED = 20261
FUZZ_CASES = 200
ALPHABET = np.frombuffer(b">\n\rACgN ", dtype=np.uint8)
WEIGHTS = np.array([3, 4, 1, 2, 2, 1, 1, 1], dtype=np.float64) / 15.0      # '>' and '\n' frequent

_FROM, _TO = b"ATCGURYKMBVDH", b"TAGCAYRMKVBHD"
COMP = np.arange(256, dtype=np.uint8)
for _f, _t in zip(_FROM, _TO):
    COMP[_f] = _t
    COMP[_f | 0x20] = _t | 0x20


def model_parse(data):
    """the rule per byte -> (text uint8[n_text], doc_off uint64[n_docs + 1])"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(a)
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    line_first = np.ones(n, dtype=bool)
    line_first[1:] = a[:-1] == 10
    last_first = np.maximum.accumulate(np.where(line_first, np.arange(n), 0))          # L(i)
    in_header = a[last_first] == ord(">")
    header_start = line_first & (a == ord(">"))
    keep = (a != 10) & (a != 13) & ~in_header & (np.cumsum(header_start) > 0)
    kept_before = np.cumsum(keep) - keep
    doc_off = np.concatenate([kept_before[header_start], [keep.sum()]]).astype(np.uint64)
    return a[keep].copy(), doc_off


def model_revcomp(text, doc_off):
    """out[doc_off[d] + k] = COMP[text[doc_off[d + 1] - 1 - k]]"""
    text = np.asarray(text, dtype=np.uint8)
    off = np.asarray(doc_off, dtype=np.int64)
    n = int(off[-1])
    if n == 0:
        return np.zeros(0, np.uint8)
    p = np.arange(n, dtype=np.int64)
    d = np.searchsorted(off, p, side="right") - 1
    return COMP[text[off[d] + off[d + 1] - 1 - p]]


def records(docs):
    """list of bytes -> (text, doc_off) as the models return them"""
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    if docs:
        off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), off


def two_line_records(size):
    return (b">r\nACGTNACGT\n" * (size // 13 + 1))[:size]


def edge_triples(w):
    """at a width w of the kernels (a lane's 16 bytes, a wave's 1024, a block's): inputs one below, at and one above it, '\\n' as the last
    byte of a unit with '>' as the first of the next, a line-first '>' as the last byte of a unit, and '\\r\\n' split by the edge"""
    out = {}
    for size in (w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1):
        out[f"{size} bytes (width {w})"] = two_line_records(size)
    out[f"newline ends a unit, '>' starts the next (width {w})"] = b">a\n" + b"A" * (w - 4) + b"\n" + b">b\nCC\n"
    out[f"a line-first '>' ends a unit (width {w})"] = b">a\n" + b"A" * (w - 5) + b"\n" + b">" + b"hdr\nCC\n"
    out[f"CR LF split by the edge (width {w})"] = b">a\n" + b"A" * (w - 4) + b"\r" + b"\nCC\n"
    return out


def cases(block):
    """name -> bytes; `block` = api.FASTA_BLOCK"""
    b = block
    c = {
        "empty": b"",
        "no header": b"ACGT\nAC\n",
        "text in front of the first header": b"ACGT\nTT\n>h\nAC\n",
        "text longer than a block in front of the first header": b"A" * (b + 37) + b"\n>h\nACGT\n",
        "lines of two blocks in front of the first header": b"ACGTACGT\n" * (2 * b // 9 + 5) + b">h\nAC",
        "header at byte 0": b">h\nACGT\n",
        "only '>'": b">",
        "header only, no newline": b">h",
        "header only": b">h\n",
        "headers only": b">a\n>b\n>c",
        "consecutive headers and empty records": b">a\n>b\nAC\n>c\n\n>d\n",
        "blank lines": b">a\n\n\nAC\n\nGT\n\n",
        "CRLF": b">a\r\nAC\r\nGT\r\n>b\r\nTT\r\n",
        "'>' in mid-line": b">a\nAC>GT\nA>\n",
        "'>' right after a lone CR": b">a\nAC\r>GT\n\r>x\n",
        "no trailing newline": b">a\nACGT",
        "every byte value in one run": b">a\n" + bytes(range(256)) + b"\n",
        "every byte value on a line of its own": b">a\n" + b"".join(bytes([v]) + b"\n" for v in range(256)),
        "a header line from block 0 into block 3": b">a\nAC\n>" + b"h" * (3 * b) + b"\nACGT\n>b\nTT\n",
        "a symbol line from block 0 into block 3": b">a\n" + b"ACGT" * (3 * b // 4) + b"\nGG\n",
        "no newline at all, '>' first": b">" + b"A" * (3 * b + 4),
        "no newline at all, 'A' first": b"A" * (3 * b + 5),
    }
    for w in (16, 1024, b):
        c.update(edge_triples(w))
    return c


def fuzz_bytes(seed, case, block):
    """bytes over '> \\n \\r A C g N space': lengths 0 .. 200, every 25th case several blocks long"""
    rng = np.random.default_rng([seed, case])
    n = int(rng.integers(0, 201)) if case % 25 != 24 else int(rng.integers(1, 4)) * block + int(rng.integers(0, block))
    return ALPHABET[rng.choice(len(ALPHABET), size=n, p=WEIGHTS)].tobytes()


IUPAC = b"ACGTURYKMBVDHSWN"


def revcomp_collections(block):
    """name -> list of documents (bytes of any value)"""
    rng = np.random.default_rng([SEED, 7])
    any_bytes = lambda n: rng.integers(0, 256, size=int(n), dtype=np.uint8).tobytes()
    return {
        "every length 0 .. 130": [any_bytes(n) for n in range(131)],
        "lengths around 256 and 4096, and three blocks + 1": [any_bytes(n) for n in (255, 256, 257, 4095, 4096, 4097, 3 * block + 1, 0, 1)],
        "every byte value": [bytes(range(256)), b"", bytes(range(255, -1, -1)), bytes([10, 13, 62])],
        "IUPAC letters in both cases": [IUPAC, IUPAC.lower(), IUPAC + IUPAC.lower(), b"a", b"T"],
    }
