"""The FASTQ parsers' cases, with two models of the format (include/lime_hip.h states it at lime_fastq_read; lime_amd/csrc/lime_fastq_kernel.hip
states the rule per byte): model_parse is that rule in numpy, split_parse a plain reader over data.split(b"\\n").  Either returns
(text, doc_off) for a valid input or (line, reason) for a refused one.  tests/test_fastq_cases_cpu.py holds both against lime_fastq_read
without a GPU; tests/test_fastq_edges_gpu.py holds the kernels against lime_fastq_read."""
import re

import numpy as np

SEED = 20265
FUZZ_CASES = 400
WIDTHS = (16, 1024, 4096)                       # a lane's bytes, a wave's, a block's
REASONS = ["record does not start with '@'", "separator line does not start with '+'", "quality length differs from sequence length",
           "truncated record"]
ALPHABET = np.frombuffer(b"@+\n\rACI", dtype=np.uint8)
WEIGHTS = np.array([2, 2, 5, 1, 2, 2, 3], dtype=np.float64) / 17.0


def is_refusal(r):
    return isinstance(r[0], (int, np.integer))


def refusal_of(message):
    """'<who>: line <L>: <reason>' -> (L, reason number)"""
    m = re.search(r"line (\d+): (.*)$", message)
    assert m and m.group(2) in REASONS, message
    return int(m.group(1)), REASONS.index(m.group(2))


def host_read(tmp_path, data, rc=0):
    """lime_fastq_read on a file of `data` -> (text, doc_off), or (line, reason) of a LIME_ERR_ARG refusal"""
    import ctypes as C
    import os
    from lime_amd import _lib
    lib = _lib.load()
    p = str(tmp_path / "in.fastq")
    with open(p, "wb") as f:
        f.write(data)
    pt, po, nd = C.c_void_p(), C.c_void_p(), C.c_uint32(7)
    code = lib.lime_fastq_read(os.fsencode(p), int(rc), C.byref(pt), C.byref(po), C.byref(nd))
    if code != 0:
        assert code == _lib.ERR_ARG and pt.value is None and po.value is None and nd.value == 0
        msg = lib.lime_last_error().decode()
        assert msg.startswith("lime_fastq_read: line "), msg
        return refusal_of(msg)
    try:
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(nd.value + 1,)).copy()
        text = np.frombuffer(C.string_at(pt, int(off[-1])), dtype=np.uint8).copy()
    finally:
        lib.lime_free(pt); lib.lime_free(po)
    return text, off


def model_parse(data):
    """the rule per byte; reason 2 by the identity: at every record's end the kept and the quality bytes so far are equally many"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    n = len(a)
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    nl = a == 10
    ln = np.cumsum(nl) - nl                                                 # an LF belongs to the line it ends
    line_first = np.ones(n, dtype=bool)
    line_first[1:] = nl[:-1]
    n_lines = int(nl.sum()) + int(a[-1] != 10)
    sym = ~nl & (a != 13)
    keep, qual = (ln % 4 == 1) & sym, (ln % 4 == 3) & sym
    last = np.zeros(n, dtype=bool)
    last[-1] = True
    end = (ln % 4 == 3) & (nl | last)
    keys = []                                                               # line * 4 + reason of every offence
    keys.extend(((ln[line_first & (ln % 4 == 0) & (a != ord("@"))] + 1) * 4 + 0).tolist())
    keys.extend(((ln[line_first & (ln % 4 == 2) & (a != ord("+"))] + 1) * 4 + 1).tolist())
    keys.extend(((ln[end & (np.cumsum(keep) != np.cumsum(qual))] + 1) * 4 + 2).tolist())
    if n_lines % 4:
        keys.append(n_lines * 4 + 3)
    if keys:
        return min(keys) // 4, min(keys) % 4
    kept_before = np.cumsum(keep) - keep
    doc_off = np.concatenate([kept_before[line_first & (ln % 4 == 0)], [keep.sum()]]).astype(np.uint64)
    assert len(doc_off) == n_lines // 4 + 1
    return a[keep].copy(), doc_off


def split_parse(data):
    """a plain reader, a record's quality length compared with its own sequence's"""
    lines = bytes(data).split(b"\n")
    if lines[-1] == b"":
        lines.pop()                                                         # nothing behind the last LF is no line
    reads, seq = [], b""
    for i, line in enumerate(lines):
        if i % 4 == 0 and not line.startswith(b"@"):
            return i + 1, 0
        if i % 4 == 1:
            seq = line.replace(b"\r", b"")
            reads.append(seq)
        if i % 4 == 2 and not line.startswith(b"+"):
            return i + 1, 1
        if i % 4 == 3 and len(line.replace(b"\r", b"")) != len(seq):
            return i + 1, 2
    if len(lines) % 4:
        return len(lines), 3
    return records(reads)


def records(docs):
    """list of bytes -> (text, doc_off) as the models return them"""
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    if docs:
        off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return np.frombuffer(b"".join(docs), dtype=np.uint8).copy(), off


def rec(header=b"r", seq=b"ACGT", qual=None, eol=b"\n", plus=b""):
    return b"@" + header + eol + seq + eol + b"+" + plus + eol + (b"I" * len(seq) if qual is None else qual) + eol


REC16 = rec(b"r1")                               # 16 bytes


def pad(size):
    """valid records of `size` bytes in all (0, or 6 and more), the last byte an LF"""
    assert size == 0 or size >= 6, size
    k = max(0, (size - 6) // 16)
    r = size - 16 * k                                                       # 6 .. 21, or 0
    tail = b"" if r == 0 else rec(b"" if r % 2 == 0 else b"h", b"ACGTTGCA"[:(r - 6) // 2])
    out = REC16 * k + tail
    assert len(out) == size
    return out


def fixed_records(n_rec):
    """n_rec records of 16 bytes with reads that differ: record k holds the 4 letters of k in base 4"""
    k = np.arange(n_rec, dtype=np.int64)
    a = np.tile(np.frombuffer(REC16, np.uint8), (n_rec, 1))
    for j in range(4):
        a[:, 4 + j] = np.frombuffer(b"ACGT", np.uint8)[(k >> (2 * j)) & 3]
    return a


def _broken(n_rec, where):
    """fixed_records(n_rec) with the records of `where` = {index: reason} broken in place (reasons 0, 1, 2; no byte more or less)"""
    a = fixed_records(n_rec)
    for k, reason in where.items():
        if reason == 0:
            a[k, 0] = ord("X")
        elif reason == 1:
            a[k, 9] = ord("-")
        else:
            a[k, 13] = 13                                                   # a quality byte becomes a CR: one short
    return a.tobytes()


def edge_cases(w):
    out = {}
    for size in (w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1):
        out[f"{size} bytes (width {w})"] = pad(size)
    out[f"LF ends a unit, '@' starts the next (width {w})"] = pad(w) + rec(b"x", b"CC")
    out[f"CR LF split by the edge (width {w})"] = pad(w - 16) + b"@r\nACGTACGTACGT\r" + b"\n+\nIIIIIIIIIIII\n" + rec()
    out[f"a record ends on the last byte of a unit, LF (width {w})"] = pad(w) + pad(7)
    out[f"a record ends on the last byte of a unit, no LF, end of input (width {w})"] = pad(w + 1)[:-1]
    for p in (w - 1, w):                                                    # the offending line's first byte at p: the last or the first byte of a unit
        out[f"reason 0 at byte {p} (width {w})"] = pad(p) + b"Xr\nAC\n+\nII\n" + rec()
        out[f"reason 0 at byte {p}, an empty line (width {w})"] = pad(p) + b"\nAC\n+\nII\n"
        out[f"reason 1 at byte {p} (width {w})"] = pad(p - 6) + b"@r\nAC\n" + b"-\nII\n" + rec()
        out[f"reason 2 with the quality line at byte {p} (width {w})"] = pad(p - 8) + b"@r\nAC\n+\n" + b"I\n" + rec()
        out[f"reason 2 with the record's end at byte {p} (width {w})"] = pad(p - 9) + b"@r\nAC\n+\nI\n" + rec()
        out[f"reason 3 with the last line at byte {p} (width {w})"] = pad(p) + b"@r"
        out[f"reason 3 with the last line at byte {p}, LF (width {w})"] = pad(p) + b"@r\n"
    return out


def cases(block):
    """name -> bytes; `block` = api.FASTA_BLOCK"""
    b = block
    per_block = b // 16
    n_rec = 3 * per_block + per_block // 2                                   # three and a half blocks of 16-byte records
    in0, in2, in3, last = 3, 2 * per_block + 5, 3 * per_block + 7, n_rec - 1
    c = {
        "empty": b"",
        "one record": rec(),
        "one record, no final LF": rec()[:-1],
        "CRLF throughout": rec(eol=b"\r\n") + rec(b"x y", b"TTGA", eol=b"\r\n"),
        "a lone CR inside a sequence": rec(seq=b"AC\rGT", qual=b"IIII") + rec(),
        "CRs in a quality line": rec(seq=b"ACGT", qual=b"I\rII\r\rI") + rec(),
        "empty reads": b"@x\n\n+\n\n" + rec() + b"@\n\n+\n\n@\n\n+\n\n",
        "only an empty read, no final LF": b"@x\n\n+\n",
        "a block of empty reads": b"@\n\n+\n\n" * (b // 6 + 2),
        "qualities beginning with '@' and '+'": rec(qual=b"@III") + rec(qual=b"+III") + rec(seq=b"A", qual=b"@") + rec(seq=b"C", qual=b"+") + rec(),
        "'+name' on the separator": rec(b"name", plus=b"name") + rec(plus=b"@x"),
        "'>' and every byte value in a header": rec(b">" + bytes(v for v in range(256) if v != 10)) + rec(b">"),
        "every byte value but LF and CR in a sequence": rec(seq=bytes(v for v in range(256) if v not in (10, 13))) + rec(),
        "a header line from block 0 into block 3": rec() + rec(b"h" * (3 * b)) + rec(seq=b"TT"),
        "a sequence line from block 0 into block 3": rec() + rec(seq=b"ACGT" * (3 * b // 4)) + rec(seq=b"GG"),
        "a quality line from block 0 into block 3": rec() + rec(seq=b"A", qual=b"I" + b"\r" * (3 * b)) + rec(seq=b"GG"),
        "a +1 then a -1 length mismatch": rec() + rec(qual=b"IIIII") + rec(qual=b"III") + rec(),
        "a mismatching last quality line without LF": rec() + b"@r\nACGT\n+\nIII",
        "a longer last quality line without LF": rec() + b"@r\nACGT\n+\nIIIII",
        "truncated after 1 line": rec() + b"@r\n",
        "truncated after 1 line, no LF": rec() + b"@r",
        "truncated after 2 lines": rec() + b"@r\nACGT\n",
        "truncated after 2 lines, no LF": rec() + b"@r\nACGT",
        "truncated after 3 lines": rec() + b"@r\nACGT\n+\n",
        "truncated after 3 lines, no LF": rec() + b"@r\nACGT\n+",
        "a truncated only record": b"@r\nACGT\n",
        "one byte, '@'": b"@",
        "one byte, not '@'": b"A",
        "one LF": b"\n",
        "a FASTA file": b">r\nACGT\n>s\nTT\n",
        "a block of only LFs": b"\n" * b,
        "a block of only LFs behind two records": rec() + rec() + b"\n" * (b + 5),
        "a wrapped sequence": b"@r\nACGT\nACGT\n+\nIIIIIIII\n",
        "several blocks of valid records": fixed_records(n_rec).tobytes(),
        "reason 3 in block 2": fixed_records(in2).tobytes() + b"@r\nAC\n+\n",
        "reason 3 in the last record": fixed_records(n_rec).tobytes()[:-6],
        "reason 2 in block 0 and reason 0 in block 3": _broken(n_rec, {in0: 2, in3: 0}),
        "reason 0 in block 0 and reason 2 in block 3": _broken(n_rec, {in0: 0, in3: 2}),
        "reason 1 in block 0 and reason 2 in block 3": _broken(n_rec, {in0: 1, in3: 2}),
        "reason 2 in block 2 and truncation at the end": _broken(n_rec, {in2: 2})[:-7],
        "reasons 0 and 3 on the last line": fixed_records(n_rec).tobytes() + b"r",
    }
    for reason in (0, 1, 2):
        for where, k in (("the first record", 0), ("a record in block 2", in2), ("the last record", last)):
            c[f"reason {reason} in {where}"] = _broken(n_rec, {k: reason})
    for w in WIDTHS:
        c.update(edge_cases(w))
    return c


def fuzz_bytes(seed, case, block):
    """bytes over '@ + LF CR A C I': lengths 0 .. 200, every 25th case several blocks long"""
    rng = np.random.default_rng([seed, 1, case])
    n = int(rng.integers(0, 201)) if case % 25 != 24 else int(rng.integers(1, 4)) * block + int(rng.integers(0, block))
    return ALPHABET[rng.choice(len(ALPHABET), size=n, p=WEIGHTS)].tobytes()


def fuzz_mutated(seed, case, block):
    """valid records with one mutation.  A record: '@' + 0 .. 3 bytes of 'r@+ ', a read of 0 .. 5 bases, qualities from '@+I!'; a line ends
    with CR LF in 20 % of the lines; a quarter of the inputs have no final LF; every 25th case is several blocks long.  The mutation: one
    byte deleted, one byte of '@ + LF CR A C I' inserted, or the input cut short."""
    rng = np.random.default_rng([seed, 2, case])
    pick = lambda alphabet, k: bytes(alphabet[i] for i in rng.integers(0, len(alphabet), size=int(k)))
    eol = lambda: b"\r\n" if rng.random() < 0.2 else b"\n"
    n_rec = int(rng.integers(1, 9)) if case % 25 != 24 else int(rng.integers(block // 8, block // 4))
    out = []
    for _ in range(n_rec):
        k = int(rng.integers(0, 6))
        out.append(b"@" + pick(b"r@+ ", rng.integers(0, 4)) + eol() + pick(b"ACGT", k) + eol() + b"+" + eol() + pick(b"@+I!", k) + eol())
    data = b"".join(out)
    if rng.random() < 0.25:
        data = data[:-1]
    kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(data)))
    if kind == 0:
        return data[:at] + data[at + 1:]
    if kind == 1:
        return data[:at] + pick(b"@+\n\rACI", 1) + data[at:]
    return data[:at]
