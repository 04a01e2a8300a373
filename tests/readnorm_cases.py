"""What the tests of the per-read norm share (test_readnorm_cases_cpu.py, test_readnorm_edges_gpu.py, test_readnorm_sample_gpu.py): the
numpy model of the norms (lime_docs_norms_dev), of clusterChoose with a norm per read (lime_lists_concat_norms_dev) and the grouping that
makes the fixed-norm path the oracle of the per-read one.  A read's rows, and so its verdict, depend on no other read: the per-read result
of read r is the fixed-norm result of r computed with r's own norms.  So the reads are grouped by their tuple of norms (one per list), the
existing fixed-norm call runs once per group on the WHOLE input, and each read is taken from its group's run.  The models of
tests/classify_cases.py and tests/shard_cases.py are used as they are (model_decide takes one norm per list).  No GPU and no library call
here."""
import numpy as np

from tests import classify_cases as CC
from tests import shard_cases as HC

SEED = 20412
BETAS = (0.0, 0.02, 0.25)
MATE_NORMS = (1, 50, 85, 100, 255)                  # what the classify tests draw a read's norm in a mate from
MAX_LEN = 255                                       # the longest read a norm byte serves (and --readlen names)


# ---- the norms ---------------------------------------------------------------------------------------------------------------------
def norms_of(lengths, alpha):
    """-> (norm u8[n], indices of the reads longer than 255): len + 1 - alpha where len >= alpha, else 1"""
    lengths = np.asarray(lengths, dtype=np.int64)
    norm = np.where(lengths >= alpha, lengths + 1 - alpha, 1)
    long_ = np.nonzero(lengths > MAX_LEN)[0]
    norm[long_] = 0                                 # (unspecified by the contract; the call is refused)
    return norm.astype(np.uint8), long_


def doc_off_of(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64), out=off[1:])
    return off


# ---- clusterChoose with a norm per read -----------------------------------------------------------------------------------------------
def pass_table(beta):
    """the 256 x 256 table of the per-read test: row n is shard_cases.passes for norm n, row 0 all false"""
    t = np.zeros((256, 256), dtype=bool)
    mx = np.arange(256)
    for n in range(1, 256):
        t[n] = HC.passes(mx, n, beta)
    return t


def choose_norms(table, norms, beta):
    """clusterChoose of a whole table, read r tested with norms[r] -> (row_max, row_off, pairs) like shard_cases.choose"""
    table = np.asarray(table, dtype=np.uint8)
    n_reads = table.shape[0]
    row_max = table.max(axis=1).astype(np.uint8) if table.shape[1] else np.zeros(n_reads, np.uint8)
    keep = pass_table(beta)[np.asarray(norms, dtype=np.int64), row_max.astype(np.int64)] if n_reads else np.zeros(0, bool)
    rows, cols = np.nonzero(table * keep[:, None])
    pairs = np.stack([cols.astype(np.uint32), table[rows, cols].astype(np.uint32)], axis=1).reshape(-1, 2)
    row_off = np.zeros(n_reads + 1, dtype=np.uint64)
    np.cumsum(np.bincount(rows, minlength=n_reads), out=row_off[1:])
    return row_max, row_off, pairs


def choose_by_groups(table, norms, beta):
    """the same from the fixed-norm model alone: shard_cases.choose once per distinct norm, every read's row from the run of its norm"""
    table = np.asarray(table, dtype=np.uint8)
    norms = np.asarray(norms)
    runs = {int(n): HC.choose(table, int(n), beta) for n in np.unique(norms)}
    row_max = table.max(axis=1).astype(np.uint8) if table.shape[1] else np.zeros(len(table), np.uint8)
    out, row_off = [], np.zeros(len(table) + 1, dtype=np.uint64)
    for r in range(len(table)):
        _, off, pairs = runs[int(norms[r])]
        p = pairs[int(off[r]):int(off[r + 1])]
        out.append(p)
        row_off[r + 1] = row_off[r] + np.uint64(len(p))
    pairs = (np.concatenate(out) if out else np.zeros((0, 2), np.uint32)).astype(np.uint32).reshape(-1, 2)
    return row_max, row_off, pairs


def threshold_rows(beta):
    """for every norm 1 .. 255 two rows whose maxima sit on either side of `float(max) / norm > beta`: the largest maximum that fails and
    the smallest that passes (where a byte holds one) -> (table u8[n, 3], norms u8[n], passes bool[n])"""
    rows, norms, want = [], [], []
    for n in range(1, 256):
        ok = HC.passes(np.arange(256), n, beta)
        first = int(np.argmax(ok)) if ok.any() else None
        for mx in ([first - 1, first] if first is not None else [255]):
            if mx is None or mx < 0:
                continue
            rows.append([mx, mx // 2, 0]); norms.append(n); want.append(bool(ok[mx]))
    return np.array(rows, dtype=np.uint8), np.array(norms, dtype=np.uint8), np.array(want, dtype=bool)


# ---- Classify with a norm per list and read ------------------------------------------------------------------------------------------
def draw_norms(n_files, n_reads, rng, choices=MATE_NORMS):
    """a norm per mate and read (F and RC of a mate share it: lists 0, 1 are mate 0's; lists 2, 3 mate 1's) -> [u8[n_reads]] per list"""
    per_mate = [rng.choice(choices, size=n_reads).astype(np.uint8) for _ in range(max(1, n_files // 2))]
    return [per_mate[i // 2] for i in range(n_files)]


def lists_norms(col, read_norms):
    """the collection's lists with the test taken per read (what lime_lists_concat_norms_dev leaves)"""
    return [choose_norms(s, nm, col["beta"]) for s, nm in zip(col["sims"], read_norms)]


def groups_of(read_norms):
    """{tuple of norms (one per list): indices of the reads that have it}"""
    key = np.stack([np.asarray(a, dtype=np.int64) for a in read_norms], axis=1)
    out = {}
    for r, k in enumerate(map(tuple, key)):
        out.setdefault(tuple(int(x) for x in k), []).append(r)
    return {k: np.array(v) for k, v in out.items()}


def by_groups(col, read_norms, run, subset=False):
    """run(lists, norms) -> per-read results, called once per group with the fixed-norm lists of the WHOLE collection; every read is
    taken from its group's run -> list of per-read results.  subset: the group's run sees the group's reads only (the slow numpy model: a
    read's verdict depends on no other read, which the whole-input runs of the library show)"""
    n_reads = col["sims"][0].shape[0]
    out = [None] * n_reads
    for key, reads in groups_of(read_norms).items():
        sims = [s[reads] for s in col["sims"]] if subset else col["sims"]
        lists = [CC.lists_of(s, n, col["beta"]) for s, n in zip(sims, key)]
        res = run(lists, list(key))
        for k, r in enumerate(reads):
            out[int(r)] = res[k if subset else int(r)]
    return out


def model_by_groups(col, read_norms, rank, higher, binary, subset=False):
    n_files, n_targ = len(col["sims"]), col["n_targ"]
    tax = CC.Tax(col["tax"], rank, higher, n_targ)
    return by_groups(col, read_norms, lambda lists, norms: CC.model_decide(lists, norms, [col["beta"]] * n_files, n_targ, tax, binary), subset)


def mixed_tolerance(n_files, n_reads, n_targ, seed):
    """tolerance_tables of norm 50 and of norm 100 in one collection: even reads from the first with norm 50, odd reads from the second
    with norm 100 -> (collection, read_norms)"""
    a = CC.tolerance_tables(n_files, n_reads, n_targ, seed, 50)
    b = CC.tolerance_tables(n_files, n_reads, n_targ, seed, 100)
    odd = np.arange(n_reads) % 2 == 1
    sims = [np.where(odd[:, None], sb, sa).astype(np.uint8) for sa, sb in zip(a["sims"], b["sims"])]
    col = dict(sims=sims, norm=None, beta=0.0, n_targ=n_targ, tax=a["tax"], name=f"tol50+100_{n_files}")
    nm = np.where(odd, 100, 50).astype(np.uint8)
    return col, [nm] * n_files


# ---- reads of mixed lengths ---------------------------------------------------------------------------------------------------------
def trim_fastq(data, every=2, keep=75, short=None):
    """four-line FASTQ bytes with every `every`-th record (1, 3, ... for 2) cut to its first `keep` symbols, sequence and quality alike;
    short = {record: length} cuts those records further -> (bytes, lengths)"""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines = lines[:-1]
    assert len(lines) % 4 == 0
    out, lengths = [], []
    for r in range(len(lines) // 4):
        h, s, p, q = lines[4 * r:4 * r + 4]
        n = len(s)
        if r % every == every - 1:
            n = min(n, keep)
        if short and r in short:
            n = min(n, short[r])
        out += [h, s[:n], p, q[:n]]
        lengths.append(n)
    return b"\n".join(out) + b"\n", np.array(lengths)


def fastq_of(reads, name="r"):
    """four-line FASTQ bytes of a list of sequences (bytes)"""
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (name.encode(), i, s, b"I" * len(s)) for i, s in enumerate(reads))


def fasta_of(reads, name="r"):
    return b"".join(b">%s%d\n%s\n" % (name.encode(), i, s) for i, s in enumerate(reads))
