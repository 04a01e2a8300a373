"""The hand-over between a wave's consecutive reads (walk_reads in lime_amd/csrc/lime_reads.h, on which k_adapter_bounds, k_filter_bounds and
k_qc_reads stand, and k_overlap_bounds' own walk over pairs): one collection through Context.docs_trim_adapter, docs_filter, docs_qc (with
and without qualities) and docs_trim_overlap, every output array, count and table equal to the host oracle's (api.adapter_trim, read_filter,
read_qc, overlap_trim).
The collection holds 2 * 8192 + 3 reads: the first three waves of the grid make three trips and all others two, and the last trip of most
waves is the one that asks for nothing more.  Read r has LENS[r % 12] symbols; 8192 % 12 == 8, so a wave's reads r, r + 8192, r + 16384
take three different entries, and every wave hands over between an empty, a one-word, a two-word and a longer read in some order.  Reads 0,
8191, 8192 and the last one are, in two more variants, all empty and all of 300 symbols.  Mate 2 of pair r has LENS[(r + 5) % 12] symbols.
What a stale word, length or offset of the read before would change is planted: an adapter, a poly-G tail, N's, lower case, reads of one
base, and for the pairs a fragment shorter than the mates in about half.
The per-kernel edge tests (tests/test_adapter_edges_gpu.py and its three siblings) hold each rule at its own edges."""
import functools

import numpy as np
import pytest

from tests import adapter_cases as A
from tests import filter_cases as F
from tests import overlap_cases as V
from tests import qc_cases as Q

pytestmark = pytest.mark.gpu

SEED = 20318
TRIP = A.READS_PER_TRIP
N = 2 * TRIP + 3
LENS = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300]
ENDS = (0, TRIP - 1, TRIP, N - 1)                # the reads whose length a variant forces
VARIANTS = {"the list": None, "ends empty": 0, "ends of 300": 300}
A20 = A.TRUSEQ_R1[:20]
ADAPTER = (A20, 3, 10)
FILTER = F.params(polyx="G", polyx_min=10, max_len=250, min_len=30, max_n=2, min_complexity=30)
OVERLAP = (20, 10)
N_POS = 100                                      # reads of 127 symbols and more reach the pool


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


def _lengths(forced, shift=0):
    lens = [LENS[(r + shift) % 12] for r in range(N)]
    if forced is not None:
        for r in ENDS:
            lens[r] = forced
    return lens


def _read(rng, L):
    r = A.bases(rng, L)
    u = rng.random()
    if L >= 63 and u < 0.33:                     # read-through into the adapter, up to two of its symbols changed
        r = A.plant(rng, r, int(rng.integers(0, L - 10)), A20, int(rng.integers(0, 3)))
    elif L >= 63 and u < 0.53:
        r = F.plant(rng, r, int(rng.integers(10, 61)), b"G", 0.05)
    elif L >= 63 and u < 0.56:
        r = b"A" * L
    v = rng.random()
    if v < 0.1 and L:
        b = bytearray(r)
        for j in rng.integers(0, L, size=int(rng.integers(1, 5))):
            b[j] = ord("N")
        r = bytes(b)
    elif v < 0.2:
        r = r.lower()
    return r


@functools.lru_cache(maxsize=None)
def _collection(variant):
    """-> (reads, their qualities, their mates): made once per variant and left as they are"""
    assert TRIP == 8192 == F.READS_PER_TRIP == Q.READS_PER_TRIP == V.PAIRS_PER_TRIP and TRIP % 12 == 8
    rng = np.random.default_rng([SEED, sorted(VARIANTS).index(variant)])
    lens = _lengths(VARIANTS[variant])
    reads = [_read(rng, L) for L in lens]
    quals = [rng.integers(33, 74, size=L, dtype=np.uint8).tobytes() for L in lens]
    mates = []
    for a, Lb in zip(reads, _lengths(VARIANTS[variant], shift=5)):
        short = min(len(a), Lb)
        b = A.bases(rng, Lb)
        if short > OVERLAP[0] + 1 and rng.random() < 0.5:      # the fragment ends inside both mates: mate 2 runs into its adapter
            b = (V.revcomp(a[:int(rng.integers(OVERLAP[0], short))]) + A.TRUSEQ_R2 + b)[:Lb]
        mates.append(b)
    return reads, quals, mates


def _docs(ctx, reads):
    import torch
    text, off = A.records(reads)
    return ctx.docs_from_arrays_dev(torch.from_numpy(text).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), len(reads), len(text))


def _same(out, w_text, w_off, what):
    o_text, o_off = out.get()
    if not np.array_equal(o_off, w_off):
        bad = int(np.nonzero(o_off != w_off)[0][0]) - 1
        raise AssertionError(f"{what}: read {bad} keeps {int(o_off[bad + 1] - o_off[bad])} symbols, not {int(w_off[bad + 1] - w_off[bad])}")
    assert np.array_equal(o_text, w_text), what
    out.close()


def _kept(off, new_off):
    """how many reads the stage left as they were, how many it changed"""
    same = int((np.diff(off.astype(np.int64)) == np.diff(new_off.astype(np.int64))).sum())
    return same, len(off) - 1 - same


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_adapter_and_filter(ctx, variant):
    from lime_amd import api
    reads = _collection(variant)[0]
    text, off = A.records(reads)
    assert len(reads) == N and [len(reads[r]) for r in ENDS] == [_lengths(VARIANTS[variant])[r] for r in ENDS]
    d = _docs(ctx, reads)
    w_text, w_off, w_info = api.adapter_trim(text, off, *ADAPTER)
    same, changed = _kept(off, w_off)
    assert same > N // 4 and changed > N // 8 and w_info["n_changed"] == changed, (variant, w_info)      # the comparison has something to show
    out, info = ctx.docs_trim_adapter(d, *ADAPTER)
    _same(out, w_text, w_off, f"{variant}, adapter")
    assert info == w_info, (variant, info, w_info)
    w_text, w_off, w_info = api.read_filter(text, off, **FILTER)
    same, changed = _kept(off, w_off)
    assert same > N // 4 and changed > N // 8 and all(w_info[k] > 50 for k in ("n_polyx", "n_capped", "n_short", "n_many_n", "n_low_complexity")), (variant, w_info)
    out, info = ctx.docs_filter(d, **FILTER)
    _same(out, w_text, w_off, f"{variant}, filter")
    assert info == w_info, (variant, info, w_info)
    d.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_qc_with_and_without_qualities(ctx, variant):
    from lime_amd import api
    reads, quals = _collection(variant)[:2]
    text, q, off = Q.flat(reads, quals)
    for with_qual in (True, False):
        d = ctx.docs_from_fastq_qual_bytes(Q.fastq_of(reads, quals)) if with_qual else _docs(ctx, reads)
        assert d.has_qual == with_qual and d.info() == (N, len(text))
        want = api.read_qc(text, off, N_POS, qual=q if with_qual else None)
        rows = want["rows"]
        # every class at every position and in the pool; lengths 0, 1, 63, 64, 65 and the pooled ones
        assert rows[:, :5].all() and np.count_nonzero(want["len_hist"]) == 6 and np.count_nonzero(want["gc_hist"]) > 20, variant
        if with_qual:
            assert rows[:, 5:].all() and np.count_nonzero(want["mq_hist"]) > 5, variant
        else:
            assert not rows[:, 5:].any() and not want["mq_hist"].any(), variant
        got = ctx.docs_qc(d, N_POS)
        for key in Q.KEYS:
            assert np.array_equal(got[key], want[key]), (variant, with_qual, key, np.nonzero(got[key] != want[key]))
        assert np.array_equal(got["tables"], want["tables"])
        d.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_overlap(ctx, variant):
    from lime_amd import api
    r1, _, r2 = _collection(variant)
    assert [len(b) for b in r2[1:13]] == [LENS[(r + 5) % 12] for r in range(1, 13)]
    (t1, f1), (t2, f2) = A.records(r1), A.records(r2)
    w1, g1, w2, g2, w_ins, w_info = api.overlap_trim(t1, f1, t2, f2, *OVERLAP)
    assert w_info["n_overlap"] > N // 8 and w_info["n_cut"] > N // 8 and int((w_ins == 0).sum()) > N // 4, (variant, w_info)
    d1, d2 = _docs(ctx, r1), _docs(ctx, r2)
    o1, o2, info, ins = ctx.docs_trim_overlap(d1, d2, *OVERLAP, want_insert=True)
    if not np.array_equal(ins, w_ins):
        bad = int(np.nonzero(ins != w_ins)[0][0])
        raise AssertionError(f"{variant}: pair {bad} of {len(r1[bad])} / {len(r2[bad])} symbols has insert {int(ins[bad])}, not {int(w_ins[bad])}")
    _same(o1, w1, g1, f"{variant}, mate 1")
    _same(o2, w2, g2, f"{variant}, mate 2")
    assert info == w_info, (variant, info, w_info)
    d1.close(); d2.close()
