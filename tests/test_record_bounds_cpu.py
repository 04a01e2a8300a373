"""The bound behind LIME_ERR_DOCID, proved on the CPU: whatever document id a scored pair carries, what the scan stores for it
(a 4-byte update record, a stand-in, or nothing) lands in a bin below n_bins and a sub-region below n_sub under the partition
kernels' own function.  The arithmetic under test is the ONE definition in lime_amd/csrc/lime_device.h that the scan and the
partition kernels share (genome_ok, rec_of, rec_sub2, rec_bin), reached through its exported wrappers lime_rec_*; the layouts
(bin_shift, n_bins, sub-regions) come from the library's own computation (lime_rec_layout), not from a restatement here.  The
reference in this file is plain Python / numpy on 64-bit integers without wrap-around.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lime_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the kernel files: all the scan, scorer, partition and apply code, joined
KERNELS = [os.path.join(ROOT, "lime_amd", "csrc", f) for f in ("lime_kernels.hip", "lime_partition.hip", "lime_apply.hip")]


class Layout(C.Structure):
    _fields_ = [("n_bins", C.c_uint32), ("bin_shift", C.c_uint32), ("n_sub", C.c_uint32), ("sub_rb", C.c_uint32), ("sub_gb", C.c_uint32)]


# (n_reads, n_refs, LIME_BIN_LEVELS or None)
SHAPES = [
    # the shapes of tests/test_gpu_bad_docid.py
    (3000, 300, None), (3000, 300, (1, 1)), (3000, 300, (4, 7)), (40000, 700, None), (40000, 700, (1, 1)), (40000, 700, (4, 7)),
    (1_100_000, 4000, None), (3_000_000, 3423, None), (2_200_000, 4000, None), (4_700_000, 4000, None), (1, 2, None),
    # tables of exactly k * 2^32 bytes, and one byte less / more
    (1 << 24, 256, None), (1 << 31, 2, None), (1 << 25, 256, None),                    # 2^32, 2^32, 2^33
    (16843009, 255, None), (6700417, 641, None),                                       # 2^32 - 1, 2^32 + 1
    (599479, 14329, None), (2863311531, 3, None),                                      # 2^33 - 1, 2^33 + 1
    # n_refs = 1, 2, 255, 256, 4000, 2^25 - 1
    (100_000, 1, None), (5_000_000, 2, None), (70_000, 255, None), (70_000, 256, None), (1_073_742, 4000, None),
    (128, (1 << 25) - 1, None), (129, (1 << 25) - 1, None), (256, (1 << 25) - 1, None), (1, (1 << 25) - 1, None),
]


def layout_of(lib, nr, ng, levels):
    lay = Layout()
    one, two = levels if levels else (0, 0)
    assert lib.lime_rec_layout(nr, ng, one, two, C.byref(lay)) == 0, lib.lime_last_error()
    return lay


def batch(lib, rd, gd, ng, lay, fixed_slot):
    n = len(rd)
    rd = np.ascontiguousarray(rd, np.uint32); gd = np.ascontiguousarray(gd, np.uint32)
    valid = np.empty(n, np.uint8); stored = np.empty(n, np.uint8)
    rec = np.empty(n, np.uint32); sub = np.empty(n, np.uint32); bn = np.empty(n, np.uint32)
    rc = lib.lime_rec_batch(rd.ctypes.data, gd.ctypes.data, n, ng, C.byref(lay), fixed_slot, valid.ctypes.data, stored.ctypes.data,
                            rec.ctypes.data, sub.ctypes.data, bn.ctypes.data)
    assert rc == 0, lib.lime_last_error()
    return valid.astype(bool), stored.astype(bool), rec, sub, bn


def edge_ids(nr, ng):
    """genome indices gd = da - n_reads of the malformed ids the issue lists (and their neighbours), as 64-bit numbers below 2^32"""
    e = [ng, ng + 1, 1 << 25, (1 << 25) + (ng - 1) // 2, (1 << 25) + ng - 1, 1 << 31, 0xFFFFFFFF - nr, 0xFFFFFFEF - nr,
         (1 << 32) - nr - 1, (1 << 26) + 1, (1 << 25) * 3 + ng // 3]
    return sorted({x for x in e if ng <= x < (1 << 32) - nr})


@pytest.mark.parametrize("nr,ng,levels", SHAPES)
def test_layout_covers_the_table(nr, ng, levels):
    lib = _lib.load()
    lay = layout_of(lib, nr, ng, levels)
    cells = nr * ng
    assert 16 <= lay.bin_shift <= 25 and 1 <= lay.n_bins <= 3072
    assert lay.n_bins == ((cells + 15) // 16 * 16 + (1 << lay.bin_shift) - 1) >> lay.bin_shift
    assert lay.n_sub == ((cells + 15) // 16 * 16 + (1 << 32) - 1) >> 32 <= 8
    if lay.n_sub == 2:
        assert lay.sub_rb * ng + lay.sub_gb == 1 << 32 and lay.sub_gb < ng


@pytest.mark.parametrize("nr,ng,levels", SHAPES)
def test_in_range_pairs_give_the_cell(nr, ng, levels):
    """rec, sub-region and bin of a valid pair are the low word, the high word and the shifted value of cell = rd * n_refs + gd"""
    lib = _lib.load()
    lay = layout_of(lib, nr, ng, levels)
    rng = np.random.default_rng(1000 + nr % 977 + ng)
    n = 300_000
    rd = rng.integers(0, nr, n, dtype=np.uint64)
    gd = rng.integers(0, ng, n, dtype=np.uint64)
    # edges: first / last rows and columns, the rows around every multiple of 2^32
    er, eg = [0, 0, nr - 1, nr - 1], [0, ng - 1, 0, ng - 1]
    for k in range(1, lay.n_sub):
        r0 = (k << 32) // ng
        for r in (r0 - 1, r0, r0 + 1):
            if 0 <= r < nr:
                g0 = (k << 32) - r0 * ng
                for g in (0, ng - 1, g0 - 1, g0, g0 + 1):
                    if 0 <= g < ng:
                        er.append(r); eg.append(g)
    rd = np.concatenate([rd, np.array(er, np.uint64)]); gd = np.concatenate([gd, np.array(eg, np.uint64)])
    cell = rd * np.uint64(ng) + gd                                         # < 2^40: no wrap in 64 bits
    assert int(cell.max()) < nr * ng
    for fixed in (0, 1):
        valid, stored, rec, sub, bn = batch(lib, rd, gd, ng, lay, fixed)
        assert valid.all() and stored.all()
        assert np.array_equal(rec.astype(np.uint64), cell & np.uint64(0xFFFFFFFF))
        assert np.array_equal(sub.astype(np.uint64), cell >> np.uint64(32))
        assert np.array_equal(bn.astype(np.uint64), cell >> np.uint64(lay.bin_shift))
        assert int(bn.max()) < lay.n_bins and int(sub.max()) < lay.n_sub
    # the thin wrappers one by one, on the edges
    for r, g in zip(er, eg):
        c = r * ng + g
        assert lib.lime_rec_valid(g, ng) == 1
        assert lib.lime_rec_of(r, g, ng) == c & 0xFFFFFFFF
        if lay.n_sub == 2:
            assert lib.lime_rec_sub2(r, g, lay.sub_rb, lay.sub_gb) == c >> 32
        assert lib.lime_rec_bin(c & 0xFFFFFFFF, c >> 32, lay.bin_shift) == c >> lay.bin_shift


@pytest.mark.parametrize("nr,ng,levels", SHAPES)
def test_any_pair_stays_inside_the_layout(nr, ng, levels):
    """Any (rd, gd), gd on all 32 bits: the validity test says bad exactly when gd >= n_refs, and whatever the scan stores -- nothing,
    or the stand-in of a slot handed out in advance -- has bin < n_bins and sub-region < n_sub under the partition kernels' function."""
    lib = _lib.load()
    lay = layout_of(lib, nr, ng, levels)
    rng = np.random.default_rng(2000 + nr % 977 + ng)
    n = 300_000
    hi = (1 << 32) - nr                                                   # gd = da - n_reads with da < 2^32
    rd = rng.integers(0, nr, n, dtype=np.uint64)
    gd = rng.integers(0, hi, n, dtype=np.uint64)
    gd[::3] = ng + rng.integers(0, 4 * ng + 64, len(gd[::3]), dtype=np.uint64) % np.uint64(hi - ng)      # just beyond the table
    gd[1::7] = (np.uint64(1 << 25) * rng.integers(1, 100, len(gd[1::7]), dtype=np.uint64) + rng.integers(0, ng, len(gd[1::7]), dtype=np.uint64)) % np.uint64(hi)   # low 25 bits valid
    gd[2::11] = rng.integers(0, ng, len(gd[2::11]), dtype=np.uint64)         # and valid ones among them
    ids = edge_ids(nr, ng)
    er = [r for r in (0, nr // 2, nr - 1) for _ in ids]
    eg = [g for _ in range(3) for g in ids]
    rd = np.concatenate([rd, np.array(er, np.uint64)]); gd = np.concatenate([gd, np.array(eg, np.uint64)])
    ok = gd < np.uint64(ng)
    assert (~ok).sum() > n // 3
    for fixed in (0, 1):
        valid, stored, rec, sub, bn = batch(lib, rd, gd, ng, lay, fixed)
        assert np.array_equal(valid, ok)                                   # full width: no masking in front of the comparison
        assert stored[ok].all()
        if not fixed or lay.n_sub != 1:
            assert not stored[~ok].any()                                   # a bad id leaves nothing
        assert int(bn[stored].max()) < lay.n_bins and int(sub[stored].max()) < lay.n_sub
        cell = sub[stored].astype(np.uint64) << np.uint64(32) | rec[stored].astype(np.uint64)
        assert int(cell.max()) < nr * ng                                   # ... and is a cell of the table
    for g in ids:
        assert lib.lime_rec_valid(g, ng) == 0, g
    assert lib.lime_rec_valid(ng - 1, ng) == 1


# ---- source tripwire -----------------------------------------------------------------------------------------------------
def _block_after(src, pos):
    """src from the start of the line holding `pos` to the end of the brace block that encloses it"""
    start = src.rfind("\n", 0, pos) + 1
    depth = 0
    for i in range(pos, len(src)):
        ch = src[i]
        if ch == "{":
            depth += 1
        elif ch == "}":
            depth -= 1
            if depth < 0:
                return src[start:i]
    return src[start:]


def test_every_genome_index_passes_the_shared_validity_test():
    """Every site of the kernel files (KERNELS) that turns a da value into a genome index (`- a.n_reads`) calls genome_ok (lime_device.h) in the same
    block, before anything is stored for it -- a new fast emitter cannot silently skip the test.  The queue / record stores of the scorers
    come only after it."""
    src = "\n".join(open(f).read() for f in KERNELS)
    src = re.sub(r"//[^\n]*", "", src)
    sites = [m.start() for m in re.finditer(r"-\s*a\.n_reads\b", src)]
    assert len(sites) >= 6, len(sites)                                     # emit, score_len2, score_small3 (two), score_rows3, k_score_big
    for pos in sites:
        blk = _block_after(src, pos)
        line = src.count("\n", 0, pos) + 1
        assert "genome_ok(" in blk, f"kernel files, joined, line {line}: a genome index is computed and never passed through genome_ok"
        for store in re.finditer(r"q[u]?\.q[rg]\[[^\]]*\]\s*=|put_rec\(", blk):
            assert "genome_ok(" in blk[:store.end() + 80], f"kernel files, joined, line {line}: stored before the validity test"
    # and no scorer packs a genome index into a queue entry by masking alone
    assert not re.search(r"q[u]?\.bad\s*\|=\s*\(uint32_t\)\s*\([^;]*>=\s*a\.n_refs", src), "a validity test written out by hand: use genome_ok"
    dev = open(os.path.join(ROOT, "lime_amd", "csrc", "lime_device.h")).read()
    assert re.search(r"bool\s+genome_ok\(uint32_t gd, uint32_t n_refs\)\s*\{\s*return gd < n_refs;\s*\}", dev)
    for fn in ("rec_of(", "rec_bin(", "rec_bin_at(", "rec_sub2("):
        assert src.count(fn) >= 2, f"{fn[:-1]} must serve the scan and the partition kernels / drains alike"
    # the partition kernels bin through the shared function only
    assert not re.search(r">>\s*sh\)\s*\+\s*(bo|t\.binoff|tc\.binoff)", src)
