"""Reads merged into a prebuilt genome index on the device (lime_gindex_build / _save / _load, lime_merge_index, lime_merge_index_dev,
bin/BuildIndex's two-step forms).  The contract: the three arrays are bit for bit what lime_build_index gives for reads + genomes, so
lime_amd/builder.py stays the oracle; every comparison is np.array_equal / torch.equal on all three arrays, no tolerance anywhere.  The
collections are those of tests/merge_cases.py, whose Python model of the merge tests/test_merge_cases_cpu.py checks without a GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import index_cases as IC
from tests import merge_cases as MC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lime_amd", "bin")


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


def _same(got, want, what):
    diff = IC.first_difference(got, want)
    assert diff is None, f"{what}: {diff}"


def _host(tensors):
    e, l, d = tensors
    return e.cpu().numpy(), l.cpu().numpy().view(np.uint32), d.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _want(reads, genomes, term=0):
    from lime_amd.builder import build_arrays
    return build_arrays(list(reads), list(genomes), term)


def _merge(ctx, reads, genomes, term=0, cap=0, index_cap=0):
    gi = ctx.build_genome_index(genomes, term, index_cap)
    try:
        assert gi.info() == {"n_docs": len(genomes), "n_text": sum(len(g) for g in genomes), "lcp_cap": index_cap, "term": term,
                             "positions": sum(len(g) + 1 for g in genomes)}
        return ctx.merge_index(reads, gi, cap)
    finally:
        gi.close()


def _check(ctx, reads, genomes, term=0, cap=0, index_cap=0, what=""):
    want = IC.capped(_want(tuple(reads), tuple(genomes), term), cap)
    _same(_merge(ctx, reads, genomes, term, cap, index_cap), want, what)


def test_ties(ctx):
    _check(ctx, *MC.TIES, what="ties")
    info = ctx.merge_info()
    assert info["read_suffixes"] == sum(len(r) + 1 for r in MC.TIES[0])
    assert info["read_runs"] == MC.model_merge(*MC.TIES)[1]["runs"]
    _check(ctx, *MC.TIES, term=ord("$"), cap=3, what="ties, term $, cap 3")


def test_one_symbol(ctx):
    _check(ctx, *MC.ONE_SYMBOL, what="one symbol")
    for cap in (1, 8, 9):
        _check(ctx, *MC.ONE_SYMBOL, cap=cap, what=f"one symbol, cap {cap}")


@pytest.mark.parametrize("name", ["as_it_is", "swapped"])
def test_word_compares(ctx, name):
    reads, genomes = MC.word_collections()[name]
    _check(ctx, reads, genomes, what=name)
    for cap in (7, 8, 9, 16):
        _check(ctx, reads, genomes, cap=cap, what=f"{name}, cap {cap}")


@pytest.mark.parametrize("term", [0x00, 0xFF])
def test_bytes_00_and_ff_as_symbols(ctx, term):
    reads, genomes = MC.extreme_bytes()
    _check(ctx, reads, genomes, term=term, what=f"term {term}")


@pytest.mark.parametrize("name", sorted(MC.degenerate()))
def test_degenerate_sides(ctx, name):
    reads, genomes = MC.degenerate()[name]
    _check(ctx, reads, genomes, what=name)
    _check(ctx, reads, genomes, term=7, cap=2, what=name + ", term 7, cap 2")


@pytest.mark.parametrize("first", MC.RUN_FIRSTS)
def test_runs(ctx, first):
    reads, genomes = MC.runs_collection(first)
    _check(ctx, reads, genomes, what=f"run from {first}")
    assert ctx.merge_info()["read_runs"] == MC.model_merge(reads, genomes)[1]["runs"]


def _carved(data, shift, fill):
    """`data` (a uint8 tensor) as a view `shift` bytes into a 16-byte aligned buffer whose other bytes are `fill`"""
    import torch
    n = len(data)
    raw = torch.full((32 + shift + n + 48,), fill, dtype=torch.uint8, device="cuda")
    buf = raw[16 + (-raw.data_ptr()) % 16:]
    view = buf[shift:shift + n]
    view.copy_(data)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == shift
    return view, raw


def test_views_into_larger_buffers(ctx):
    import torch
    reads, genomes = MC.views_collection()
    want = _want(tuple(reads), tuple(genomes), 0)
    (rt, ro), (gt, go) = MC.pack(reads), MC.pack(genomes)
    rt_t, gt_t = torch.from_numpy(rt).cuda(), torch.from_numpy(gt).cuda()
    ro_t, go_t = torch.from_numpy(ro.astype(np.int64)).cuda(), torch.from_numpy(go.astype(np.int64)).cuda()
    for shift in range(16):
        for fill in (0x00, 0xFF):
            rv, keep_r = _carved(rt_t, shift, fill)
            gv, keep_g = _carved(gt_t, shift, fill)
            gi = ctx.build_genome_index_dev(gv, go_t, len(genomes), int(go[-1]))
            got = ctx.merge_index_dev(rv, ro_t, len(reads), int(ro[-1]), gi)
            _same(_host(got), want, f"shift {shift}, fill {fill:#x}")
            gi.close()
            assert bool((keep_r[:16] == fill).all()) and bool((keep_r[-16:] == fill).all())
    # only some of the outputs
    gi = ctx.build_genome_index(genomes)
    n = len(want[0])
    only = ctx.merge_index_dev(rt_t, ro_t, len(reads), int(ro[-1]), gi, out=(None, torch.empty(n, dtype=torch.int32, device="cuda"), None))
    assert only[0] is None and only[2] is None and np.array_equal(only[1].cpu().numpy().view(np.uint32), want[1])
    only = ctx.merge_index_dev(rt_t, ro_t, len(reads), int(ro[-1]), gi, out=(torch.empty(n, dtype=torch.uint8, device="cuda"), None, None))
    assert np.array_equal(only[0].cpu().numpy(), want[0])
    gi.close()


def test_caps(ctx):
    from lime_amd import _lib, api
    reads, genomes = MC.caps_collection()
    for cap in (0, 1, 15, 16, 17, 1000):
        _check(ctx, reads, genomes, cap=cap, what=f"uncapped index, cap {cap}")
    for cap in (16, 5):
        _check(ctx, reads, genomes, cap=cap, index_cap=16, what=f"index cap 16, cap {cap}")
    # what an index built with cap 16 cannot serve: refused before anything is written
    gi = ctx.build_genome_index(genomes, 0, 16)
    text, off = MC.pack(reads)
    n = int(ctx.lib.lime_merge_size(gi.h, off.ctypes.data, len(reads)))
    assert n == sum(len(d) + 1 for d in reads + genomes)
    for cap in (17, 0):
        e, l, d = np.full(n, 0xEE, np.uint8), np.full(n, 0xEEEEEEEE, np.uint32), np.full(n, 0xDDDDDDDD, np.uint32)
        rc = ctx.lib.lime_merge_index(ctx.h, text.ctypes.data, off.ctypes.data, len(reads), gi.h, cap, e.ctypes.data, l.ctypes.data, d.ctypes.data)
        msg = ctx.lib.lime_last_error().decode()
        assert rc == _lib.ERR_ARG and str(cap) in msg and "16" in msg, (rc, msg)
        assert (e == 0xEE).all() and (l == 0xEEEEEEEE).all() and (d == 0xDDDDDDDD).all()
        with pytest.raises(api.LimeError):
            ctx.merge_index(reads, gi, cap)
    gi.close()


def test_seeded_fuzz(ctx):
    from lime_amd.builder import build_arrays_sa
    compared = 0
    for case in range(IC.FUZZ_CASES):
        reads, genomes, term, cap, desc = IC.fuzz_collection(MC.SEED, case)
        want = IC.capped(build_arrays_sa(reads, genomes, term), cap)
        diff = IC.first_difference(_merge(ctx, reads, genomes, term, cap), want)
        assert diff is None, f"fuzz_collection({MC.SEED}, {case}) [{desc}]: {diff}"
        compared += 1
    assert compared == IC.FUZZ_CASES == 200


@pytest.mark.parametrize("big_side", ["reads", "genomes"])
def test_past_every_grid_stride_cap(ctx, big_side):
    """The launchers of lime_merge_kernel.hip cap their grids at MRG_RANK_BLOCKS = MRG_ENDS_BLOCKS = MRG_WRITE_BLOCKS = 8192 workgroups of
    256 threads = 2 097 152 threads; whoever changes those changes these.  index_cases.closed_form_documents(130 001, 16): 130 000
    documents 'A' * 16 and one 'A' * 15 + 'C'.
      reads:    the 130 000 documents are the reads, 2 210 000 read positions > 2 097 152: k_mrg_rank, k_mrg_ends and k_mrg_write_reads
                go round their stride loops; the one genome has 17 positions
      genomes:  the roles reversed, the one document is the read and the 130 000 are the genomes, 2 210 000 genome positions:
                k_mrg_write_genomes goes round its loop (and the running maximum runs over 2 210 001 words)
    Compared on the device with lime_build_index_dev on the concatenation, which tests/test_index_edges_gpu.py holds against the closed form."""
    import torch
    many, one = IC.closed_form_documents(130_001, 16)
    reads, genomes = (many, one) if big_side == "reads" else (one, many)
    assert sum(len(d) + 1 for d in many) == 2_210_000 > 8192 * 256
    (rt, ro), (gt, go) = MC.pack(reads), MC.pack(genomes)
    rt_t, gt_t = torch.from_numpy(rt).cuda(), torch.from_numpy(gt).cuda()
    ro_t, go_t = torch.from_numpy(ro.astype(np.int64)).cuda(), torch.from_numpy(go.astype(np.int64)).cuda()
    gi = ctx.build_genome_index_dev(gt_t, go_t, len(genomes), int(go[-1]))
    got = ctx.merge_index_dev(rt_t, ro_t, len(reads), int(ro[-1]), gi)
    gi.close()
    all_t = torch.cat([rt_t[:int(ro[-1])], gt_t[:int(go[-1])]])
    off_t = torch.cat([ro_t, go_t[1:] + int(ro[-1])])
    want = ctx.build_index_dev(all_t, off_t, len(reads) + len(genomes), int(ro[-1]) + int(go[-1]))
    for name, g, w in zip(("ebwt", "lcp", "da"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if not torch.equal(g, w):
            bad = torch.nonzero(g != w).reshape(-1)
            raise AssertionError(f"{name} differs at {len(bad)} of {len(w)} rows, first {bad[:5].tolist()}: got {g[bad[:5]].tolist()}, want {w[bad[:5]].tolist()}")


@functools.lru_cache(maxsize=None)
def _sampled():
    from tests.test_index_gpu import _sampled_collection
    return _sampled_collection(np.random.default_rng(79), 12_000, 4, 300)          # 7.8 * 10^4 symbols, a genome pair 1 % apart


def test_side_stream(ctx):
    import torch
    from lime_amd.builder import build_arrays_sa
    reads, genomes = _sampled()
    (rt, ro), (gt, go) = MC.pack(reads), MC.pack(genomes)
    rt_t = torch.from_numpy(rt).cuda()
    ro_t = torch.from_numpy(ro.astype(np.int64)).cuda()
    gi = ctx.build_genome_index(genomes, 0, 0)
    n_reads, n_text = len(reads), int(ro[-1])
    want = ctx.merge_index_dev(rt_t, ro_t, n_reads, n_text, gi, lcp_cap=40)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    text_s = torch.zeros(n_text, dtype=torch.uint8, device="cuda")           # not the reads yet
    filler = torch.rand(16_000_000, device="cuda")
    busy = torch.rand(16_000_000, device="cuda")
    torch.cuda.synchronize()
    # Best effort, as in tests/test_index_edges_gpu.py::test_side_stream: sorts stand in front of the write of the reads on the side stream, so
    # a merge that ignored `stream` would read zeros; the null stream is kept busy with sorts of its own meanwhile.
    for _ in range(3):
        busy = torch.sort(busy.flip(0))[0]
    with torch.cuda.stream(s):
        for _ in range(6):
            filler = torch.sort(filler.flip(0))[0]
        text_s.copy_(rt_t.flip(0).flip(0))
        got = ctx.merge_index_dev(text_s, ro_t, n_reads, n_text, gi, lcp_cap=40, stream=s.cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()
    gi.close()
    for name, g, w in zip(("ebwt", "lcp", "da"), got, want):
        assert torch.equal(g, w), name
    _same(_host(got), IC.capped(build_arrays_sa(reads, genomes, 0), 40), "side stream")


def _free_bytes():
    import torch
    from lime_amd import api
    torch.cuda.synchronize()
    api.trim_cache()
    return torch.cuda.mem_get_info()[0]


def test_save_load_in_a_fresh_context(ctx, tmp_path):
    import torch
    from lime_amd import _lib, api
    rng = np.random.default_rng([MC.SEED, 12])
    acgt = lambda n: bytes(IC.ACGTN[rng.integers(0, 4, size=int(n))].tobytes())
    genomes = [acgt(1_500_000), acgt(500_000), b"", acgt(77)]                # 28 MB of index: what it holds shows in the device's free memory
    reads = [genomes[0][o:o + 100] for o in range(0, 900_000, 9_001)] + [genomes[1][-50:], b"", acgt(60)]
    path = str(tmp_path / "genomes.gidx")
    gi = ctx.build_genome_index(genomes, ord("#"), 64)
    gi.save(path)
    assert sorted(os.listdir(tmp_path)) == ["genomes.gidx"]                  # the temporary name is gone
    info = gi.info()
    assert api.gindex_probe(path) == {k: info[k] for k in ("n_docs", "n_text", "lcp_cap", "term")}
    body = 16 * sum((b + 15) // 16 for b in (5 * 8, info["positions"] * 4, info["positions"] * 4, info["positions"] * 4, info["n_text"], info["positions"]))
    assert os.path.getsize(path) == 64 + body
    want = ctx.merge_index(reads, gi, 32)
    data = open(path, "rb").read()
    other = api.Context(0)
    try:
        # one whole cycle first, so that what the runtime allocates on a context's first launches is there before the free memory is read
        warm = other.build_genome_index(MC.TIES[1])
        other.merge_index(MC.TIES[0], warm)
        warm.close()
        before = _free_bytes()
        # refused files: nothing stays allocated
        bad = {"truncated": (data[:-1], _lib.ERR_IO), "header only": (data[:64], _lib.ERR_IO), "short header": (data[:40], _lib.ERR_IO),
               "magic": (b"XGIL" + data[4:], _lib.ERR_ARG), "version": (data[:4] + b"\x02\x00" + data[6:], _lib.ERR_ARG),
               "sa size": (data[:32] + np.array([info["positions"] * 4 + 4], "<u8").tobytes() + data[40:], _lib.ERR_ARG),
               "n_text": (data[:16] + np.array([info["n_text"] - 1], "<u8").tobytes() + data[24:], _lib.ERR_ARG),
               "too long": (data + b"\0" * 16, _lib.ERR_ARG),
               "doc_off decreases": (data[:64 + 8] + np.array([2_100_000], "<u8").tobytes() + data[64 + 16:], _lib.ERR_ARG),
               "doc_off start": (data[:64] + np.array([1], "<u8").tobytes() + data[64 + 8:], _lib.ERR_ARG),
               "doc_off end": (data[:64 + 32] + np.array([info["n_text"] - 1], "<u8").tobytes() + data[64 + 40:], _lib.ERR_ARG)}
        for name, (blob, code) in bad.items():
            p = str(tmp_path / "bad.gidx")
            open(p, "wb").write(blob)
            with pytest.raises(api.LimeError) as e:
                other.load_genome_index(p)
            assert e.value.code == code, (name, e.value)
        with pytest.raises(api.LimeError) as e:
            other.load_genome_index(str(tmp_path / "no_such_file"))
        assert e.value.code == _lib.ERR_IO
        assert _free_bytes() == before
        g2 = other.load_genome_index(path)
        assert g2.info() == info
        assert before - _free_bytes() >= body
        _same(other.merge_index(reads, g2, 32), want, "merge from the loaded index")
        p2 = str(tmp_path / "again.gidx")
        g2.save(p2)
        assert open(p2, "rb").read() == data
        g2.close()
        assert _free_bytes() == before
        # sa = 0xFFFFFFFF everywhere: every value is clamped before use -- wrong output, no fault
        small = [genomes[3], b"ACGTACGT", b""]
        gs = other.build_genome_index(small)
        ps = str(tmp_path / "small.gidx")
        gs.save(ps)
        gs.close()
        blob = bytearray(open(ps, "rb").read())
        n = sum(len(g) + 1 for g in small)
        sa_at = 64 + 32
        assert len(blob) == 64 + 32 + 3 * 16 * ((n * 4 + 15) // 16) + 16 * ((n - 3 + 15) // 16) + 16 * ((n + 15) // 16)
        blob[sa_at:sa_at + n * 4] = b"\xff" * (n * 4)
        open(ps, "wb").write(bytes(blob))
        gbad = other.load_genome_index(ps)
        out = other.merge_index(reads[-3:] + [b"ACGTACGTAC", b"TTTT", b"A"], gbad, 0)       # LIME_OK; the arrays are not compared
        assert len(out[0]) == n + sum(len(r) + 1 for r in reads[-3:]) + 11 + 5 + 2
        torch.cuda.synchronize()
        gbad.close()
        assert _free_bytes() == before
    finally:
        other.close()
    gi.close()
    _check(ctx, *MC.TIES, what="the first context after all that")


def test_outputs_feed_the_scan_directly(ctx):
    import torch
    from lime_amd import api
    reads, genomes = _sampled()
    n_reads, n_refs, alpha = len(reads), len(genomes), 16
    (rt, ro) = MC.pack(reads)
    text, off = api.pack_documents(reads, genomes)
    gi = ctx.build_genome_index(genomes)
    got = ctx.merge_index_dev(torch.from_numpy(rt).cuda(), torch.from_numpy(ro.astype(np.int64)).cuda(), n_reads, int(ro[-1]), gi)
    want = ctx.build_index_dev(torch.from_numpy(text).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), len(off) - 1, int(off[-1]))
    gi.close()
    n = int(off[-1]) + len(off) - 1
    assert all(t.data_ptr() % 16 == 0 and len(t) == n for t in got)
    tables = []
    for e, l, d in (got, want):
        sim = torch.zeros(api.sim_bytes(n_reads, n_refs), dtype=torch.uint8, device="cuda")
        ctx.fused_dev(l, d, e, n, n, True, n_reads, n_refs, alpha, sim)
        torch.cuda.synchronize()
        tables.append(sim)
    assert int((tables[1] != 0).sum()) > n_reads // 2                        # most reads score against some genome
    assert torch.equal(tables[0], tables[1])


def test_buildindex_two_step_forms(ctx, tmp_path):
    from lime_amd import api
    from lime_amd.builder import build_arrays_sa
    from tests.test_index_cpu import py_fasta
    exe = os.path.join(BIN, "BuildIndex")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    d = str(tmp_path)
    rd, rf = os.path.join(d, "reads.fasta"), os.path.join(d, "refs.fasta")
    open(rd, "wb").write(IC.REAL_WORLD_READS)
    open(rf, "wb").write(IC.REAL_WORLD_REFS)
    refs = py_fasta(IC.REAL_WORLD_REFS)
    run = lambda args: subprocess.run([exe] + args, capture_output=True, timeout=600, cwd=d)
    files = lambda base: tuple(open(base + ext, "rb").read() for ext in (".ebwt", ".lcp", ".da"))
    p = run(["--refs", rf, os.path.join(d, "g")])
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert b"numGenomes: 4\n" in p.stdout and b"numReads" not in p.stdout
    assert api.gindex_probe(os.path.join(d, "g.gidx")) == {"n_docs": 4, "n_text": sum(len(g) for g in refs), "lcp_cap": 0, "term": 0}
    p = run(["--refs", rf, os.path.join(d, "g20"), "--trlcp", "20"])
    assert p.returncode == 0 and api.gindex_probe(os.path.join(d, "g20.gidx"))["lcp_cap"] == 20
    for flags, gidx in (([], "g.gidx"), (["--rc"], "g.gidx"), (["--trlcp", "20"], "g.gidx"), (["--trlcp", "20"], "g20.gidx"), (["--rc", "--trlcp", "20"], "g20.gidx")):
        tag = "".join(flags) + gidx
        one, two = os.path.join(d, "one" + tag), os.path.join(d, "two" + tag)
        p1 = run([rd, rf, one] + flags)
        p2 = run([rd, "--gidx", os.path.join(d, gidx), two] + flags)
        assert p1.returncode == 0 and p2.returncode == 0, (p1.stderr.decode()[-1000:], p2.stderr.decode()[-1000:])
        assert p1.stdout == p2.stdout and b"numReads: 5\nnumGenomes: 4\n" in p2.stdout
        assert files(one) == files(two), tag
        # the one-step form's output is what it was: the oracle's
        reads = py_fasta(IC.REAL_WORLD_READS, rc="--rc" in flags)
        want = IC.capped(build_arrays_sa(reads, refs, 0), 20 if "--trlcp" in flags else 0)
        _same((np.fromfile(one + ".ebwt", np.uint8), np.fromfile(one + ".lcp", "<u4"), np.fromfile(one + ".da", "<u4")), want, "one step " + tag)
    # an index built with --trlcp 20 cannot serve the full lcp
    p = run([rd, "--gidx", os.path.join(d, "g20.gidx"), os.path.join(d, "no")])
    assert p.returncode == 1 and b"20" in p.stderr and not os.path.exists(os.path.join(d, "no.lcp"))
    # usage: the old text for a wrong argument count, in every form
    for args in ([rd, rf], [rd, rf, "a", "b"], ["--refs", rf], ["--refs", rf, "a", "b"], [rd, "--gidx", os.path.join(d, "g.gidx")], [rd, "--gidx"],
                 ["--refs", "--gidx", os.path.join(d, "g.gidx"), rf, "a"]):
        p = run(args)
        assert p.returncode == 1 and b"usage" in p.stderr and b"reads.fasta refs.fasta outBase [--rc] [--trlcp k]" in p.stderr, args
