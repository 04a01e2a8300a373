"""The index builder (lime_build_index, lime_build_index_dev, bin/BuildIndex) where tests/test_index_gpu.py does not reach: every packing
width with documents at the lengths the rounds end at, k_idx_lcp's word compares and caps, a text that is not 16-byte aligned, the
grid-stride loops past their caps, a side stream, FASTA as it comes, and a seeded fuzz.  The collections and references are those of
tests/index_cases.py (checked without a GPU in tests/test_index_cases_cpu.py); every comparison is np.array_equal / torch.equal on all
three arrays: no tolerance anywhere."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import index_cases as IC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "lime_amd", "bin")
SEED = 20261


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
    """build_index_dev's tensors as build_index's numpy arrays"""
    e, l, d = tensors
    return e.cpu().numpy(), l.cpu().numpy().view(np.uint32), d.cpu().numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def _boundary_docs(sigma):
    return IC.boundary_collection(sigma, SEED)


@functools.lru_cache(maxsize=None)
def _boundary(sigma, term_in_text):
    from lime_amd.builder import build_arrays
    reads, genomes = _boundary_docs(sigma)
    term = max(reads[-1]) if term_in_text else 0                       # reads[-1] holds every byte of the alphabet
    return reads, genomes, term, build_arrays(reads, genomes, term)


@pytest.mark.parametrize("term_in_text", [False, True], ids=["term0", "term_in_text"])
@pytest.mark.parametrize("sigma", IC.SIGMAS)
def test_every_packing_width(ctx, sigma, term_in_text):
    reads, genomes, term, want = _boundary(sigma, term_in_text)
    k = IC.width_of(sigma)[1]
    _same(ctx.build_index(reads, genomes, term), want, f"sigma {sigma}")
    # The twins s[:4k] agree on 4k symbols and differ only in their terminators.  The first sort looks at k symbols, doubling round r at
    # k * 2^r: before round 2 nothing has seen all 4k of them, so they cannot have separated earlier.
    info = ctx.index_info()
    assert info["rounds"] >= 2
    # what the first sort leaves in groups says how many symbols it packed: the count for k_syms, stated independently
    assert info["unresolved"][0] == IC.tied_after(reads, genomes, k), (sigma, k, info)
    for cap in (k - 1, k, k + 1):
        _same(ctx.build_index(reads, genomes, term, cap), IC.capped(want, cap), f"sigma {sigma} cap {cap}")


def test_lcp_word_path_and_caps(ctx):
    from lime_amd.builder import build_arrays
    reads, genomes = IC.lcp_word_collection(SEED)
    want = build_arrays(reads, genomes, 0)
    for cap in (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25):
        _same(ctx.build_index(reads, genomes, 0, cap), IC.capped(want, cap), f"cap {cap}")


def _three_value_collection():
    """about 3000 symbols over three byte values (bits = 2, k_syms = 32) with repeats of 24 .. 30 symbols, which 32 symbols tell apart and
    the 21 or 16 of a wider alphabet do not, and one of 40, so that a doubling round runs in any case; the last document is long"""
    rng = np.random.default_rng([SEED, 3])
    abc = np.array([0x41, 0x9C, 0xF0], np.uint8)
    draw = lambda n: bytearray(abc[rng.integers(0, 3, size=int(n))].tobytes())
    docs = [draw(n) for n in (0, 1, 33, 64, 150, 31, 417, 32, 600, 255, 256, 257, 300, 0, 580)]
    for rep_len in (24, 26, 27, 29, 30, 40):
        rep = draw(rep_len)
        for d in rng.choice([4, 6, 8, 9, 12, 14], size=3, replace=False):
            o = int(rng.integers(0, len(docs[d]) - rep_len - 16))
            docs[d][o:o + rep_len] = rep
    docs = [bytes(d) for d in docs]
    return docs[:9], docs[9:]


def test_unaligned_text_base_and_end(ctx):
    import torch
    from lime_amd import api
    from lime_amd.builder import build_arrays_sa
    reads, genomes = _three_value_collection()
    assert set(b"".join(reads + genomes)) == {0x41, 0x9C, 0xF0} and len(genomes[-1]) > 32
    text, off = api.pack_documents(reads, genomes)
    n_docs, n_full = len(off) - 1, int(off[-1])
    assert 2900 <= n_full <= 3100
    other = torch.tensor([0x00, 0x42, 0x9D, 0xEF, 0xFF], dtype=torch.uint8, device="cuda")

    def build(shift, drop, out=None):
        """the collection without the last `drop` symbols of its last document: (aligned build, build on a view `shift` bytes into a 16-byte
        aligned buffer whose other bytes hold five other values) -> (arrays, info) of each"""
        n_text = n_full - drop
        o = off.astype(np.int64); o[-1] = n_text
        off_t = torch.from_numpy(o).cuda()
        body = torch.from_numpy(text[:n_text].copy()).cuda()
        raw = other[torch.arange(16 + shift + n_text + 48, device="cuda") % 5]
        buf = raw[16 + (-raw.data_ptr()) % 16:]                           # 16 bytes of the other values in front, whatever the shift
        assert buf.data_ptr() % 16 == 0
        view = buf[shift:shift + n_text]
        view.copy_(body)
        assert view.data_ptr() % 16 == shift and body.data_ptr() % 16 == 0
        res = []
        for t, o_ in ((body, None), (view, out)):
            got = ctx.build_index_dev(t, off_t, n_docs, n_text, out=o_)
            res.append((_host(got), ctx.index_info()))
        return res, n_text

    refs = {}
    def want_for(drop):
        if drop not in refs:
            refs[drop] = build_arrays_sa(reads, genomes[:-1] + [genomes[-1][:len(genomes[-1]) - drop]], 0)
        return refs[drop]

    for shift, drop in [(s, 0) for s in range(16)] + [(5, d) for d in range(1, 16)]:
        (aligned, info_a), (shifted, info_s) = build(shift, drop)[0]
        _same(aligned, want_for(drop), f"aligned, {drop} dropped")
        _same(shifted, want_for(drop), f"shift {shift}, {drop} dropped")
        # A byte of the padding that k_idx_present counted would change no output (the codes stay in order); it would raise sigma from 3
        # to 4 .. 8 and k_syms from 32 to 21 or 16, and then the repeats of 24 .. 30 symbols are still in groups after the first sort.
        # So the count of suffixes left in groups is compared with the one 32 symbols give, computed here, for both builds: that pins
        # k_idx_present's own mask (`c + k >= lo && c + k < hi`) at the text's base and at its end.  It does NOT see what
        # load16_within's fast path returns for bytes outside [lo, hi): both callers mask those bytes again.
        tied = IC.tied_after(reads, genomes[:-1] + [genomes[-1][:len(genomes[-1]) - drop]], 32)
        assert tied > 0 and info_a["rounds"] >= 1
        assert info_a["unresolved"][0] == tied and info_s["unresolved"][0] == tied, (shift, drop, tied, info_a, info_s)
        assert (info_s["rounds"], info_s["unresolved"]) == (info_a["rounds"], info_a["unresolved"]), (shift, drop, info_s, info_a)

    # outputs that are views at a 4-byte (not 16-byte) offset; what lies around them stays
    n = n_full + n_docs
    eb = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    lb = torch.full((n + 16,), -7, dtype=torch.int32, device="cuda")
    db = torch.full((n + 16,), -9, dtype=torch.int32, device="cuda")
    outs = (eb[4:4 + n], lb[1:1 + n], db[1:1 + n])
    assert all(t.data_ptr() % 16 == 4 for t in outs)
    res, _ = build(11, 0, out=outs)
    _same(res[1][0], want_for(0), "outputs at a 4-byte offset")
    _same(_host(outs), want_for(0), "outputs at a 4-byte offset, the tensors passed")
    assert bool((eb[:4] == 0xEE).all()) and bool((eb[4 + n:] == 0xEE).all())
    assert int(lb[0]) == -7 and bool((lb[1 + n:] == -7).all()) and int(db[0]) == -9 and bool((db[1 + n:] == -9).all())


def test_grid_stride_limits_closed_form(ctx):
    """The sizes follow the caps of the launches in lime_index_kernel.hip; whoever changes those changes these:
      idx_launch_check      k_idx_check      blocks_for(n_docs + 1, 4096) * 256 = 1 048 576 threads  < 2 200 001 offsets; the bad one is
                                                                                                       past two full trips of the stride
      idx_launch_check      k_idx_present    blocks_for(chunks, 8192) * 256     = 2 097 152 chunks of 16 bytes = 33 554 432 bytes
                                                                                                     < 35 200 000 of text, the only 'C' last
      idx_launch_doc_heads  k_idx_doc_heads  blocks_for(n_docs - 1, 8192) * 256 = 2 097 152 threads  < 2 199 999 document heads
    All documents are 'A' * 16 but the last, 'A' * 15 + 'C': every suffix reaches its terminator inside the first 32 symbols (two byte
    values: k_syms = 32), so no doubling round runs, and index_cases.closed_form_runs states the three arrays."""
    import torch
    from lime_amd import _lib, api
    n_docs, L = 2_200_000, 16
    n_text = n_docs * L
    assert n_docs - 1 > 8192 * 256 and (n_text + 15) // 16 > 8192 * 256 and n_docs + 1 > 2 * 4096 * 256
    text_t = torch.full((n_text,), ord("A"), dtype=torch.uint8, device="cuda")
    text_t[-1] = ord("C")
    off_t = torch.arange(n_docs + 1, dtype=torch.int64, device="cuda") * L
    got = ctx.build_index_dev(text_t, off_t, n_docs, n_text)
    assert ctx.index_info()["rounds"] == 0
    want = IC.closed_form_runs_torch(n_docs, L, 0, device="cuda")
    for name, g, w in zip(("ebwt", "lcp", "da"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if not torch.equal(g, w):
            bad = torch.nonzero(g != w).reshape(-1)
            raise AssertionError(f"{name} differs at {len(bad)} of {len(w)} rows, first {bad[:5].tolist()}: got {g[bad[:5]].tolist()}, want {w[bad[:5]].tolist()}")
    del got, want
    # an offset below its predecessor, at a document that only the stride loop's third trip reaches
    off_t[2_150_000] = off_t[2_149_999] - 1
    with pytest.raises(api.LimeError) as e:
        ctx.build_index_dev(text_t, off_t, n_docs, n_text)
    assert e.value.code == _lib.ERR_ARG and "doc_off" in str(e.value)
    del text_t, off_t
    torch.cuda.empty_cache()
    # the context is still good
    from lime_amd.builder import build_arrays
    reads, genomes = IC.closed_form_documents(7, L)
    small = ctx.build_index(reads, genomes, 0)
    _same(small, build_arrays(reads, genomes, 0), "a small build after the refused one")
    _same(small, IC.closed_form_runs(7, L, 0), "the closed form at the small size")


def test_side_stream(ctx):
    import torch
    from lime_amd import api
    from tests.test_index_gpu import _sampled_collection
    reads, genomes = _sampled_collection(np.random.default_rng(78), 12_000, 4, 300)          # 7.8 * 10^4 symbols, a genome pair 1 % apart
    text, off = api.pack_documents(reads, genomes)
    n_docs, n_text = len(off) - 1, int(off[-1])
    text_t = torch.from_numpy(text).cuda()
    off_t = torch.from_numpy(off.astype(np.int64)).cuda()
    want = ctx.build_index_dev(text_t, off_t, n_docs, n_text, lcp_cap=40)
    info = ctx.index_info()
    assert info["rounds"] >= 2
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != 0
    text_s = torch.zeros(n_text, dtype=torch.uint8, device="cuda")           # not the text yet
    filler = torch.rand(16_000_000, device="cuda")
    torch.cuda.synchronize()
    # Best effort: a builder that ignored `stream` shows only if the write of the text is still pending when it reads the text.  Six sorts
    # of 1.6 * 10^7 floats (tens of milliseconds of device work, queued in microseconds) stand in front of the write; torch's side streams do
    # not wait for the NULL stream nor it for them.  Were the queue already drained, the test would pass without having shown anything.
    with torch.cuda.stream(s):
        for _ in range(6):
            filler = torch.sort(filler.flip(0))[0]                            # work in front of the write, so that it is still pending at the call
        text_s.copy_(text_t.flip(0).flip(0))                                  # the text is written on the stream immediately before
        got = ctx.build_index_dev(text_s, off_t, n_docs, n_text, lcp_cap=40, stream=s.cuda_stream)
    s.synchronize()
    for name, g, w in zip(("ebwt", "lcp", "da"), got, want):
        assert torch.equal(g, w), name
    assert (ctx.index_info()["rounds"], ctx.index_info()["unresolved"]) == (info["rounds"], info["unresolved"])
    from lime_amd.builder import build_arrays_sa
    _same(_host(got), IC.capped(build_arrays_sa(reads, genomes, 0), 40), "side stream")


def test_buildindex_on_real_world_fasta(ctx, tmp_path):
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
    assert len(refs) == 4 and b"" in refs
    for flag in ([], ["--rc"]):
        reads = py_fasta(IC.REAL_WORLD_READS, rc=bool(flag))
        assert len(reads) == 5 and b"" in reads and len(set(b"".join(reads + refs))) > 16          # case, N and IUPAC kept: more than 4 bits a code
        want = build_arrays_sa(reads, refs, 0)
        base = os.path.join(d, "out" + "".join(flag))
        p = subprocess.run([exe, rd, rf, base] + flag, capture_output=True, timeout=600, cwd=d)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert b"numReads: 5\nnumGenomes: 4\n" in p.stdout
        _same((np.fromfile(base + ".ebwt", np.uint8), np.fromfile(base + ".lcp", "<u4"), np.fromfile(base + ".da", "<u4")), want, "files " + "".join(flag))
        _same(ctx.build_index(reads, refs, 0), want, "the same documents through the library " + "".join(flag))
    assert py_fasta(IC.REAL_WORLD_READS, rc=True)[4] == b"TGTAATCNNNNNTGTAATCtgtaatcTGTAATCTGTAATC"


def test_seeded_fuzz(ctx):
    from lime_amd.builder import build_arrays_sa
    compared = 0
    for case in range(IC.FUZZ_CASES):
        reads, genomes, term, cap, desc = IC.fuzz_collection(SEED, case)
        want = IC.capped(build_arrays_sa(reads, genomes, term), cap)
        got = ctx.build_index(reads, genomes, term, cap)
        diff = IC.first_difference(got, want)
        assert diff is None, f"fuzz_collection({SEED}, {case}) [{desc}]: {diff}"
        compared += 1
    assert compared == IC.FUZZ_CASES == 200
