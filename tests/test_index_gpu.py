"""ebwt / lcp / da from the sequences on the device (lime_build_index, lime_build_index_dev, bin/BuildIndex) against the Python builders
of lime_amd/builder.py, which define the contract.  Every comparison is np.array_equal on all three arrays: no tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
BIN = os.path.join(ROOT, "lime_amd", "bin")
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


def _rand(rng, n):
    return bytes(rng.choice(ACGT, size=int(n)).tobytes())


def _same(got, want, what):
    for name, g, w in zip(("ebwt", "lcp", "da"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{what}: {name} differs at {len(bad)} of {len(w)} positions, first {bad[:5]}: got {g[bad[:5]]}, want {w[bad[:5]]}")


def _small_cases():
    rng = np.random.default_rng(20260)
    rep = _rand(rng, 60)
    cases = {}
    g1 = _rand(rng, 500) + rep + _rand(rng, 300) + rep + rep + _rand(rng, 200)
    g2 = _rand(rng, 300) + rep + _rand(rng, 400)
    cases["planted_repeats"] = ([g1[i:i + 50] for i in rng.integers(0, len(g1) - 50, size=12)] + [rep[:40], rep[10:]], [g1, g2])
    d = _rand(rng, 300)
    cases["identical_documents"] = ([d, d, d[:100], d[:100]], [d, d])
    cases["prefixes_and_suffixes"] = ([d[:10], d[:50], d[:200], d[100:], d[250:], d[299:]], [d, d[:150], d[150:]])
    cases["empty_and_one_symbol"] = ([b"", b"A", b"", b"C", b"A", b""], [b"", b"T", _rand(rng, 40), b""])
    cases["single_document"] = ([], [_rand(rng, 700)])
    cases["single_empty_document"] = ([b""], [])
    cases["runs_of_one_symbol"] = ([b"A" * 2000], [b"A" * 1999])
    allb = bytes(range(256))
    cases["all_byte_values"] = ([allb, allb[::-1], bytes(rng.integers(0, 256, size=400, dtype=np.uint8))], [allb * 2, bytes([255]) * 30, bytes([0]) * 30])
    cases["no_reads"] = ([], [_rand(rng, 400), _rand(rng, 300)])
    cases["no_refs"] = ([_rand(rng, 80) for _ in range(10)], [])
    cases["two_symbols_long_repeats"] = ([b"AC" * 300, b"CA" * 299], [b"AC" * 301 + b"G" + b"AC" * 200])
    return cases


SMALL = _small_cases()


@pytest.mark.parametrize("term", [0, ord("$")])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_matches_naive_builder(ctx, name, term):
    from lime_amd.builder import build_arrays
    reads, genomes = SMALL[name]
    assert sum(len(d) + 1 for d in reads + genomes) <= 4100
    want = build_arrays(reads, genomes, term)
    _same(ctx.build_index(reads, genomes, term), want, name)
    for cap in (1, 7):
        got = ctx.build_index(reads, genomes, term, cap)
        _same(got, (want[0], np.minimum(want[1], cap).astype(np.uint32), want[2]), f"{name} cap {cap}")


def _sampled_collection(rng, genome_len, n_genomes, n_reads, read_len=100, twin_rate=0.01):
    """random genomes, the last one a copy of the first with twin_rate of its positions substituted; reads sampled from them with ~1 % substitutions"""
    genomes = [bytearray(_rand(rng, genome_len)) for _ in range(n_genomes - 1)]
    twin = bytearray(genomes[0])
    for p in np.nonzero(rng.random(genome_len) < twin_rate)[0]:
        twin[p] = b"ACGT"[(b"ACGT".index(twin[p]) + 1 + int(rng.integers(0, 3))) % 4]
    genomes = [bytes(g) for g in genomes] + [bytes(twin)]
    reads = []
    for _ in range(n_reads):
        g = genomes[int(rng.integers(0, n_genomes))]
        s = int(rng.integers(0, genome_len - read_len))
        r = bytearray(g[s:s + read_len])
        for p in np.nonzero(rng.random(read_len) < 0.01)[0]:
            r[p] = b"ACGT"[int(rng.integers(0, 4))]
        reads.append(bytes(r))
    return reads, genomes


@pytest.fixture(scope="module")
def mid():
    from lime_amd.builder import build_arrays_sa
    reads, genomes = _sampled_collection(np.random.default_rng(77), 40_000, 4, 1500)        # 3.1 * 10^5 symbols
    return reads, genomes, build_arrays_sa(reads, genomes, 0)


def test_matches_prefix_doubling_builder_with_caps(ctx, mid):
    reads, genomes, want = mid
    assert int(want[1].max()) > 300                                      # the genome pair: long common stretches, several doubling rounds
    _same(ctx.build_index(reads, genomes, 0), want, "sampled reads")
    info = ctx.index_info()
    assert info["rounds"] >= 3 and info["unresolved"][0] > info["unresolved"][1] > 0
    for cap in (16, 33):
        _same(ctx.build_index(reads, genomes, 0, cap), (want[0], np.minimum(want[1], cap).astype(np.uint32), want[2]), f"cap {cap}")


def test_device_outputs_feed_the_scan_directly(ctx, mid):
    import torch
    from lime_amd import api
    reads, genomes, want = mid
    n_reads, n_refs, alpha, norm, beta = len(reads), len(genomes), 16, 85, 0.25
    text, off = api.pack_documents(reads, genomes)
    text_t = torch.from_numpy(text).cuda()
    off_t = torch.from_numpy(off.astype(np.int64)).cuda()
    ebwt_t, lcp_t, da_t = ctx.build_index_dev(text_t, off_t, len(off) - 1, int(off[-1]))
    n = len(want[0])
    assert all(t.data_ptr() % 16 == 0 for t in (ebwt_t, lcp_t, da_t)) and len(ebwt_t) == len(lcp_t) == len(da_t) == n
    got_lists, _ = ctx.fused_choose_lists_dev(lcp_t, da_t, ebwt_t, n, n_reads, n_refs, alpha, norm, beta)
    e, l, d = (torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else np.uint8)).cuda() for a in want)
    want_lists, _ = ctx.fused_choose_lists_dev(l, d, e, n, n_reads, n_refs, alpha, norm, beta)
    g, w = got_lists.get(), want_lists.get()
    assert int(w[1][-1]) > n_reads // 2                                  # most reads have a list
    for a, b in zip(g, w):
        assert np.array_equal(a, b)
    _same((ebwt_t.cpu().numpy(), lcp_t.cpu().numpy().view(np.uint32), da_t.cpu().numpy().view(np.uint32)), want, "device arrays")
    # only some of the outputs
    only = ctx.build_index_dev(text_t, off_t, len(off) - 1, int(off[-1]), out=(None, torch.empty(n, dtype=torch.int32, device="cuda"), None))
    assert only[0] is None and only[2] is None and np.array_equal(only[1].cpu().numpy().view(np.uint32), want[1])
    got_lists.close(); want_lists.close()


def test_example_collections_and_programs(ctx, tmp_path):
    import make_golden_example as G
    from lime_amd import api
    from lime_amd.builder import build_arrays_sa
    for exe in ("BuildIndex", "LiME_paired"):
        if not os.path.exists(os.path.join(BIN, exe)):
            subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1800)
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_full.npz"))
    genomes, sets = G.collections(z["reads_1"], z["reads_2"], z["src"])
    n_reads, d = len(z["reads_1"]), str(tmp_path)

    def fasta(path, seqs):
        with open(path, "wb") as f:
            for i, s in enumerate(seqs):
                f.write(b">s%d\n" % i)
                for o in range(0, len(s), 70):
                    f.write(s[o:o + 70] + b"\n")

    refs = os.path.join(d, "refs.fasta")
    fasta(refs, genomes)
    bases = []
    for name, src, flag in (("F1", "F1", []), ("F1RC", "F1", ["--rc"]), ("F2", "F2", []), ("F2RC", "F2", ["--rc"])):
        want = build_arrays_sa(sets[name], genomes, term=0)
        _same(api.build_index(sets[name], genomes, ctx=ctx), want, name)
        rd = os.path.join(d, f"reads_{src}.fasta")
        fasta(rd, sets[src])
        base = os.path.join(d, f"{name}.fasta")
        p = subprocess.run([os.path.join(BIN, "BuildIndex"), rd, refs, base] + flag, capture_output=True, timeout=600, cwd=d)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        assert f"numReads: {n_reads}\nnumGenomes: {len(genomes)}\n".encode() in p.stdout
        _same((np.fromfile(base + ".ebwt", np.uint8), np.fromfile(base + ".lcp", "<u4"), np.fromfile(base + ".da", "<u4")), want, name + " files")
        bases.append(base)
    tax = os.path.join(d, "LineageFile.csv")
    open(tax, "wb").write(bytes(z["lineage"]))
    out = os.path.join(d, "classification.txt")
    p = subprocess.run([os.path.join(BIN, "LiME_paired")] + bases + [out, str(n_reads), str(len(genomes)), tax, str(G.READ_LEN), "4"],
                       capture_output=True, timeout=600, cwd=d)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert open(out, "rb").read() == bytes(z["classification"])
    # --trlcp at or above alpha changes nothing downstream
    p = subprocess.run([os.path.join(BIN, "BuildIndex"), os.path.join(d, "reads_F1.fasta"), refs, os.path.join(d, "capped"), "--trlcp", "32"],
                       capture_output=True, timeout=600, cwd=d)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert np.array_equal(np.fromfile(os.path.join(d, "capped.lcp"), "<u4"), np.minimum(np.fromfile(bases[0] + ".lcp", "<u4"), 32))


def test_two_hundred_million_symbols_on_the_device(ctx):
    """Past what the Python builders can check.  Checked in full on the device: da holds every document len + 1 times; the LF mapping that
    ebwt and da define, followed from every row to its document's start (pointer jumping), gives every row a position, and the positions
    are a permutation of the collection.  Checked on a SAMPLE (4000 rows, stated as such): suffix i - 1 < suffix i and lcp[i] by direct
    comparison of the text on the host."""
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(9)
    n_gen, gen_len, n_reads, read_len = 10, 5_000_000, 1_500_000, 100
    sym = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    genomes = sym[torch.randint(0, 4, (n_gen, gen_len), device="cuda", generator=g)]
    src = torch.randint(0, n_gen, (n_reads,), device="cuda", generator=g)
    start = torch.randint(0, gen_len - read_len, (n_reads,), device="cuda", generator=g)
    reads = genomes.reshape(-1)[(src * gen_len + start)[:, None] + torch.arange(read_len, device="cuda")[None, :]]
    subst = torch.rand(reads.shape, device="cuda", generator=g) < 0.01
    reads = torch.where(subst, sym[torch.randint(0, 4, reads.shape, device="cuda", generator=g)], reads)
    text_t = torch.cat([reads.reshape(-1), genomes.reshape(-1)]).contiguous()
    lens = torch.cat([torch.full((n_reads,), read_len, dtype=torch.int64), torch.full((n_gen,), gen_len, dtype=torch.int64)])
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    n_docs, n_text = n_reads + n_gen, int(off[-1])
    assert n_text == 200_000_000
    del reads, subst, genomes, src, start
    ebwt_t, lcp_t, da_t = ctx.build_index_dev(text_t, off.cuda(), n_docs, n_text)
    n = n_text + n_docs
    da64 = da_t.to(torch.int64)
    assert int(da64.min()) >= 0 and int(da64.max()) == n_docs - 1
    assert torch.equal(torch.bincount(da64, minlength=n_docs).cpu(), lens + 1)
    assert int(lcp_t[0]) == 0
    # LF: the row of the suffix one symbol to the left (rows whose ebwt is the terminator byte 0 are their document's whole suffix)
    nxt = torch.arange(n, device="cuda")
    base = n_docs
    for c in b"ACGT":
        mask = ebwt_t == c
        cnt = int(mask.sum())
        assert cnt == int((text_t == c).sum())
        nxt[mask] = base + torch.arange(cnt, device="cuda")
        base += cnt
        del mask
    assert base == n and int((ebwt_t == 0).sum()) == n_docs
    dist = (nxt != torch.arange(n, device="cuda")).to(torch.int64)
    for _ in range(24):                                                  # 2^24 > the longest document
        dist = dist + dist[nxt]
        nxt = nxt[nxt]
    assert int((ebwt_t[nxt] != 0).sum()) == 0                            # every chain ended at a whole-document suffix
    pos = off.cuda()[da64] + da64 + dist                                 # the suffix's position in the terminated collection
    assert int(dist.max()) == gen_len and torch.equal(torch.sort(pos)[0], torch.arange(n, device="cuda"))
    # the sample
    rows = torch.randint(1, n, (4000,), generator=torch.Generator().manual_seed(3))
    rows = torch.cat([rows, torch.arange(1, 40), torch.arange(n_docs - 20, n_docs + 20), torch.arange(n - 40, n)]).cuda()
    h = lambda t: t.cpu().numpy()
    k1, o1, k0, o0, lc = h(da64[rows]), h(dist[rows]), h(da64[rows - 1]), h(dist[rows - 1]), h(lcp_t[rows])
    text, offh = h(text_t), off.numpy()
    big = 0
    for i in range(len(rows)):
        a = text[offh[k0[i]] + o0[i]:offh[k0[i] + 1]]
        b = text[offh[k1[i]] + o1[i]:offh[k1[i] + 1]]
        m = min(len(a), len(b))
        neq = np.nonzero(a[:m] != b[:m])[0]
        l = int(neq[0]) if len(neq) else m
        assert int(lc[i]) == l, (i, int(rows[i]), int(lc[i]), l)
        if l < m:
            assert a[l] < b[l]
        elif len(a) == len(b):
            assert k0[i] < k1[i]
        else:
            assert len(a) == l
        big += l >= 16
    assert big > 1000
    info = ctx.index_info()
    assert 1 <= info["rounds"] <= 8 and info["unresolved"][0] > info["unresolved"][1]


def test_limits_and_bad_offsets_are_argument_errors(ctx):
    import torch
    from lime_amd import _lib
    lib = ctx.lib
    text = np.frombuffer(b"ACGTACGT", np.uint8)
    out = np.zeros(64, np.uint32)

    def host(off, n_docs):
        off = np.array(off, dtype=np.uint64)
        return lib.lime_build_index(ctx.h, text.ctypes.data, off.ctypes.data, n_docs, 0, 0, None, out.ctypes.data, None)

    assert host([0, 1 << 32], 1) == _lib.ERR_ARG and b"2^32 - 1" in lib.lime_last_error()
    assert host([0, (1 << 32) - 1], 1) == _lib.ERR_ARG                   # + 1 terminator
    assert host([1, 8], 1) == _lib.ERR_ARG
    assert host([0, 6, 4, 8], 3) == _lib.ERR_ARG and b"decreases" in lib.lime_last_error()
    assert lib.lime_build_index(ctx.h, None, np.array([0, 4], np.uint64).ctypes.data, 1, 0, 0, None, out.ctypes.data, None) == _lib.ERR_ARG
    text_t = torch.from_numpy(text.copy()).cuda()
    dev = lambda off, n_docs, n_text: lib.lime_build_index_dev(ctx.h, text_t.data_ptr(), torch.tensor(off, dtype=torch.int64).cuda().data_ptr(),
                                                               n_docs, n_text, 0, 0, None, None, None, None)
    assert dev([0, 8], 1, (1 << 32) - 1) == _lib.ERR_ARG
    assert dev([0, 6], 1, 8) == _lib.ERR_ARG and b"doc_off" in lib.lime_last_error()      # does not end at n_text
    assert dev([0, 6, 4, 8], 3, 8) == _lib.ERR_ARG
    assert dev([2, 8], 1, 8) == _lib.ERR_ARG
    assert dev([0, 8], 1, 8) == 0
    assert host([0], 0) == 0                                             # an empty collection: nothing to do


def test_the_context_still_passes_a_fused_golden_after_builds(ctx):
    from oracle import oracle_py as O
    n, nr, ng = 300_000, 2_000, 60
    lcp, da, eb = O.synth(7, 0, n, nr, ng, 16, 1)
    cl, nc, ml = O.detect(lcp, da, nr, 16)
    exp = O.score(da, eb, cl, nr, ng, threads=4)
    ctx.build_index([b"ACGT" * 50] * 20, [b"ACGT" * 500])
    sim, gnc, gml = ctx.fused(lcp, da, eb, nr, ng, 16)
    assert (gnc, gml) == (nc, ml) and np.array_equal(sim, exp)
