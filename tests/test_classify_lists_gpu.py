"""Classify on the device (lime_classify_lists_dev) over clusterChoose lists left in HBM (lime_choose_lists_dev,
lime_fused_choose_lists_dev), and LiME_paired, the whole paired-end chain in one process:
  - the reference's own Classify output bytes of tests/golden/classify_*.npz for every BIN / HIGHER / rank key;
  - the example's full chain (tests/golden/example_full.npz) byte for byte;
  - at scale (10^8 symbols at configs[1]'s shape, and a collection the table-free path serves): device verdicts = lime_classify_mem on
    lime_lists_get's copies = lime_classify over .res.bin files written from lime_fused_choose_dev's output, including reads that
    take rule 3's every-genome path (beta 0);
  - the documented errors, none of which faults the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from test_classify_lists_cpu import CASES, KEYS, fixture_lists  # noqa: E402


def _ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    return api.Context(0)


def _upload_table(sim):
    import torch
    from lime_amd import api
    nr, ng = sim.shape
    t = torch.zeros(api.sim_bytes(nr, ng), dtype=torch.uint8, device="cuda")
    t[:nr * ng] = torch.from_numpy(np.ascontiguousarray(sim).reshape(-1)).cuda()
    return t


def test_device_classify_matches_reference_classify(tmp_path):
    from lime_amd import api
    ctx = _ctx()
    rules, types = set(), set()
    for case in CASES:
        g = np.load(case)
        norm, beta = int(g["norm"]), float(g["beta"])
        n_files, n_reads, n_targ = g["sims"].shape
        tax = str(tmp_path / "lineage.csv")
        open(tax, "wb").write(g["tax"].tobytes())
        tables = [_upload_table(s) for s in g["sims"]]
        lists = [ctx.choose_lists_dev(t, n_reads, n_targ, norm, beta) for t in tables]
        for li, want in zip(lists, fixture_lists(g)[0]):         # the lists themselves
            mx, off, pairs = li.get()
            assert np.array_equal(mx, want[0]) and np.array_equal(off, want[1]) and np.array_equal(pairs, want[2])
        for key in KEYS:
            if key not in g.files:
                continue
            binary, higher, rank = int(key[5]), int(key[8]), int(key[11:])
            tx = api.load_taxonomy(tax, rank, higher, n_targ)
            v, counts = ctx.classify_lists_dev(lists, n_targ, tx, binary)
            outp = str(tmp_path / f"{os.path.basename(case)}_{key}.txt")
            api.write_classification(outp, v)
            assert open(outp, "rb").read() == g[key].tobytes(), (case, key)
            assert [int((v["type"] == ord(t)).sum()) for t in "CUAH"] == counts
            rules |= set(int(x) for x in v["rule"])
            types |= set(chr(x) for x in v["type"])
            tx.close()
        for li in lists:
            li.close()
    ctx.close()
    assert {1, 2, 3} <= rules and set("CUAH") <= types, (rules, types)


def test_lime_paired_whole_chain_matches_reference(tmp_path):
    import make_golden_example as G
    from lime_amd.builder import build_arrays_sa
    exe = os.path.join(ROOT, "lime_amd", "bin", "LiME_paired")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1200)
    z = np.load(os.path.join(ROOT, "tests", "golden", "example_full.npz"))
    genomes, sets = G.collections(z["reads_1"], z["reads_2"], z["src"])
    n_reads, d = len(z["reads_1"]), str(tmp_path)
    bases = []
    for name in G.SETS:
        base = os.path.join(d, f"{name}.fasta")
        ebwt, lcp, da = build_arrays_sa(sets[name], genomes, term=0)
        lcp.astype("<u4").tofile(base + ".lcp"); da.astype("<u4").tofile(base + ".da"); ebwt.tofile(base + ".ebwt")
        bases.append(base)
    tax = os.path.join(d, "LineageFile.csv")
    open(tax, "wb").write(bytes(z["lineage"]))
    out = os.path.join(d, "classification.txt")
    before = set(os.listdir(d))
    p = subprocess.run([exe] + bases + [out, str(n_reads), str(len(genomes)), tax, str(G.READ_LEN), "4"], capture_output=True, timeout=600, cwd=d)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    assert open(out, "rb").read() == bytes(z["classification"])
    assert set(os.listdir(d)) - before == {"classification.txt"}          # no .clrs / .out / .res.* files
    assert b"Number of successfully classified reads" in p.stdout
    # the Python mirror does the same
    from lime_amd import api
    out2 = os.path.join(d, "classification_py.txt")
    counts = api.lime_paired(bases, out2, n_reads, len(genomes), tax, G.READ_LEN, 4)
    assert open(out2, "rb").read() == bytes(z["classification"]) and sum(counts) == n_reads


def _taxonomy_file(path, n_targ):
    import make_golden_classify as M
    open(path, "wb").write(M.taxonomy(n_targ, np.random.default_rng(11), True))
    return path


def _res_classify(lib, d, tag, host_lists, norm, beta, n_reads, n_targ, tax, rank, higher):
    """today's chain: .res.bin / .res.pos written from lime_fused_choose_dev's output, read back by lime_classify"""
    import ctypes as C
    bases = []
    for i, (mx, off, pairs) in enumerate(host_lists):
        b = os.path.join(d, f"{tag}_{i}.res")
        pr = np.ascontiguousarray(pairs, dtype=np.uint32)
        assert lib.lime_write_res_bin_pairs((b + ".bin").encode(), (b + ".pos").encode(), mx.ctypes.data, off.ctypes.data,
                                            pr.ctypes.data if len(pr) else None, n_reads, norm, C.c_float(beta)) == 0
        bases.append(b)
    arr = (C.c_char_p * len(bases))(*[b.encode() for b in bases])
    outp = os.path.join(d, f"{tag}_r{rank}_h{higher}.ref.txt")
    counts = (C.c_uint64 * 4)()
    assert lib.lime_classify(len(bases), arr, 1, n_reads, n_targ, outp.encode(), tax.encode(), rank, higher, counts) == 0, lib.lime_classify_error()
    return open(outp, "rb").read()


def _rule3_h(host_lists, r, norm):
    """rule 3's h of read r: the largest per-strand sum (v0 + v3, v1 + v2; v0, v1 single-end) over the genomes of its lists"""
    vals = []
    for mx, off, pairs in host_lists:
        p = np.asarray(pairs[int(off[r]):int(off[r + 1])])
        vals.append({int(g): np.float32(np.float32(k & 0xFF) / np.float32(norm)) for g, k in p})
    while len(vals) < 4:
        vals.append({})
    zero = np.float32(0.0)
    h = zero
    for g in set().union(*vals):
        s0 = np.float32(vals[0].get(g, zero) + vals[3].get(g, zero))
        s1 = np.float32(vals[1].get(g, zero) + vals[2].get(g, zero))
        h = max(h, s0, s1)
    return h


@pytest.mark.parametrize("shape", ["c1", "table_free"])
def test_device_classify_at_scale(shape, tmp_path):
    import torch
    from lime_amd import api, _lib
    lib = _lib.load()
    if shape == "c1":        # configs[1]: 10^8 symbols, 10^5 reads x 500 genomes, EBWT=1, four collections
        n, nr, ng, k = 100_000_000, 100_000, 500, 4
    else:                    # a 90 MB table (two levels of bins) at 2^25 symbols: the pass that never builds the table
        n, nr, ng, k = 1 << 25, 300_000, 300, 2
    alpha, norm = 16, 100 + 1 - 16
    d = str(tmp_path)
    tax = _taxonomy_file(os.path.join(d, "lineage.csv"), ng)
    ctx = _ctx()
    lcp = torch.empty(n, dtype=torch.int32, device="cuda")
    da = torch.empty(n, dtype=torch.int32, device="cuda")
    eb = torch.empty(n, dtype=torch.uint8, device="cuda")
    dev, host = {0.25: [], 0.0: []}, {0.25: [], 0.0: []}
    free0 = ctx.host_times()["choose_without_table"]
    for c in range(k):
        ctx.synth_dev(101 + c, 0, n, nr, ng, alpha, 0, lcp, da, eb)
        for beta in (0.25, 0.0):
            li, _ = ctx.fused_choose_lists_dev(lcp, da, eb, n, nr, ng, alpha, norm, beta)
            mx, off, pairs, _ = ctx.fused_choose_dev(lcp, da, eb, n, nr, ng, alpha, norm, beta)
            gm, go, gp = li.get()
            assert np.array_equal(gm, mx) and np.array_equal(go, off) and np.array_equal(gp, pairs), (c, beta)
            dev[beta].append(li)
            host[beta].append((mx.copy(), off.copy(), np.array(pairs)))
    if shape == "table_free":
        assert ctx.host_times()["choose_without_table"] > free0
    del lcp, da, eb
    torch.cuda.empty_cache()
    slow_path_reads = 0
    for beta in (0.25, 0.0):
        for rank, higher in ((0, 0), (1, 0), (1, 1)):
            tx = api.load_taxonomy(tax, rank, higher, ng)
            v, counts = ctx.classify_lists_dev(dev[beta], ng, tx, True)
            vm, cm = api.classify_mem(host[beta], [norm] * k, [beta] * k, ng, tx, True)
            a, b = os.path.join(d, "dev.txt"), os.path.join(d, "mem.txt")
            api.write_classification(a, v)
            api.write_classification(b, vm)
            got = open(a, "rb").read()
            assert got == open(b, "rb").read(), (beta, rank, higher)
            assert got == _res_classify(lib, d, f"b{beta}", host[beta], norm, beta, nr, ng, tax, rank, higher), (beta, rank, higher)
            assert counts == cm and sum(counts) == nr
            if beta == 0.0:
                # reads decided by rule 3 with h < TOL (the pass over every genome): h recomputed from the host lists, in float32
                top = np.max(np.stack([h[0] for h in host[beta]]), axis=0)
                cand = np.nonzero((v["rule"] == 3) & (top == 1))[0]
                slow_path_reads = max(slow_path_reads, sum(1 for r in cand[:4000] if _rule3_h(host[beta], r, norm) < np.float32(0.02)))
            tx.close()
    assert slow_path_reads > 0
    ctx.close()


def test_device_classify_errors(tmp_path):
    import ctypes as C
    import torch
    from lime_amd import api, _lib
    lib = _lib.load()
    g = np.load(os.path.join(ROOT, "tests", "golden", "classify_paired.npz"))
    norm, beta = int(g["norm"]), float(g["beta"])
    n_files, n_reads, n_targ = g["sims"].shape
    tax = str(tmp_path / "lineage.csv")
    open(tax, "wb").write(g["tax"].tobytes())
    ctx = _ctx()
    lists = [ctx.choose_lists_dev(_upload_table(s), n_reads, n_targ, norm, beta) for s in g["sims"]]
    # an idRef at or beyond numGenomes
    short = str(tmp_path / "short.csv")
    open(short, "w").write("\n".join(g["tax"].tobytes().decode().split("\n")[:n_targ - 3]) + "\n")
    with pytest.raises(api.LimeError) as e:
        ctx.classify_lists_dev(lists, n_targ - 4, api.load_taxonomy(short, 1, 0, n_targ - 4))
    assert e.value.code == _lib.ERR_ARG and "beyond numGenomes" in str(e.value)
    # lists with different numbers of reads
    other = ctx.choose_lists_dev(_upload_table(g["sims"][0][:n_reads - 1]), n_reads - 1, n_targ, norm, beta)
    tx = api.load_taxonomy(tax, 1, 0, n_targ)
    with pytest.raises(api.LimeError) as e:
        ctx.classify_lists_dev([lists[0], other], n_targ, tx)
    assert e.value.code == _lib.ERR_ARG and "different numbers of reads" in str(e.value)
    # three lists
    hs = (C.c_void_p * 3)(*[li.h for li in lists[:3]])
    v = np.zeros(n_reads, dtype=api.VERDICT)
    rc = lib.lime_classify_lists_dev(ctx.h, 3, hs, n_targ, tx.h, 1, v.ctypes.data, None, None)
    assert rc == _lib.ERR_ARG and b"2 (single-end reads) or 4 (paired-end reads)" in lib.lime_last_error()
    # a lineage file shorter than numGenomes
    with pytest.raises(api.LimeError) as e:
        api.load_taxonomy(tax, 1, 0, n_targ + 1)
    assert e.value.code == _lib.ERR_ARG and "poor taxonomy" in str(e.value)
    # and the device is fine: the same call without the error gives the reference's bytes
    v, _ = ctx.classify_lists_dev(lists, n_targ, tx, True)
    outp = str(tmp_path / "after.txt")
    api.write_classification(outp, v)
    assert open(outp, "rb").read() == g["out_b1_h0_r1"].tobytes()
    torch.cuda.synchronize()
    ctx.close()
