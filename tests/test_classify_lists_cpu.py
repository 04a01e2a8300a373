"""Read assignment over lists held in memory (lime_classify_mem, the CPU reference of the device path lime_classify_lists_dev):
the decision factored out of lime_classify.cpp must give the bytes the reference's own Classify builds wrote
(tests/golden/classify_*.npz) for every BIN / HIGHER / rank key, from the clusterChoose lists of the fixtures' tables.  Host code."""
import glob
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "classify_*.npz")))
KEYS = [f"out_b{b}_h{h}_r{r}" for b in (1, 0) for h in (0, 1) for r in (0, 1, 2, 4)]


def lists_of(sim, norm, beta):
    """clusterChoose of one table as the library's lists: row maxima, row offsets of the passing rows' cells, (idRef, sim) pairs"""
    sim = np.asarray(sim, dtype=np.uint8)
    mx = sim.max(axis=1) if sim.shape[1] else np.zeros(sim.shape[0], np.uint8)
    passing = mx.astype(np.float32) / np.float32(norm) > np.float32(beta)
    nz = (sim > 0) & passing[:, None]
    off = np.zeros(sim.shape[0] + 1, dtype=np.uint64)
    off[1:] = np.cumsum(nz.sum(axis=1))
    r, g = np.nonzero(nz)
    pairs = np.stack([g.astype(np.uint32), sim[r, g].astype(np.uint32)], axis=1)
    return mx, off, pairs


def fixture_lists(g):
    norm, beta = int(g["norm"]), float(g["beta"])
    return [lists_of(s, norm, beta) for s in g["sims"]], norm, beta


@pytest.mark.parametrize("case", CASES, ids=[os.path.basename(c)[9:-4] for c in CASES])
def test_classify_mem_matches_reference(case, tmp_path):
    from lime_amd import api
    g = np.load(case)
    lists, norm, beta = fixture_lists(g)
    n_files, n_reads, n_targ = g["sims"].shape
    tax = str(tmp_path / "lineage.csv")
    open(tax, "wb").write(g["tax"].tobytes())
    seen = 0
    for key in KEYS:
        if key not in g.files:
            continue
        binary, higher, rank = int(key[5]), int(key[8]), int(key[11:])
        tx = api.load_taxonomy(tax, rank, higher, n_targ)
        v, counts = api.classify_mem(lists, [norm] * n_files, [beta] * n_files, n_targ, tx, binary)
        outp = str(tmp_path / f"{key}.txt")
        api.write_classification(outp, v)
        got = open(outp, "rb").read()
        assert got == g[key].tobytes(), key
        assert [int((v["type"] == ord(t)).sum()) for t in "CUAH"] == counts
        assert set(np.unique(v["rule"][v["type"] == ord("U")])) <= {0}
        seen += 1
    assert seen >= 14


def test_classify_mem_covers_every_rule_and_verdict(tmp_path):
    """across the fixtures the device path's tests run on: rules 1, 2 and 3, and the verdicts C, U, A and H all occur"""
    from lime_amd import api
    rules, types = set(), set()
    for case in CASES:
        g = np.load(case)
        lists, norm, beta = fixture_lists(g)
        n_files, _, n_targ = g["sims"].shape
        tax = str(tmp_path / "lineage.csv")
        open(tax, "wb").write(g["tax"].tobytes())
        for rank, higher in ((1, 1), (2, 1), (0, 0)):
            v, _ = api.classify_mem(lists, [norm] * n_files, [beta] * n_files, n_targ, api.load_taxonomy(tax, rank, higher, n_targ))
            rules |= set(int(x) for x in v["rule"])
            types |= set(chr(x) for x in v["type"])
    assert {0, 1, 2, 3} <= rules and set("CUAH") <= types, (rules, types)


def test_taxonomy_and_list_errors(tmp_path):
    from lime_amd import api, _lib
    g = np.load(os.path.join(ROOT, "tests", "golden", "classify_single.npz"))
    lists, norm, beta = fixture_lists(g)
    n_files, _, n_targ = g["sims"].shape
    tax = str(tmp_path / "lineage.csv")
    open(tax, "wb").write(g["tax"].tobytes())
    with pytest.raises(api.LimeError) as e:                 # a lineage file shorter than numGenomes
        api.load_taxonomy(tax, 1, 0, n_targ + 1)
    assert e.value.code == _lib.ERR_ARG and "poor taxonomy" in str(e.value)
    with pytest.raises(api.LimeError) as e:                 # an idRef beyond numGenomes
        small = "\n".join(g["tax"].tobytes().decode().split("\n")[:n_targ - 1]) + "\n"
        open(tax + ".short", "w").write(small)
        tx = api.load_taxonomy(tax + ".short", 1, 0, n_targ - 2)
        api.classify_mem(lists, [norm] * n_files, [beta] * n_files, n_targ - 2, tx)
    assert e.value.code == _lib.ERR_ARG and "beyond numGenomes" in str(e.value)
    with pytest.raises(api.LimeError) as e:                 # three lists
        api.classify_mem(lists + lists[:1], [norm] * 3, [beta] * 3, n_targ, api.load_taxonomy(tax, 1, 0, n_targ))
    assert e.value.code == _lib.ERR_ARG


def test_lime_paired_program_is_built_and_explains_itself():
    exe = os.path.join(ROOT, "lime_amd", "bin", "LiME_paired")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s"], check=True, timeout=1200)
    p = subprocess.run([exe], capture_output=True, timeout=60)
    assert p.returncode == 1 and b"no .clrs, .out or .res.* files" in p.stderr


def test_classify_kernel_resources_and_exec_lint():
    """lime_classify_kernel.hip through `make resources`: no VGPR spills or scratch, no cross-lane operation under a partial EXEC mask"""
    import shutil
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "lime_amd", "csrc"), "-s", "resources"], capture_output=True, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-2000:]
    assert "k_classify" in out and out.count("exec lint ok") == 2, out[-2000:]
