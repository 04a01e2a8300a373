"""k_classify (lime_classify_lists_dev) where tests/test_classify_lists_gpu.py does not reach: reads whose deciding element is the last of
64, 65, 128 or 129; rows of 1 .. 200 pairs searched for a genome at their first and last pair and absent below, above and between; reads in
one list only and in every pair of lists; counts one and two units apart on the 0.02 tolerance (norm 50 and 100, both value tables); rule 3
over every genome at 1 .. 1000 genomes; the grid stride at 16384 + 5 reads, on a side stream too; 200 seeded random collections.  The
collections and the model are those of tests/classify_cases.py (checked without a GPU in tests/test_classify_cases_cpu.py); the lists are
made on the device (lime_choose_lists_dev).  Every case compares the device's verdicts (every field, pad zero) with lime_classify_mem and
with the model on the same lists, and the bytes of the three classification files: no tolerance anywhere."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import classify_cases as CC  # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    import torch
    from lime_amd import api
    torch.cuda.set_device(0)
    c = api.Context(0)
    yield c
    c.close()


def _upload(sim, stream=None):
    import torch
    from lime_amd import api
    nr, ng = sim.shape
    t = torch.zeros(api.sim_bytes(nr, ng), dtype=torch.uint8, device="cuda")
    t[:nr * ng] = torch.from_numpy(np.ascontiguousarray(sim).reshape(-1)).cuda()
    return t


def run(ctx, col, combos, tmp_path, tag=None, stream=None, tables=None):
    """the collection through the device path for every (binary, higher, rank) of combos, against lime_classify_mem and the model"""
    from lime_amd import api
    n_files, n_targ, norm, beta = len(col["sims"]), col["n_targ"], col["norm"], col["beta"]
    n_reads = col["sims"][0].shape[0]
    tag = tag or col["name"]
    tables = tables or [_upload(s) for s in col["sims"]]
    dev = [ctx.choose_lists_dev(t, n_reads, n_targ, norm, beta, stream) for t in tables]
    host = CC.collection_lists(col)
    for li, want in zip(dev, host):
        mx, off, pairs = li.get()
        assert np.array_equal(mx, want[0]) and np.array_equal(off, want[1]) and np.array_equal(pairs, want[2]), (tag, "lists")
    tax = str(tmp_path / "lineage.csv")
    open(tax, "wb").write(col["tax"])
    files = [str(tmp_path / n) for n in ("dev.txt", "mem.txt")]
    for binary, higher, rank in combos:
        where = (tag, binary, higher, rank)
        tx = api.load_taxonomy(tax, rank, higher, n_targ)
        v, counts = ctx.classify_lists_dev(dev, n_targ, tx, binary, stream)
        vm, cm = api.classify_mem(host, [norm] * n_files, [beta] * n_files, n_targ, tx, binary)
        rep = CC.model_decide(host, [norm] * n_files, [beta] * n_files, n_targ, CC.Tax(col["tax"], rank, higher, n_targ), binary)
        assert CC.same_verdicts(rep, v) is None, (where, "device against the model", CC.same_verdicts(rep, v))
        assert CC.same_verdicts(rep, vm) is None, (where, "lime_classify_mem against the model", CC.same_verdicts(rep, vm))
        assert v.tobytes() == vm.tobytes(), where
        assert counts == cm == [sum(1 for x in rep if x.type == t) for t in "CUAH"], where
        api.write_classification(files[0], v)
        api.write_classification(files[1], vm)
        got = open(files[0], "rb").read()
        assert got == open(files[1], "rb").read() == CC.classification_bytes(rep), where
        tx.close()
    for li in dev:
        li.close()


@pytest.mark.parametrize("n_files", (2, 4))
def test_placement_cases(ctx, n_files, tmp_path):
    run(ctx, CC.placement_cases(n_files), [(b, h, r) for b in (1, 0) for h in (0, 1) for r in (1, 2)] + [(1, 0, 0)], tmp_path)


@pytest.mark.parametrize("norm", (50, 100))
def test_tolerance_tables(ctx, norm, tmp_path):
    for n_files in (2, 4):
        run(ctx, CC.tolerance_tables(n_files, 90, 70, seed=33 + n_files, norm=norm), CC.COMBOS, tmp_path)


def test_near_tie_and_beta0_tables(ctx, tmp_path):
    run(ctx, CC.near_tie_tables(2, 60, 130, seed=31), CC.COMBOS, tmp_path)
    run(ctx, CC.near_tie_tables(4, 60, 200, seed=32), CC.COMBOS, tmp_path)
    run(ctx, CC.beta0_tables(4, 45, 129, seed=35), CC.COMBOS, tmp_path)


@pytest.mark.parametrize("n_targ", CC.EVERY_GENOME_N)
def test_every_genome_cases(ctx, n_targ, tmp_path):
    for kind in CC.EVERY_GENOME_TAX:
        for n_files in (2, 4):
            run(ctx, CC.every_genome_cases(n_targ, kind, n_files), ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 2), (1, 0, 0)), tmp_path)


def test_shifted_lineage(ctx, tmp_path):
    for n_files in (2, 4):
        run(ctx, CC.shifted_lineage_case(n_files), ((1, 1, 1), (0, 1, 1), (1, 0, 1)), tmp_path)


def test_stride_case(ctx, tmp_path):
    run(ctx, CC.stride_case(), ((1, 1, 1), (0, 0, 0)), tmp_path)


def test_stride_case_on_a_side_stream(ctx, tmp_path):
    """With a second context alive, on a stream of torch's.  Best effort: a call that ignored `stream` shows only if the tables' upload
    is still pending on the side stream when the lists are made; sorts are queued in front of it.  Were the queue already drained, the
    test would pass without having shown anything."""
    import torch
    from lime_amd import api
    col = CC.stride_case()
    other = api.Context(0)
    try:
        staged = [_upload(s) for s in col["sims"]]
        filler = torch.rand(16_000_000, device="cuda")
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        assert s.cuda_stream != 0
        tables = [torch.zeros_like(t) for t in staged]                       # not the tables yet
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            for _ in range(4):
                filler = torch.sort(filler.flip(0))[0]
            for t, src in zip(tables, staged):
                t.copy_(src.flip(0).flip(0))
            run(ctx, col, ((1, 1, 1),), tmp_path, tag="stride, side stream", stream=s.cuda_stream, tables=tables)
        s.synchronize()
    finally:
        other.close()


def test_200_fuzz_seeds(ctx, tmp_path):
    for seed in range(200):
        col, rank, higher, binary = CC.fuzz_collection(seed)
        run(ctx, col, ((binary, higher, rank),), tmp_path, tag=f"classify_cases.fuzz_collection({seed})")


def test_zz_device_left_usable(ctx, tmp_path):
    """last in the module: the same context still gives the reference's bytes on classify_paired.npz"""
    from lime_amd import api
    import torch
    g = np.load(os.path.join(ROOT, "tests", "golden", "classify_paired.npz"))
    norm, beta = int(g["norm"]), float(g["beta"])
    _, n_reads, n_targ = g["sims"].shape
    tax = str(tmp_path / "lineage.csv")
    open(tax, "wb").write(g["tax"].tobytes())
    lists = [ctx.choose_lists_dev(_upload(s), n_reads, n_targ, norm, beta) for s in g["sims"]]
    tx = api.load_taxonomy(tax, 1, 1, n_targ)
    v, _ = ctx.classify_lists_dev(lists, n_targ, tx, True)
    outp = str(tmp_path / "after.txt")
    api.write_classification(outp, v)
    assert open(outp, "rb").read() == g["out_b1_h1_r1"].tobytes()
    torch.cuda.synchronize()
