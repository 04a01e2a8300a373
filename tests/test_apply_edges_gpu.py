"""The apply stage -- k_regroup, then k_tile_bases + k_sort_tiles + k_apply_tiles<WIDE, 0>, or k_part2 + k_apply, or k_apply alone, then
k_apply_bigrecs -- through lime_apply_records_dev on the hand-made record streams of tests/apply_cases.py (checked without a GPU in
tests/test_apply_cases_cpu.py), along every path its bin_shift allows.  The block and 4 KB of guard bytes behind it are filled with 0xAB, and
the block must then equal the numpy model byte for byte with the guard untouched: no tolerance anywhere.  A mismatch names the regions and
tiles it lies in; nothing here is run a second time."""
import functools

import numpy as np
import pytest

from tests import apply_cases as AC

pytestmark = pytest.mark.gpu

GUARD = 4096
# option -> value per path; one context per path (module scope)
PATHS = {
    "tiles": {"second_level": "tiles", "apply_wide": 0, "sort_nt": 0},
    "wide": {"second_level": "tiles", "apply_wide": 1, "sort_nt": 0},
    "sort_nt": {"second_level": "tiles", "apply_wide": 0, "sort_nt": 1},
    "sweeps": {"second_level": "sweeps"},
    "one_level": {},
}


def paths_of(bin_shift):
    return ["one_level"] if bin_shift == AC.REGION_SHIFT else ["tiles", "wide", "sort_nt", "sweeps"]


@functools.lru_cache(maxsize=2)
def _case(name):
    """the case and its model, computed once per case (the tests are ordered by case; nothing writes to either)"""
    c = AC.make(name)
    m = AC.model(c)
    m.setflags(write=False)
    return c, m


@pytest.fixture(scope="module")
def ctxs():
    import lime_amd
    made = {}
    for path, opts in PATHS.items():
        c = lime_amd.Context()
        for k, v in opts.items():
            c.set_option(k, v)
        made[path] = c
    yield made
    for c in made.values():
        c.close()


def _upload(torch, c):
    dev = torch.device("cuda", 0)
    rx = torch.from_numpy(c.rx.view(np.int32).copy()).to(dev) if len(c.rx) else torch.empty(1, dtype=torch.int32, device=dev)
    big = torch.from_numpy(c.bigrecs.view(np.int64).copy()).to(dev) if len(c.bigrecs) else None
    return rx, big


def _launch(torch, ctx, c, rx, big):
    """-> the buffer: block_bytes of block, GUARD bytes behind it; no synchronise"""
    buf = torch.full((c.block_bytes + GUARD,), 0xAB, dtype=torch.uint8, device=rx.device)
    ctx.apply_records_dev(c.n_src, rx, c.srcoff, c.nb, c.bin_shift, big, len(c.bigrecs), c.cell_lo, c.block_bytes, buf)
    return buf


def _where(c, bad):
    """the cells that differ by region, and the tiles of the regions' bins"""
    regions = np.unique(bad >> AC.REGION_SHIFT)
    bins = np.unique(bad >> c.bin_shift)
    tiles_per_bin, _ = AC.runs(c)
    return (f"{len(bad)} cells differ in {len(regions)} regions {regions[:12].tolist()} of bins {bins[:12].tolist()} "
            f"(tiles per bin {[tiles_per_bin[b] for b in bins[:12]]}); first cells {bad[:8].tolist()}")


def _check(torch, c, want, buf, what):
    torch.cuda.synchronize()
    n = c.block_bytes
    if n > 4 << 20:                                                       # compared on the device; the cells come back only where it fails
        want_t = torch.tensor(want, device=buf.device)                  # (a copy: the model stays read-only)
        if not torch.equal(buf[:n], want_t):
            bad = torch.nonzero(buf[:n] != want_t).flatten().cpu().numpy()
            got = buf[:n][torch.from_numpy(bad[:8]).to(buf.device)].cpu().tolist()
            raise AssertionError(f"{what}: {_where(c, bad)}: got {got}, want {want[bad[:8]].tolist()}")
    else:
        got = buf[:n].cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f"{what}: {_where(c, bad)}: got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")
    assert bool((buf[n:] == 0xAB).all()), f"{what}: bytes behind the block were written"


def _run(torch, ctx, name, what):
    c, want = _case(name)
    rx, big = _upload(torch, c)
    _check(torch, c, want, _launch(torch, ctx, c, rx, big), what)


@pytest.mark.parametrize("name,path", [(n, p) for n, (sh, _) in AC.CASES.items() for p in paths_of(sh)])
def test_block_equals_the_model(ctxs, name, path):
    import torch
    _run(torch, ctxs[path], name, f"{name} / {path}")


@pytest.mark.parametrize("name,lg", [(n, lg) for n in AC.GROUPED for lg in range(1, 7)])
def test_block_equals_the_model_with_forced_lanes_per_run(ctxs, name, lg):
    """option apply_group: 2^lg lanes share a run, whatever the regions per bin (6: a wave per run); it is process-wide"""
    import torch
    ctx = ctxs["tiles"]
    ctx.set_option("apply_group", lg)
    try:
        _run(torch, ctx, name, f"{name} / apply_group {lg}")
    finally:
        ctx.set_option("apply_group", 0)


@pytest.mark.parametrize("path", ["tiles", "sweeps"])
def test_recycled_scratch_of_another_shape(path):
    """a small call, the 96 MB case, a small call with another nb, bin_shift and n_src, on ONE context of its own: the scratch arrays grow and are
    recycled (filled with 0xA5 under the test hooks), so nothing may depend on what they held"""
    import torch
    import lime_amd
    ctx = lime_amd.Context()
    try:
        for k, v in PATHS[path].items():
            ctx.set_option(k, v)
        for name in ("padding", "wrap_alternate", "regroup_7", "per_region_16"):
            _run(torch, ctx, name, f"{name} / {path} on a used context")
    finally:
        ctx.close()


@pytest.mark.parametrize("path", ["tiles", "sweeps"])
def test_two_calls_back_to_back(ctxs, path):
    """no synchronise between two calls with different source offsets into different blocks: the second call's offsets go through the same
    pinned staging buffer as the first's"""
    import torch
    a, b = AC.make("regroup_7"), AC.make("empty_bins")
    want_a, want_b = AC.model(a), AC.model(b)
    rxa, biga = _upload(torch, a)
    rxb, bigb = _upload(torch, b)
    torch.cuda.synchronize()
    bufa = _launch(torch, ctxs[path], a, rxa, biga)
    bufb = _launch(torch, ctxs[path], b, rxb, bigb)
    _check(torch, a, want_a, bufa, f"first call / {path}")
    _check(torch, b, want_b, bufb, f"second call / {path}")


REFUSED = {
    "nb_beyond_bin_max": dict(nb=AC.BIN_MAX + 1, srcoff=np.zeros((1, AC.BIN_MAX + 2), dtype=np.uint64)),
    "bin_shift_15": dict(bin_shift=15),
    "bin_shift_26": dict(bin_shift=26),
    "block_bytes_not_16": dict(block_bytes=24),
    "block_misaligned": dict(block_align=8),
    "block_beyond_bins": dict(block_bytes=(2 << 17) + 16),
    "cell_lo_not_bin_aligned": dict(cell_lo=1 << 16),
    "descending_offsets": dict(srcoff=np.array([[0, 5, 3]], dtype=np.uint64)),
    "no_source": dict(n_src=0),
}


@pytest.mark.parametrize("what", list(REFUSED))
def test_refused_arguments_leave_the_block_alone(ctxs, what):
    """LIME_ERR_ARG before anything is launched"""
    import torch
    from lime_amd._lib import ERR_ARG, LimeError
    a = dict(n_src=1, nb=2, bin_shift=17, block_bytes=1 << 17, cell_lo=0, srcoff=np.array([[0, 4, 8]], dtype=np.uint64), block_align=0)
    assert AC.geometry_error(**a) is None
    a.update(REFUSED[what])
    assert AC.geometry_error(**a) is not None
    dev = torch.device("cuda", 0)
    rx = torch.full((16,), (1 << 17) | 5, dtype=torch.int32, device=dev)
    buf = torch.full(((2 << 17) + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    block = buf[a["block_align"]:]
    assert block.data_ptr() % 16 == a["block_align"]
    for path in ("tiles", "sweeps"):
        with pytest.raises(LimeError) as e:
            ctxs[path].apply_records_dev(a["n_src"], rx, a["srcoff"], a["nb"], a["bin_shift"], None, 0, a["cell_lo"], a["block_bytes"], block)
        assert e.value.code == ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == 0xAB).all())
    # and the same call without the change is taken
    ok = dict(n_src=1, nb=2, bin_shift=17, block_bytes=1 << 17, cell_lo=0, srcoff=np.array([[0, 4, 8]], dtype=np.uint64))
    ctxs["tiles"].apply_records_dev(ok["n_src"], rx, ok["srcoff"], ok["nb"], ok["bin_shift"], None, 0, ok["cell_lo"], ok["block_bytes"], buf)
    torch.cuda.synchronize()
    assert int(buf[5]) == 4 and int(buf[:1 << 17].to(torch.int64).sum()) == 4 and bool((buf[1 << 17:] == 0xAB).all())
