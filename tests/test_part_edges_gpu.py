"""The first-level partition -- k_bin_rowscan, k_bin_bases, then k_part<512, BIN_MAX, P64> or k_part_lines<P64> -- through
lime_partition_records_dev on the hand-made record pools of tests/part_cases.py (checked without a GPU in tests/test_part_cases_cpu.py), along
every path: whole lines and scattered pieces, 32- and 64-bit positions, and positions shifted so that 2^32 falls on a bin's first position,
inside a producer's range several tiles in, and on the records of the final flush of the carries.  The output array is filled with 0xABABABAB
with 1024 guard words on either side; afterwards the bin bases must equal the numpy model's, and the output the model's word for word once
every (bin, producer) range is sorted on both sides -- the only order the kernels are free in.  No tolerance anywhere; a mismatch names bin,
producer and the tiles of the producer's stream; nothing here is run a second time."""
import functools

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import part_cases as PC

pytestmark = pytest.mark.gpu

G = PC.GUARD
OUT_FILL_I32 = PC.OUT_FILL - (1 << 32)
# option -> value per path; one context per path (module scope).  The "_base" paths get their p64_test_base per call, from the case's model
PATHS = {
    "lines": {"part_lines": 1},
    "scatter": {"part_lines": 0},
    "lines_p64": {"part_lines": 1, "force_p64": 1},
    "scatter_p64": {"part_lines": 0, "force_p64": 1},
    "lines_base": {"part_lines": 1},
    "scatter_base": {"part_lines": 0},
}
ALL = list(PC.CASES) + PC.FUZZ
KERNEL_NAME = {0: "k_part", 1: "k_part_lines"}


@functools.lru_cache(maxsize=2)
def _case(name):
    """the case, its model and the bases taken from it, computed once per case (the tests are ordered by case; nothing writes to them)"""
    c = PC.make(name)
    m = PC.Model(c)
    return c, m, PC.p64_bases(c, m)


def _context(path):
    import lime_amd
    c = lime_amd.Context()
    for k, v in PATHS[path].items():
        c.set_option(k, v)
    return c


@pytest.fixture(scope="module")
def ctxs():
    made = {path: _context(path) for path in PATHS}
    yield made
    for c in made.values():
        c.close()


def _launch(torch, ctx, c, total, base=0, **change):
    """-> (the buffer: G guard words, `total` words, G guard words; bin bases; kernel)"""
    buf = torch.full((total + 2 * G,), OUT_FILL_I32, dtype=torch.int32, device=torch.device("cuda", 0))
    out = buf[G + change.pop("out_shift", 0):]
    assert out.data_ptr() % 64 == change.pop("out_align", 0)
    ctx.set_option("p64_test_base", base)
    a = dict(n_prod=c.n_prod, prod_waves=c.prod_waves, n_sub=c.n_sub, cap_w=c.cap_w, pool=c.pool, wave_cnt=c.wave_cnt, n_bins=c.n_bins,
             bin_shift=c.bin_shift, out_words=total)
    a.update(change)
    binbase, kernel = ctx.partition_records(a["n_prod"], a["prod_waves"], a["n_sub"], a["cap_w"], a["pool"], a["wave_cnt"], a["n_bins"],
                                            a["bin_shift"], out, a["out_words"])
    return buf, binbase, kernel


def _check(c, m, buf, binbase, what):
    msg = PC.compare(c, m, buf.cpu().numpy().view(np.uint32), binbase)
    assert msg is None, f"{what}: {msg}"


def _serves(path, n_bins, kernel, what):
    """which kernel must have served: k_part wherever whole lines are switched off and from 1537 bins up (three bins per thread at most),
    k_part_lines on the lines paths up to 256 bins; between those the device's LDS decides, and the test records it"""
    assert kernel in (0, 1)
    if not path.startswith("lines") or n_bins > PC.LINES_BINS_MAX:
        assert kernel == 0, f"{what}: {KERNEL_NAME[kernel]} ran"
    elif n_bins <= 256:
        assert kernel == 1, f"{what}: {KERNEL_NAME[kernel]} ran: the whole-line kernel was not tested"
    print(f"kernel served: {path} {what} n_bins {n_bins}: {KERNEL_NAME[kernel]}")


def _run(torch, ctx, name, path, base=0, what=None):
    c, m, _ = _case(name)
    what = what or f"{name} / {path}" + (f" / base {base:#x}" if base else "")
    buf, binbase, kernel = _launch(torch, ctx, c, m.total, base)
    _check(c, m, buf, binbase, what)
    _serves(path, c.n_bins, kernel, what)
    return kernel


@pytest.mark.parametrize("name,path", [(n, p) for n in ALL for p in PATHS])
def test_output_equals_the_model(ctxs, record_property, name, path):
    import torch
    if not path.endswith("_base"):
        record_property("kernel", KERNEL_NAME[_run(torch, ctxs[path], name, path)])
        return
    bases = _case(name)[2]
    assert bases["above"] == (1 << 33) + 48
    for kind, base in bases.items():
        k = _run(torch, ctxs[path], name, path, base, f"{name} / {path} / {kind} {base:#x}")
        record_property(f"kernel_{kind}", KERNEL_NAME[k])


@pytest.mark.parametrize("path", ["lines", "scatter", "lines_p64"])
def test_recycled_scratch_of_another_shape(path):
    """a small call, the largest case, a small call with another n_bins, n_sub and n_prod, on ONE context of its own: the scratch arrays grow and
    are recycled (filled with 0xA5 under the test hooks), so nothing may depend on what they held"""
    import torch
    ctx = _context(path)
    try:
        for name in ("pad_mod4", "carry_trickle", "sub_regions_2_25", "one_record"):
            _run(torch, ctx, name, path, what=f"{name} / {path} on a used context")
    finally:
        ctx.close()


@pytest.mark.parametrize("path", ["lines", "scatter"])
def test_two_calls_back_to_back(ctxs, path):
    """two calls into different outputs, checked after both: the second call's pool, counts and bases go through the same scratch as the first's"""
    import torch
    a, ma, _ = _case("first_piece")
    b = PC.make("prod_waves_6")
    mb = PC.Model(b)
    bufa, basea, _ = _launch(torch, ctxs[path], a, ma.total)
    bufb, baseb, _ = _launch(torch, ctxs[path], b, mb.total)
    _check(a, ma, bufa, basea, f"first call / {path}")
    _check(b, mb, bufb, baseb, f"second call / {path}")


@pytest.mark.parametrize("path", ["lines", "scatter"])
def test_a_fused_pass_before_and_after(path):
    """the hook leaves the context usable: a binned pass against the oracle, a partition call (which grows the pool and replaces counts, bases
    and wave counts), the same pass again -- and lime_get_stats after the hook repeats nothing"""
    import torch
    ctx = _context(path)
    try:
        ctx.set_option("update_path", "bin")
        n, nr, ng = 300_000, 2_000, 60
        lcp, da, eb = O.synth(7, 0, n, nr, ng, 16, 1)
        cl, nc, ml = O.detect(lcp, da, nr, 16)
        exp = O.score(da, eb, cl, nr, ng, threads=4)
        sim, gnc, gml = ctx.fused(lcp, da, eb, nr, ng, 16)
        assert (gnc, gml) == (nc, ml) and np.array_equal(sim, exp), "before the partition call"
        repeats = ctx.host_times()["repeats"]
        _run(torch, ctx, "tile_edges", path, what=f"tile_edges / {path} between two passes")
        ctx.stats()
        assert ctx.host_times()["repeats"] == repeats
        sim, gnc, gml = ctx.fused(lcp, da, eb, nr, ng, 16)
        assert (gnc, gml) == (nc, ml) and np.array_equal(sim, exp), "after the partition call"
    finally:
        ctx.close()


def _refusals(c):
    over = c.wave_cnt.copy(); over[2] = c.cap_w + 1
    far = c.pool.copy(); far[0] = (c.n_bins << c.bin_shift) | 5              # segment 0 holds a record: its bin becomes n_bins
    return {
        "cap_w_24": dict(cap_w=24),
        "count_above_cap_w": dict(wave_cnt=over),
        "prod_waves_17": dict(prod_waves=17),
        "n_sub_9": dict(n_sub=9),
        "bin_shift_15": dict(bin_shift=15),
        "bin_shift_26": dict(bin_shift=26),
        "n_bins_3073": dict(n_bins=PC.BIN_MAX + 1),
        "record_in_bin_n_bins": dict(pool=far),
        "out_words_one_short": dict(out_words=c.total - 1),
        "d_out_off_by_16_bytes": dict(out_shift=4, out_align=16),
    }


REFUSED = ["cap_w_24", "count_above_cap_w", "prod_waves_17", "n_sub_9", "bin_shift_15", "bin_shift_26", "n_bins_3073", "record_in_bin_n_bins",
           "out_words_one_short", "d_out_off_by_16_bytes"]


@pytest.mark.parametrize("what", REFUSED)
def test_refused_arguments_leave_the_output_alone(ctxs, what):
    """LIME_ERR_ARG before anything is launched (the checks are on the host), and the same call without the change is taken"""
    import torch
    from lime_amd._lib import ERR_ARG, LimeError
    c = PC.make("pad_mod4")
    m = PC.Model(c)
    change = _refusals(c)
    assert list(change) == REFUSED
    ok = dict(n_prod=c.n_prod, prod_waves=c.prod_waves, n_sub=c.n_sub, cap_w=c.cap_w, pool=c.pool, wave_cnt=c.wave_cnt, n_bins=c.n_bins,
              bin_shift=c.bin_shift, out_words=m.total)
    assert PC.geometry_error(**ok) is None
    ch = {k: v for k, v in change[what].items() if k != "out_shift"}
    assert PC.geometry_error(**{**ok, **ch}) is not None
    dev = torch.device("cuda", 0)
    for path in ("lines", "scatter"):
        buf = torch.full((m.total + 2 * G,), OUT_FILL_I32, dtype=torch.int32, device=dev)
        a = {**ok, **ch}
        out = buf[G + change[what].get("out_shift", 0):]
        assert out.data_ptr() % 64 == a.pop("out_align", 0)
        ctxs[path].set_option("p64_test_base", 0)
        with pytest.raises(LimeError) as e:
            ctxs[path].partition_records(a["n_prod"], a["prod_waves"], a["n_sub"], a["cap_w"], a["pool"], a["wave_cnt"], a["n_bins"], a["bin_shift"],
                                         out, a["out_words"])
        assert e.value.code == ERR_ARG
        torch.cuda.synchronize()
        assert bool((buf == OUT_FILL_I32).all()), f"{what} / {path}: the output was written"
        bufok, binbase, _ = _launch(torch, ctxs[path], c, m.total)
        _check(c, m, bufok, binbase, f"the call without {what} / {path}")
