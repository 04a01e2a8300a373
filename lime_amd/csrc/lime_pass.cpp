// lime_pass.cpp -- the passes on device-resident arrays: scratch sizing (ensure_scratch, ensure_binned), the choice of the update path and the bin
// layout (want_binned, bin_layout_of), the density probe, the kernel sequence of a fused pass (fused_dev_impl), the owner-partitioned record
// exchange (lime_fused_records_dev, lime_apply_records_dev), the partition stage's test hook (lime_partition_records_dev) and the detect / score / choose / synth entry points that take device pointers.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>

#include "lime_device.h"
#include "lime_ctx.h"

using namespace lime;
using namespace lime_host;

// scratch sized for an array of n_avail positions; grow-only, so steady-state calls allocate nothing
// (acct: the account the allocations' host time goes to -- the ctx's alloc_ms for a fused pass, NULL for the other callers)
static int ensure_scratch(lime_ctx *c, uint64_t n_avail, bool detect, bool score, hipStream_t st, double *acct)
{
    const size_t n_tiles = (size_t)((n_avail + WIN - 1) / WIN);
    int rc;
    // the four per-tile arrays grow together: one size for all of them (after a growth that failed, the ones that are gone are sized again)
    const size_t have = std::min(std::min(c->summ.cap, c->tile_cnt.cap), std::min(c->tile_off.cap, c->cross.cap));
    const size_t cap = n_tiles > have ? n_tiles + 16 : have;
    if ((rc = c->summ.ensure(cap, st, acct)) || (rc = c->tile_cnt.ensure(cap, st, acct)) || (rc = c->tile_off.ensure(cap, st, acct)) ||
        (rc = c->cross.ensure(cap, st, acct))) return rc;
    if (score) {
        // clusters longer than SMALL_MAX; at most n/(SMALL_MAX+1) exist, sized for 1 in 4 of that
        const uint64_t want_small = 16, want_big = n_avail / (4u * SMALL_MAX) + 65536u;
        if (want_big > 0xFFFFFFF0ull) return fail(LIME_ERR_ARG, "array too long for one shard: %llu", (unsigned long long)n_avail);
        if ((rc = c->small.ensure(want_small, st, acct)) || (rc = c->big.ensure(want_big, st, acct))) return rc;
        if (!c->big_scratch.p) {
            const size_t words = (size_t)BIG_GRID * BIG_SCRATCH_WORDS;
            if ((rc = c->big_scratch.grow(words, acct))) return rc;     // (its time is in the ctx's allocation account; nothing runs on a block that is not there yet: no wait)
            HIP_TRY(hipMemsetAsync(c->big_scratch.p, 0, words * sizeof(uint32_t), st));
            launch_fill_u32(c->big_scratch.p, HT_SIZE, HT_EMPTY, st, BIG_GRID, BIG_SCRATCH_WORDS);      // one launch (32 of them were 0.16 ms of a cold 0.25 ms pass)
            HIP_TRY(hipGetLastError());
        }
    }
    if (detect && (rc = c->wmask.ensure(cap, st, acct))) return rc;
    return LIME_OK;
}

static ScanArgs base_args(lime_ctx *c, const uint32_t *lcp, const uint32_t *da, const uint8_t *ebwt,
                          uint64_t n_own, uint64_t n_avail, int eof, uint32_t n_reads, uint32_t n_refs,
                          uint32_t alpha, uint8_t *sim)
{
    ScanArgs a;
    memset(&a, 0, sizeof a);
    a.lcp = lcp; a.da = da; a.ebwt = ebwt;
    a.n_own = n_own; a.n_avail = n_avail; a.pos_base = 0; a.eof = eof;
    a.n_reads = n_reads; a.n_refs = n_refs; a.alpha = alpha;
    a.n_tiles = (uint32_t)((n_avail + WIN - 1) / WIN);
    a.sim = sim; a.summ = c->summ.p; a.open = reinterpret_cast<OpenRec *>(c->summ.p); a.stats = c->stats.p;
    a.small = c->small.p; a.cross_cap = (uint32_t)c->small.cap; a.big = c->big.p; a.big_cap = (uint32_t)c->big.cap;
    a.tile_cnt = c->tile_cnt.p; a.tile_off = c->tile_off.p; a.cross = c->cross.p; a.out = c->out.p;
    a.wmask = c->wmask.p;
    a.edge = &c->stats.p->edge;
    a.sticky = c->d_sticky; a.dyn = c->d_sticky + 1;
    // Measured with the final round-4 kernels (LIME_SCAN_STATIC_PCT = 0 / 25 / 50 / 75, ABAB): long inputs run faster with every chunk but a
    // workgroup's first handed out as the workgroups get there (configs[2] 1.66 -> 1.60 ms, N = 1e10 14.6 -> 14.4, configs[4]'s shape 17.1 -> 15.9),
    // 1e8 symbols 1 .. 2 % faster with three quarters of the rounds round-robin (fewer trips to the device-wide counter in a 0.2 ms kernel)
    a.static_pct = c->scan_static_pct >= 0 ? (uint32_t)c->scan_static_pct : (n_avail >= 500000000ull ? 0u : 75u);
    a.ablate = c->ablate;
    a.dense_min = c->dense_min;
    a.no_direct = c->no_direct ? 1u : 0u;
    a.flush_gran = c->flush_gran;
    return a;
}

// ---- device-pointer API -----------------------------------------------------------------
// Which way the scan's table updates go.  Binned (records -> bins -> table regions built in LDS, the table
// written once and never cleared) pays for update-dense passes over tables beyond the caches; compare-and-swap
// on the table for sparse ones and wherever the table must be added to (zero_sim == 0, streaming chunks).
static bool want_binned(const lime_ctx *c, uint64_t n_own, size_t sim_bytes, int zero_sim, bool keep_stats, int ebwt)
{
    if (!zero_sim || keep_stats || !n_own) return false;
    if (sim_bytes > ((size_t)BIN_MAX << BIN_SHIFT_MAX) || sim_bytes >= (1ull << CELL_BITS) || sim_bytes > ((uint64_t)MAX_SUB << 32)) return false;
    if (c->upd_pref >= 0) return c->upd_pref == 1;
    if (n_own < (1u << 24)) return false;                 // short passes: the extra launches cost more than they save
    if (sim_bytes < (1u << 20)) return false;             // tiny tables: all updates would land in one or two bins
    // Measured (tools/r03_big.sh, 0.03 updates per symbol, EBWT=1): a table the Infinity Cache holds takes the compare-and-swaps
    // under the scan (configs[1], 50 MB: 0.24 ms against 0.3-0.4 binned); beyond it every update is a 64-byte request to
    // HBM at ~20 G/s while a record costs the later kernels ~7 ps (10^10 symbols: 1 GB table 26.7 ms against 18.4 binned,
    // configs[4]'s 10.3 GB table 31.5 against 20.8, configs[3]'s shape 8.3 against 7.6) -- worth ~0.3 ms of extra launches
    // from about 5 million records on.
    // (round 5, EBWT=1 and a cached table: the compare-and-swap scan runs 12 waves per CU, the record-emitting one 16 -- 0.223 against 0.190 ms
    // per 10^8 symbols -- and the binned pass's fixed launches are 45 us since two of them were merged: level at 10^8 symbols (0.242 : 0.244 ms),
    // binned ahead from there on whatever the density -- 2*10^8: 0.414 against 0.44-0.456, tools/r05_c2_paths.sh)
    if (c->density_known) return sim_bytes > (256u << 20) ? c->density * (double)n_own >= 5e6 : (c->density >= 0.06 || (ebwt && n_own >= 150000000ull));
    // Nothing known yet (a first pass too short for the density probe to pay -- below 2^28 symbols its fixed 0.13 ms is a third to a half of the
    // pass --, or LIME_NO_PROBE): binned.  It is the path that loses little where it loses (configs[1], 0.03 records per symbol: 0.29 against
    // 0.24 ms) and wins much where it wins (the same shape at 0.17: 0.40 against 0.85 ms; text statistics: 0.56 against 4.3 ms); rounds 2-4 took
    // compare-and-swap for tables the Infinity Cache holds.
    return true;
}

// records per owned symbol the pool of the next pass is sized for: what the last pass measured, with a margin (the waves'
// shares differ: ensure_binned adds its own), once one has been read back; the default before that; and never below what
// a repeated pass (pool too small) settled on
// waves of a scan workgroup that count their records together = one producer of k_part: as few as the LDS histogram allows
// (its BIN_MAX counters are shared by the workgroup's producers), so that the partition runs several workgroups per CU
static uint32_t part_prod_waves(const lime_ctx *c, int ebwt, uint32_t n_bins)
{
    const uint32_t wpw = scan_waves_per_wg(ebwt, 0);
    uint32_t best = wpw;
    for (uint32_t pw = wpw; pw >= 1u; --pw) {
        if (wpw % pw) continue;
        const uint32_t h = wpw / pw;
        if (h <= c->part_split && (uint64_t)h * n_bins <= BIN_MAX) best = pw;
    }
    return best;
}

// which record-emitting scan serves a pass: 2 = the scorers write finished records (tables of one or two sub-regions), 1 = through the update queue
static int bin_mode(const lime_ctx *c, uint32_t n_sub) { return (n_sub <= 2u && !c->no_direct) ? 2 : 1; }

double lime_host::sizing_density(const lime_ctx *c)
{
    if (c->pool_density_fixed || !c->density_known) return c->pool_density;
    return c->density * 1.25 + 0.002;             // (rounds 3-4 capped this at the default: a collection denser than 0.2 overflowed its first pool)
}

// the largest part of a wave's records that one of its sub-regions (4 GB of table each, the last one what is left) has to take when the
// cells spread evenly over the table: the sub-regions are sized for THAT share of the wave's records (round 5; rounds 3-4 gave every one of
// the n_sub sub-regions room for the wave's whole share, n_sub times the memory and -- with 32-bit positions -- a third of the reach)
static double sub_share(size_t sim_bytes)
{
    return sim_bytes > (1ull << 32) ? (double)(1ull << 32) / (double)sim_bytes : 1.0;
}

// the scan's per-(wave, sub-region) record counts, its per-(bin, producer) counts and the bins' totals / bases (also what the density probe needs)
static int ensure_bin_counters(lime_ctx *c, size_t segs, size_t want_counts, hipStream_t st, double *acct)
{
    int rc;
    if ((rc = c->wave_cnt.ensure(segs, st, acct)) || (rc = c->counts.ensure(want_counts, st, acct))) return rc;
    if (!c->totals.p && (rc = c->totals.alloc((BIN_MAX + 1) * sizeof(uint32_t)))) return rc;
    if (!c->binbase.p && (rc = c->binbase.alloc((BIN_MAX + 2) * sizeof(uint64_t)))) return rc;
    return LIME_OK;
}

// records the pool and the binned array hold, both of them (they are allocated with 16 records of slack: k_part2 / k_apply read aligned groups of
// four 4-byte records); 0 where one of the two could not be had.  While both are there, pool.cap == recs.cap == this number + 16: ensure_binned
// asks the same size of both, so the min only matters after a growth that failed half way
static size_t pool_records(const lime_ctx *c)
{
    const size_t both = std::min(c->pool.cap, c->recs.cap);
    return both > 16 ? both - 16 : 0;
}

// *p64: the pool holds 2^32 records or more -- the partition kernels then run with 64-bit positions (launch_part)
static int ensure_binned(lime_ctx *c, uint64_t n_own, uint32_t n_waves, uint32_t n_prod, uint32_t n_bins, uint32_t bin_shift,
                         uint32_t n_sub, double share, uint32_t *cap_w, bool *p64, hipStream_t st, double *acct)
{
    int rc;
    const size_t pool_cap = pool_records(c);
    const double per_wave = (double)n_own * sizing_density(c) / (double)n_waves;
    // (the waves draw their windows from counters: their record counts differ by a few % -- x 1.35; a sub-region's part of them by a little more)
    const double per_sub = per_wave * share * (n_sub > 1u ? 1.5 : 1.35);
    if (per_sub > 4.0e9) return fail(LIME_ERR_ARG, "update record pool: more than 2^32 records per scan wave and sub-region");
    uint64_t cw = (((uint64_t)per_sub + c->pool_slack) & ~15ull) + 16u;   // a multiple of 16 records: sub-regions start on a 64-byte line
    const size_t segs = (size_t)n_waves * n_sub;
    if (pool_cap / segs > cw && pool_cap / segs < 0xFFFFFFF0ull) cw = (pool_cap / segs) & ~15ull;      // grow-only: use all of what is there
    size_t want = (size_t)cw * segs;
    // 64-bit positions: their high part rides in a record's bits above t through k_part's stage (31 - bin_shift of them)
    if ((uint64_t)want >> (32u + 31u - bin_shift)) return fail(LIME_ERR_ARG, "update record pool too large for one shard");
    *p64 = c->force_p64 || want >= 0xF0000000ull;
    {   // the second level's 16-bit rows (one per tile, a bin's last one partly used) fit the pool
        const size_t rows_words = ((size_t)tiles_bound(want, n_bins) * row_stride() + 1) / 2;
        if (want < rows_words) want = rows_words;
    }
    if (want > pool_cap && pool_cap >= want - want / 5) {
        // A pool within 20 % of what this pass would ask for is kept: the sizes carry margins of 1.25 x 1.35, a pass that overflows is repeated with
        // a larger one, and replacing a block costs more than it looks -- the driver clears recycled pages inside hipMalloc at about 30 GB/s (the
        // 15.6 GB pool of N = 10^10 clustered was re-grown by 0.02 % after the probe's density had been replaced by the measured one: 4.9 s)
        const uint64_t cw2 = (pool_cap / segs) & ~15ull;
        const size_t want2 = (size_t)cw2 * segs, rows2 = ((size_t)tiles_bound(want2, n_bins) * row_stride() + 1) / 2;
        if (cw2 >= 16 && want2 <= pool_cap && rows2 <= pool_cap) { cw = cw2; want = want2; *p64 = c->force_p64 || want >= 0xF0000000ull; }
    }
    if (want > pool_cap) {
        if ((rc = c->pool.ensure(want + 16, st, acct)) || (rc = c->recs.ensure(want + 16, st, acct))) {      // slack: k_part2 / k_apply read aligned groups of four 4-byte records
            c->pool.release();                                   // (the records cannot be had: the pool is of no use without them)
            return rc;
        }
    }
    if ((rc = ensure_bin_counters(c, segs, (size_t)n_bins * n_prod, st, acct))) return rc;
    if (bin_shift > REGION_SHIFT) {
        if (!c->tbase.p && (rc = c->tbase.alloc((BIN_MAX + 2) * sizeof(uint32_t)))) return rc;
        const size_t want_idx = (size_t)tiles_bound(pool_records(c), n_bins) * (((size_t)1 << (bin_shift - REGION_SHIFT)) + 1);
        if ((rc = c->tidx.ensure(want_idx, st, acct))) return rc;
    }
    const size_t want_reg = ((size_t)n_bins << (bin_shift - REGION_SHIFT)) + 2;
    if (bin_shift > REGION_SHIFT && (rc = c->regbase.ensure(want_reg, st, acct))) return rc;
    *cap_w = (uint32_t)cw;
    return LIME_OK;
}

// The table's bins for the binned update path: one bin per 64 KB region for small tables; else as few levels of fan-out
// as fit: at most 2048 bins of 2^k regions (the bins' open output lines then merge in the L2), more bins only when k would
// pass its limit.  A pure function of the table's size (and LIME_BIN_LEVELS): every rank of an exchange gets the same.
void lime_host::bin_layout_of(uint32_t one_level, uint32_t two_level, bool levels_forced, size_t sim_bytes, uint32_t *n_bins, uint32_t *bin_shift_out)
{
    uint32_t bin_shift = REGION_SHIFT;
    auto bins_at = [&](uint32_t sh) { return (sim_bytes + ((size_t)1 << sh) - 1) >> sh; };
    const uint32_t bmax = BIN_MAX;                        // what the scan's LDS histogram holds
    const uint32_t one = one_level < bmax ? one_level : bmax, two = two_level < bmax ? two_level : bmax;
    if (bins_at(bin_shift) > one) {
        while ((bins_at(bin_shift) > two && bin_shift < BIN_SHIFT_MAX) || bins_at(bin_shift) > bmax) ++bin_shift;
        // fewer, wider bins while that leaves at least 256 of them and at most 64 regions per bin: measured on a 1 GB
        // table (N = 10^10) 477 bins of 32 regions beat 1908 of 8 by 1 ms in 11; a 5 GB table keeps its 1193 bins of 64
        if (!levels_forced)
            while (bin_shift < REGION_SHIFT + 6 && bin_shift < BIN_SHIFT_MAX && bins_at(bin_shift + 1) >= 256) ++bin_shift;
        // Round 6: wider bins still where that brings the table under LINES_BINS bins -- k_part_lines (whole 64-byte lines, two workgroups per CU) then
        // does the first level instead of k_part (pieces of lines: 2 against 3.4 TB/s), and since k_apply_tiles shares a wave among short runs the
        // second level no longer pays for the regions per bin: configs[2] (5 GB: 1193 bins of 64 regions -> 299 of 256) 3.10 -> 2.95 ms per pass,
        // configs[4]'s shape (10.3 GB: 1229 of 128 -> 308 of 512) clustered 31.8 -> 31.0 ms.  Tables beyond 477 x 32 MB = 16 GB keep what they had.
        constexpr uint32_t LINES_BINS = 477;                 // (what fits a CU twice, 32- and 64-bit positions: tools/kres.py gates it)
        if (!levels_forced && bins_at(bin_shift) > LINES_BINS) {
            uint32_t sh = bin_shift;
            while (sh < BIN_SHIFT_MAX && bins_at(sh) > LINES_BINS) ++sh;
            if (bins_at(sh) <= LINES_BINS) bin_shift = sh;
        }
    }
    *n_bins = (uint32_t)bins_at(bin_shift);               // <= BIN_MAX: want_binned checked the table size
    *bin_shift_out = bin_shift;
}
void lime_host::bin_layout(const lime_ctx *c, size_t sim_bytes, uint32_t *n_bins, uint32_t *bin_shift_out)
{
    bin_layout_of(c->bin_one_level, c->bin_two_level, c->bin_levels_forced, sim_bytes, n_bins, bin_shift_out);
}
// the sub-regions of a table (4 GB each) and, for two of them, the first cell of the second as (read, genome index)
void lime_host::sub_layout(size_t sim_bytes, uint32_t n_refs, uint32_t *n_sub, uint32_t *sub_rb, uint32_t *sub_gb)
{
    *n_sub = (uint32_t)((sim_bytes + 0xFFFFFFFFull) >> 32);
    *sub_rb = 0xFFFFFFFFu; *sub_gb = 0u;
    if (*n_sub == 2) { *sub_rb = (uint32_t)((1ull << 32) / n_refs); *sub_gb = (uint32_t)((1ull << 32) - (uint64_t)*sub_rb * n_refs); }
}

// which variant of k_apply_tiles / of k_sort_tiles' row stores a pass of `records` update records takes (lime_set_option "apply_wide" / "sort_nt" force one)
bool lime_host::many_records_of(const lime_ctx *c, double records) { return c->apply_wide >= 0 ? c->apply_wide != 0 : records >= 2e8; }
bool lime_host::big_rows_of(const lime_ctx *c, double records) { return c->sort_nt >= 0 ? c->sort_nt != 0 : records >= 1e8; }

// Update records per owned symbol, estimated from a sample before the first pass on a ctx: the record-emitting scan kernel runs over every
// 2^ps-th chunk of 16 windows -- spread over the whole collection, on all CUs -- with sub-regions of capacity 0: every update record is counted
// (lime_stats_t.n_updates) and none is stored, no histogram entry made, no table touched.  About 1/64 of a pass + one synchronisation.
// Reference: what is sampled is the number of `SimArray_[r][g] += t` executions per symbol, ClusterBWT_DA.cpp:178-184, 243-248.
static int density_probe(lime_ctx *c, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt, uint64_t n_own, uint64_t n_avail, int eof,
                         uint32_t n_reads, uint32_t n_refs, uint32_t alpha, size_t sim_bytes, hipStream_t st)
{
    int rc;
    const auto t0 = std::chrono::steady_clock::now();
    const int ebwt = d_ebwt != nullptr;
    const uint32_t n_tiles = (uint32_t)((n_avail + WIN - 1) / WIN);
    const uint32_t ps = n_own < (1ull << 30) ? 6u : n_own < (1ull << 32) ? 7u : 8u;
    uint32_t n_bins = 0, bin_shift = REGION_SHIFT;
    bin_layout(c, sim_bytes, &n_bins, &bin_shift);
    uint32_t n_sub = 1, sub_rb = 0xFFFFFFFFu, sub_gb = 0u;
    sub_layout(sim_bytes, n_refs, &n_sub, &sub_rb, &sub_gb);
    const uint32_t wpw = scan_waves_per_wg(ebwt, 0);
    const uint32_t grid = scan_grid(ebwt, 0, bin_mode(c, n_sub), n_tiles, c->max_blocks, ps);
    const uint32_t prod_waves = part_prod_waves(c, ebwt, n_bins), n_prod = grid * (wpw / prod_waves);
    if ((rc = ensure_bin_counters(c, (size_t)grid * wpw * n_sub, (size_t)n_bins * n_prod, st, &c->alloc_ms))) return rc;
    launch_zero2(c->stats.p, sizeof(DevStats), nullptr, 0, st);
    ScanArgs a = base_args(c, d_lcp, d_da, d_ebwt, n_own, n_avail, eof, n_reads, n_refs, alpha, nullptr);
    a.upd_mode = 1; a.pool = reinterpret_cast<uint32_t *>(c->stats.p);       // (never written: no slot is below a capacity of 0)
    a.cap_w = 0; a.n_sub = n_sub; a.wave_cnt = c->wave_cnt.p; a.counts = c->counts.p;
    a.n_bins = n_bins; a.bin_shift = bin_shift; a.prod_waves = prod_waves;
    a.sub_rb = sub_rb; a.sub_gb = sub_gb;
    a.probe_shift = ps; a.static_pct = 100u;
    launch_tile(ebwt, 0, a, c->max_blocks, st);
    HIP_TRY(hipGetLastError());
    lime_stats_t s;
    if ((rc = read_stats(c, &s, st))) return rc;                              // waits for the sample
    HIP_TRY(hipMemsetAsync(c->d_sticky, 0, 4, st));                           // (every sub-region "overflowed": not a pass to settle)
    const uint64_t chunk = (uint64_t)wpw * WIN, phys = (n_avail + chunk - 1) / chunk, logical = (phys + (1ull << ps) - 1) >> ps;
    uint64_t sampled = logical * chunk;
    if (sampled > n_own) sampled = n_own;
    c->density = (double)s.n_updates / (double)(sampled ? sampled : 1); c->density_known = true;
    c->probe_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); ++c->n_probes;
    if (c->debug_stats) fprintf(stderr, "density_probe: every %u-th chunk, %llu symbols, %llu updates -> %.4f records per symbol\n", 1u << ps,
                                            (unsigned long long)sampled, (unsigned long long)s.n_updates, c->density);
    return LIME_OK;
}

// keep_stats: this call continues a position-range sequence on the same table (lime_fused_stream):
// cluster / update counters and flags accumulate, only the per-call list counters restart.
int lime_host::fused_dev_impl(lime_ctx *c, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt,
                          uint64_t n_own, uint64_t n_avail, int eof, uint32_t n_reads, uint32_t n_refs,
                          uint32_t alpha, uint8_t *d_sim, int zero_sim, bool keep_stats, hipStream_t st,
                          uint32_t *d_edge, bool no_bin, bool records_only)
{
    int rc;
    if (n_own > n_avail) return fail(LIME_ERR_ARG, "lime_fused_dev: n_own > n_avail");
    if (n_avail && (!d_lcp || !d_da || (!d_sim && !records_only))) return fail(LIME_ERR_ARG, "lime_fused_dev: NULL array");
    if (misaligned(d_lcp, 16) || misaligned(d_da, 16) || misaligned(d_ebwt, 8) || misaligned(d_sim, 16))
        return fail(LIME_ERR_ARG, "lime_fused_dev: device arrays must be 16-byte aligned (ebwt: 8)");
    if (!n_reads || !n_refs) return fail(LIME_ERR_ARG, "lime_fused_dev: n_reads and n_refs must be > 0");
    if (n_refs >= MAX_REFS || (uint64_t)n_reads + n_refs > 0xFFFFFFF0ull)
        return fail(LIME_ERR_ARG, "lime_fused_dev: n_refs must be < 2^%u and n_reads + n_refs <= 2^32 - 16", T_SHIFT);
    if ((n_avail + WIN - 1) / WIN > 0xFFFFFFF0ull) return fail(LIME_ERR_ARG, "array too long for one shard: %llu", (unsigned long long)n_avail);
    if ((rc = ensure_scratch(c, n_avail, false, true, st, &c->alloc_ms))) return rc;
    const size_t sim_bytes = lime_sim_bytes(n_reads, n_refs);
    const int ebwt = d_ebwt != nullptr;
    const uint32_t n_tiles = (uint32_t)((n_avail + WIN - 1) / WIN);
    // no_bin: a chunk of a multi-chunk stream -- its device buffers are reused by later chunks, so the pass could not be
    // repeated after a pool overflow, and the later chunks add to the table by compare-and-swap
    const bool bin_fits = !(sim_bytes > ((size_t)BIN_MAX << BIN_SHIFT_MAX) || sim_bytes >= (1ull << CELL_BITS) || sim_bytes > ((uint64_t)MAX_SUB << 32));
    if (records_only && !bin_fits) return fail(LIME_ERR_ARG, "lime_fused_records_dev: table too large for update records");
    // The first pass on a ctx knows nothing of the collection's update density, which decides the update path and sizes the record pool
    // (rounds 2-4 guessed 0.2 records per symbol: text has 0.24 .. 0.39, the iid generators 0.03 .. 0.12, and a pass that guessed wrong
    // was repeated or ran on the other path).  LiME_paired.sh:62-68 runs every collection ONCE, so the density is sampled first: the
    // scan kernel itself over every 2^k-th chunk of 16 windows, counting its update records without storing one (density_probe).
    if (n_avail && !no_bin && !keep_stats && zero_sim && bin_fits && c->probe && !c->density_known && !c->pool_density_fixed && !c->ablate &&
        c->upd_pref != 0 && n_own >= c->probe_min && sim_bytes >= (1u << 20) && n_tiles < 0x7FF00000u)
        if ((rc = density_probe(c, d_lcp, d_da, d_ebwt, n_own, n_avail, eof, n_reads, n_refs, alpha, sim_bytes, st))) return rc;
    bool binned = n_avail && !no_bin && want_binned(c, n_own, sim_bytes, zero_sim, keep_stats, ebwt);
    if (records_only) binned = true;                      // the records ARE the result: the binned path or nothing
    uint32_t grid = 0, cap_w = 0, n_bins = 0, bin_shift = REGION_SHIFT, n_sub = 1, sub_rb = 0xFFFFFFFFu, sub_gb = 0u, prod_waves = 0, n_prod = 0;
    bool p64 = false, fell_back = false;
    const double share = sub_share(sim_bytes);
    if (binned) {
        bin_layout(c, sim_bytes, &n_bins, &bin_shift);
        sub_layout(sim_bytes, n_refs, &n_sub, &sub_rb, &sub_gb);
        grid = scan_grid(ebwt, 0, bin_mode(c, n_sub), n_tiles, c->max_blocks);
        prod_waves = part_prod_waves(c, ebwt, n_bins);
        n_prod = grid * (scan_waves_per_wg(ebwt, 0) / prod_waves);
        rc = ensure_binned(c, n_own, grid * scan_waves_per_wg(ebwt, 0), n_prod, n_bins, bin_shift, n_sub, share, &cap_w, &p64, st, &c->alloc_ms);
        if (rc == LIME_ERR_NOMEM && !records_only) {
            // no room for the records: the pass runs on the compare-and-swap path -- several times slower where the binned path was wanted --
            // and says so: LIME_FLAG_CAS_FALLBACK in the pass's statistics, the reason in lime_last_error()
            (void)hipGetLastError();
            const std::string why = lime_last_error();
            (void)fail(LIME_ERR_NOMEM, "lime_fused_dev: no device memory for the update records of the binned path (%s): this pass falls back to "
                                       "compare-and-swap on the table (LIME_FLAG_CAS_FALLBACK)", why.c_str());
            binned = false; fell_back = true; ++c->n_fallbacks;
        } else if (rc) return rc;
        if (p64 && !c->by_tiles && bin_shift > REGION_SHIFT) return fail(LIME_ERR_ARG, "LIME_SECOND_LEVEL=sweeps: a record pool of 2^32 records or more needs the tile kernels");
    }
    if ((rc = timing_mark(c, st))) return rc;
    if (keep_stats) {
        HIP_TRY(hipMemsetAsync(&c->stats.p->n_cross, 0, 2 * sizeof(uint32_t), st));      // n_cross, n_big
        HIP_TRY(hipMemsetAsync(&c->stats.p->n_open, 0, sizeof(uint32_t), st));
        if (zero_sim && !binned) HIP_TRY(hipMemsetAsync(d_sim, 0, sim_bytes, st));
    } else {
        // the counters and (compare-and-swap path: the binned path writes every byte of the table itself) the table, one launch
        static_assert(sizeof(DevStats) % 4 == 0, "whole words");
        const bool zt = zero_sim && !binned && d_sim;
        launch_zero2(c->stats.p, sizeof(DevStats), zt ? d_sim : nullptr, zt ? (sim_bytes & ~(size_t)15) : 0, st);
        if (zt && (sim_bytes & 15)) HIP_TRY(hipMemsetAsync(d_sim + (sim_bytes & ~(size_t)15), 0, sim_bytes & 15, st));
    }
    if (records_only) {                                   // the long clusters' updates leave as records too
        if (!c->bigrec.p && (rc = c->bigrec.acquire(16u << 20))) return rc;
        if (!c->bigrec_n.p && (rc = c->bigrec_n.alloc(sizeof(uint32_t)))) return rc;
        HIP_TRY(hipMemsetAsync(c->bigrec_n.p, 0, sizeof(uint32_t), st));
        c->rec_n_bins = n_bins; c->rec_bin_shift = bin_shift;
    }
    if (!n_avail && !records_only) { if ((rc = timing_mark(c, st)) || (rc = timing_mark(c, st)) || (rc = timing_mark(c, st))) return rc; return LIME_OK; }
    ScanArgs a = base_args(c, d_lcp, d_da, d_ebwt, n_own, n_avail, eof, n_reads, n_refs, alpha, d_sim);
    if (d_edge) a.edge = d_edge;                          // a chunk of a stream: its own (cleared) word
    if (binned) {
        a.upd_mode = 1; a.pool = c->pool.p; a.cap_w = cap_w; a.n_sub = n_sub; a.wave_cnt = c->wave_cnt.p; a.counts = c->counts.p;
        a.n_bins = n_bins; a.bin_shift = bin_shift; a.prod_waves = prod_waves;
        a.sub_rb = sub_rb; a.sub_gb = sub_gb;
    }
    if (records_only) { a.sim = nullptr; a.bigrec = c->bigrec.p; a.bigrec_n = c->bigrec_n.p; a.bigrec_cap = (uint32_t)c->bigrec.cap; }
    if ((rc = timing_mark(c, st))) return rc;
    launch_tile(ebwt, 0, a, c->max_blocks, st);
    if ((rc = timing_mark(c, st))) return rc;
    if (!(binned && !c->ablate)) launch_resolve(0, a, st);
    if (binned && !c->ablate) {                          // (timing experiments cut the scan short: nothing to partition)
        const bool tiles = bin_shift > REGION_SHIFT && c->by_tiles && !records_only;
        launch_rowscan_resolve(a, c->counts.p, c->totals.p, n_bins, n_prod, st);      // (the open segments are closed in the same launch)
        launch_bin_bases(c->totals.p, c->binbase.p, tiles ? c->tbase.p : nullptr, n_bins, st);
        const uint32_t *recs = c->recs.p;
        if (c->p64_test_base && !records_only && (c->by_tiles || bin_shift == REGION_SHIFT)) {      // tests: positions from a base near a multiple of 2^32 on
            launch_add_u64(c->binbase.p, (size_t)n_bins + 1, c->p64_test_base, st);
            recs = c->recs.p - c->p64_test_base;                   // (an address only: the kernels add positions >= the base to it)
        }
        launch_part(a, n_prod, c->binbase.p, const_cast<uint32_t *>(recs), st, p64, c->part_lines != 0);
        if (records_only) {
            // the records grouped by bin are the result: the owners of the bins build the table (lime_apply_records_dev)
        } else if (bin_shift > REGION_SHIFT && c->by_tiles) {      // second level tile by tile into the (by now free) pool, regions from the tiles' runs
            // (how many records: what the last pass counted per symbol, once one has been read back)
            const double expect = c->density_known ? c->density * (double)n_own : 0.0;
            launch_apply_by_tiles(d_sim, sim_bytes, recs, c->binbase.p, n_bins, bin_shift, c->tbase.p, c->tidx.p,
                                  reinterpret_cast<uint16_t *>(c->pool.p), many_records_of(c, expect), st, big_rows_of(c, expect), !c->p64_test_base);
        } else if (bin_shift > REGION_SHIFT) {            // second level into the (by now free) pool, then regions from there
            uint32_t *recs2 = c->pool.p;
            launch_part2(c->recs.p, c->binbase.p, n_bins, bin_shift, c->regbase.p, recs2, st);
            // the base after the last region = the total (regions past the table's end hold no records)
            HIP_TRY(hipMemcpyAsync(c->regbase.p + ((size_t)n_bins << (bin_shift - REGION_SHIFT)), c->binbase.p + n_bins, sizeof(uint64_t),
                                   hipMemcpyDeviceToDevice, st));
            launch_apply(d_sim, sim_bytes, recs2, c->regbase.p, bin_shift, st);
        } else {
            launch_apply(d_sim, sim_bytes, recs, c->binbase.p, bin_shift, st);
        }
    }
    launch_score_big(ebwt, a, c->big_scratch.p, st);      // after k_apply: its compare-and-swaps add to the finished table
    if ((rc = timing_mark(c, st))) return rc;
    HIP_TRY(hipGetLastError());
    if (!keep_stats) {
        lime_ctx::Last &l = c->last;
        l.valid = true; l.binned = binned; l.lcp = d_lcp; l.da = d_da; l.ebwt = d_ebwt; l.n_own = n_own; l.n_avail = n_avail;
        l.eof = eof; l.n_reads = n_reads; l.n_refs = n_refs; l.alpha = alpha; l.sim = d_sim; l.zero_sim = zero_sim; l.st = st;
        l.n_waves = grid * scan_waves_per_wg(ebwt, 0);
        l.own_total = n_own; l.records_only = records_only; l.share = share; l.fell_back = fell_back;
    } else {
        c->last.own_total += n_own;         // a later chunk of a stream: the update counter keeps accumulating
        c->last.binned = false;             // and the pass stored in `last` can no longer be repeated on its own
    }
    return LIME_OK;
}

extern "C" int lime_fused_dev(lime_ctx *c, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt,
                              uint64_t n_own, uint64_t n_avail, int eof, uint32_t n_reads, uint32_t n_refs,
                              uint32_t alpha, uint8_t *d_sim, int zero_sim, void *stream)
{
    int rc = check_ctx(c, "lime_fused_dev"); if (rc) return rc;
    return fused_dev_impl(c, d_lcp, d_da, d_ebwt, n_own, n_avail, eof, n_reads, n_refs, alpha, d_sim, zero_sim, false,
                          (hipStream_t)stream);
}


// ---- owner-partitioned exchange of table updates (several GPUs, large tables) -------------------------------------
// Instead of a private table per rank and a dense reduce-scatter of whole tables (every rank allocates and writes T bytes
// and moves T (G-1)/G over xGMI), a rank leaves its updates as records grouped by table bin; the owner of a range of bins
// receives the slices of its bins from every rank and builds its block of the table alone: T/G bytes per rank, about
// 4 bytes per update over the links.  The reference's counterpart is the cluster-range split of ClusterBWT_DA.cpp:630-670
// with all threads adding into one table.
extern "C" int lime_records_layout(lime_ctx *c, uint32_t n_reads, uint32_t n_refs, uint32_t *n_bins, uint32_t *bin_shift)
{
    int rc = check_ctx(c, "lime_records_layout"); if (rc) return rc;
    if (!n_reads || !n_refs || !n_bins || !bin_shift) return fail(LIME_ERR_ARG, "lime_records_layout: bad argument");
    bin_layout(c, lime_sim_bytes(n_reads, n_refs), n_bins, bin_shift);
    return LIME_OK;
}

extern "C" int lime_fused_records_dev(lime_ctx *c, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt,
                                      uint64_t n_own, uint64_t n_avail, int eof, uint32_t n_reads, uint32_t n_refs,
                                      uint32_t alpha, void *stream)
{
    int rc = check_ctx(c, "lime_fused_records_dev"); if (rc) return rc;
    return fused_dev_impl(c, d_lcp, d_da, d_ebwt, n_own, n_avail, eof, n_reads, n_refs, alpha, nullptr, 1, false,
                          (hipStream_t)stream, nullptr, false, true);
}

extern "C" int lime_records_get(lime_ctx *c, lime_records_t *out, uint64_t *h_binbase, void *stream)
{
    int rc = check_ctx(c, "lime_records_get"); if (rc) return rc;
    if (!out) return fail(LIME_ERR_ARG, "lime_records_get: out is NULL");
    if (!c->last.valid || !c->last.records_only) return fail(LIME_ERR_ARG, "lime_records_get: the last pass on this ctx was not lime_fused_records_dev");
    hipStream_t st = (hipStream_t)stream;
    uint32_t nb = 0;
    HIP_TRY(hipMemcpyAsync(&nb, c->bigrec_n.p, sizeof nb, hipMemcpyDeviceToHost, st));
    if (h_binbase) HIP_TRY(hipMemcpyAsync(h_binbase, c->binbase.p, ((size_t)c->rec_n_bins + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (nb > c->bigrec.cap) return fail(LIME_ERR_NOMEM, "more update records of long clusters (%u) than their list holds (%u)", nb, (uint32_t)c->bigrec.cap);
    out->n_bins = c->rec_n_bins; out->bin_shift = c->rec_bin_shift;
    out->d_recs = c->recs.p; out->d_binbase = c->binbase.p; out->d_bigrecs = c->bigrec.p; out->n_bigrecs = nb;
    return LIME_OK;
}

// the same without a word read back (lime_comm_exchange_records takes bases and counts from the device): the arrays, where the
// long clusters' record count lives, and what their list holds
int lime_internal_records_peek(lime_ctx *c, lime_records_t *out, const uint32_t **d_bigrec_n, uint32_t *bigrec_cap)
{
    int rc = check_ctx(c, "lime_comm_exchange_records"); if (rc) return rc;
    if (!c->last.valid || !c->last.records_only) return fail(LIME_ERR_ARG, "lime_comm_exchange_records: the last pass on this ctx was not lime_fused_records_dev");
    out->n_bins = c->rec_n_bins; out->bin_shift = c->rec_bin_shift;
    out->d_recs = c->recs.p; out->d_binbase = c->binbase.p; out->d_bigrecs = c->bigrec.p; out->n_bigrecs = 0;
    *d_bigrec_n = c->bigrec_n.p; *bigrec_cap = (uint32_t)c->bigrec.cap;
    return LIME_OK;
}

// d_rx: the record slices received for this rank's bins, source after source; h_srcoff[s * (nb + 1) + b]: where source s's
// records of local bin b start in d_rx (h_srcoff[s * (nb + 1) + nb]: where they end).  Builds bytes [cell_lo, cell_lo +
// block_bytes) of the table -- cell_lo = first own bin << bin_shift -- in d_block: every byte is written.
extern "C" int lime_apply_records_dev(lime_ctx *c, uint32_t n_src, const uint32_t *d_rx, const uint64_t *h_srcoff, uint32_t nb,
                                      uint32_t bin_shift, const uint64_t *d_bigrecs, uint64_t n_bigrecs, uint64_t cell_lo,
                                      uint64_t block_bytes, uint8_t *d_block, void *stream)
{
    int rc = check_ctx(c, "lime_apply_records_dev"); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!n_src || !h_srcoff || !d_block || (n_bigrecs && !d_bigrecs)) return fail(LIME_ERR_ARG, "lime_apply_records_dev: NULL argument");
    if (bin_shift < REGION_SHIFT || bin_shift > BIN_SHIFT_MAX || (block_bytes & 15u) || misaligned(d_block, 16) ||
        block_bytes > ((uint64_t)nb << bin_shift) || (cell_lo & (((uint64_t)1 << bin_shift) - 1u)))
        return fail(LIME_ERR_ARG, "lime_apply_records_dev: bad block geometry");
    // (k_tile_bases counts the bins' tiles in LDS arrays of BIN_MAX words, and tbase holds BIN_MAX + 2)
    if (nb > BIN_MAX) return fail(LIME_ERR_ARG, "lime_apply_records_dev: nb %u beyond the %u bins a block may have", nb, BIN_MAX);
    if (!nb || !block_bytes) return LIME_OK;
    // where every bin starts in the regrouped array: the sources' counts added up
    std::vector<uint64_t> dstbase((size_t)nb + 1, 0);
    for (uint32_t b = 0; b < nb; ++b) {
        uint64_t cnt = 0;
        for (uint32_t s = 0; s < n_src; ++s) {
            const uint64_t lo = h_srcoff[(size_t)s * (nb + 1) + b], hi = h_srcoff[(size_t)s * (nb + 1) + b + 1];
            if (hi < lo) return fail(LIME_ERR_ARG, "lime_apply_records_dev: source offsets not ascending");
            cnt += hi - lo;
        }
        dstbase[b + 1] = dstbase[b] + cnt;
    }
    const uint64_t total = dstbase[nb];
    if (total > 0xF0000000ull) return fail(LIME_ERR_ARG, "lime_apply_records_dev: too many records for one block");
    if (total && !d_rx) return fail(LIME_ERR_ARG, "lime_apply_records_dev: d_rx is NULL");
    const size_t f2 = (size_t)1 << (bin_shift - REGION_SHIFT), n_reg = (size_t)nb * f2;
    size_t xwant = (size_t)total + 16;
    {   // (the second level's 16-bit tile rows)
        const size_t rows_words = ((size_t)tiles_bound(total, nb) * row_stride() + 1) / 2 + 16;
        if (xwant < rows_words) xwant = rows_words;
    }
    if (xwant > std::min(c->xrecs.cap, c->xrecs2.cap) &&           // (the two grow together)
        ((rc = c->xrecs.ensure(xwant + total / 8, st, nullptr)) || (rc = c->xrecs2.ensure(xwant + total / 8, st, nullptr)))) return rc;
    if (bin_shift > REGION_SHIFT) {
        if (!c->tbase.p && (rc = c->tbase.alloc((BIN_MAX + 2) * sizeof(uint32_t)))) return rc;
        const size_t want_idx = (size_t)tiles_bound(total, nb) * (f2 + 1);
        if ((rc = c->tidx.ensure(want_idx, st, nullptr))) return rc;
    }
    const size_t off_words = (size_t)n_src * (nb + 1) + (nb + 1);
    if ((rc = c->xoff.ensure(off_words, st, nullptr)) || (rc = c->xreg.ensure(n_reg + 2, st, nullptr))) return rc;
    uint64_t *d_srcoff = c->xoff.p, *d_dstbase = c->xoff.p + (size_t)n_src * (nb + 1);
    // the offsets go up from a pinned buffer of the ctx (the caller's and this function's vectors go out of scope while the copy
    // may still be queued): the only wait is for the PREVIOUS call's copy out of that buffer, long done by now
    if (c->ev_xoff_pending) { HIP_TRY(hipEventSynchronize(c->ev_xoff)); c->ev_xoff_pending = false; }
    if (off_words > c->h_xoff_cap) {
        if (c->h_xoff) (void)hipHostFree(c->h_xoff);
        c->h_xoff = nullptr; c->h_xoff_cap = 0;
        HIP_TRY(hipHostMalloc(&c->h_xoff, (off_words + off_words / 4) * sizeof(uint64_t)));
        c->h_xoff_cap = off_words + off_words / 4;
    }
    if (!c->ev_xoff) HIP_TRY(hipEventCreateWithFlags(&c->ev_xoff, hipEventDisableTiming));
    memcpy(c->h_xoff, h_srcoff, (size_t)n_src * (nb + 1) * sizeof(uint64_t));
    memcpy(c->h_xoff + (size_t)n_src * (nb + 1), dstbase.data(), ((size_t)nb + 1) * sizeof(uint64_t));
    HIP_TRY(hipMemcpyAsync(d_srcoff, c->h_xoff, off_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(c->ev_xoff, st)); c->ev_xoff_pending = true;
    launch_regroup(d_rx, d_srcoff, n_src, nb, d_dstbase, c->xrecs.p, st);
    if (bin_shift > REGION_SHIFT && c->by_tiles) {
        launch_apply_by_tiles(d_block, (size_t)block_bytes, c->xrecs.p, d_dstbase, nb, bin_shift, c->tbase.p, c->tidx.p,
                              reinterpret_cast<uint16_t *>(c->xrecs2.p), many_records_of(c, (double)total), st, big_rows_of(c, (double)total));
    } else if (bin_shift > REGION_SHIFT) {
        launch_part2(c->xrecs.p, d_dstbase, nb, bin_shift, c->xreg.p, c->xrecs2.p, st);
        HIP_TRY(hipMemcpyAsync(c->xreg.p + n_reg, d_dstbase + nb, sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
        launch_apply(d_block, (size_t)block_bytes, c->xrecs2.p, c->xreg.p, bin_shift, st);
    } else {
        launch_apply(d_block, (size_t)block_bytes, c->xrecs.p, d_dstbase, bin_shift, st);
    }
    launch_apply_bigrecs(d_bigrecs, n_bigrecs, cell_lo, cell_lo + block_bytes, d_block, st);
    HIP_TRY(hipGetLastError());
    return LIME_OK;
}

// ---- test and diagnosis hook: the first-level partition alone on a record pool the caller made ---------------------------------
// what runs on the stream once the arguments have been checked and the raw counts built; the caller waits for the stream whatever this returns
// (counts is the caller's vector, and the copies out of it are queued here)
static int partition_records_run(lime_ctx *c, uint32_t n_prod, uint32_t prod_waves, uint32_t n_sub, uint32_t cap_w, const uint32_t *h_pool,
                                 const uint32_t *h_wave_cnt, uint32_t n_bins, uint32_t bin_shift, uint32_t *d_out, const std::vector<uint32_t> &counts,
                                 bool p64, uint64_t *h_binbase, hipStream_t st)
{
    int rc;
    const size_t segs = (size_t)n_prod * prod_waves * n_sub, pool_words = segs * cap_w;
    if ((rc = c->pool.ensure(pool_words + 16, st, nullptr)) || (rc = ensure_bin_counters(c, segs, counts.size(), st, nullptr))) return rc;
    if (pool_words) HIP_TRY(hipMemcpyAsync(c->pool.p, h_pool, pool_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->wave_cnt.p, h_wave_cnt, segs * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(c->counts.p, counts.data(), counts.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    ScanArgs a;
    memset(&a, 0, sizeof a);
    a.upd_mode = 1; a.pool = c->pool.p; a.cap_w = cap_w; a.n_sub = n_sub; a.wave_cnt = c->wave_cnt.p; a.counts = c->counts.p;
    a.n_bins = n_bins; a.bin_shift = bin_shift; a.prod_waves = prod_waves;
    launch_bin_rowscan(c->counts.p, c->totals.p, n_bins, n_prod, st);
    launch_bin_bases(c->totals.p, c->binbase.p, nullptr, n_bins, st);
    uint32_t *out = d_out;
    if (c->p64_test_base) {                               // positions from a base near a multiple of 2^32 on, as in fused_dev_impl
        launch_add_u64(c->binbase.p, (size_t)n_bins + 1, c->p64_test_base, st);
        out = d_out - c->p64_test_base;                   // (an address only: the kernels add positions >= the base to it)
    }
    launch_part(a, n_prod, c->binbase.p, out, st, p64, c->part_lines != 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_binbase, c->binbase.p, ((size_t)n_bins + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    return LIME_OK;
}

// The contract is in include/lime_hip.h.  Everything is checked on the host before the first launch: the kernels trust the counts (they
// index the pool with them) and the records' bins (they index LDS counters with them).
extern "C" int lime_partition_records_dev(lime_ctx *c, uint32_t n_prod, uint32_t prod_waves, uint32_t n_sub, uint32_t cap_w, const uint32_t *h_pool,
                                          const uint32_t *h_wave_cnt, uint32_t n_bins, uint32_t bin_shift, uint32_t *d_out, uint64_t out_words,
                                          uint64_t *h_binbase, int *kernel, void *stream)
{
    int rc = check_ctx(c, "lime_partition_records_dev"); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!h_pool || !h_wave_cnt || !d_out || !h_binbase || !kernel) return fail(LIME_ERR_ARG, "lime_partition_records_dev: NULL argument");
    if (!n_prod || prod_waves < 1u || prod_waves > 16u || n_sub < 1u || n_sub > MAX_SUB || (cap_w & 15u))
        return fail(LIME_ERR_ARG, "lime_partition_records_dev: want n_prod >= 1, 1 <= prod_waves <= 16, 1 <= n_sub <= %u, cap_w a multiple of 16", MAX_SUB);
    if (bin_shift < REGION_SHIFT || bin_shift > BIN_SHIFT_MAX || n_bins < 1u || n_bins > BIN_MAX)
        return fail(LIME_ERR_ARG, "lime_partition_records_dev: want %u <= bin_shift <= %u and 1 <= n_bins <= %u", REGION_SHIFT, BIN_SHIFT_MAX, BIN_MAX);
    if (misaligned(d_out, 64)) return fail(LIME_ERR_ARG, "lime_partition_records_dev: d_out must be 64-byte aligned");
    // (a producer's stream -- its segments, each padded to four records -- is addressed with 32 bits, and so is counts[bin][producer])
    if ((uint64_t)prod_waves * n_sub * cap_w > 0xFFFFFFF0ull || (uint64_t)n_bins * n_prod > 0xFFFFFFF0ull)
        return fail(LIME_ERR_ARG, "lime_partition_records_dev: pool too large");
    const size_t segs = (size_t)n_prod * prod_waves * n_sub;
    uint64_t total = 0;
    for (size_t i = 0; i < segs; ++i) {
        if (h_wave_cnt[i] > cap_w) return fail(LIME_ERR_ARG, "lime_partition_records_dev: segment %zu holds %u records, cap_w is %u", i, h_wave_cnt[i], cap_w);
        total += h_wave_cnt[i];
    }
    if (total > out_words) return fail(LIME_ERR_ARG, "lime_partition_records_dev: %llu records, out_words is %llu", (unsigned long long)total, (unsigned long long)out_words);
    // 64-bit positions: their high part rides in a record's bits above t through k_part's stage (31 - bin_shift of them)
    if ((c->p64_test_base + total) >> (32u + 31u - bin_shift)) return fail(LIME_ERR_ARG, "lime_partition_records_dev: positions beyond what bin_shift %u leaves room for", bin_shift);
    // the raw counts[bin][producer] the scan would have left
    std::vector<uint32_t> counts((size_t)n_bins * n_prod, 0u);
    for (size_t i = 0; i < segs; ++i) {
        const uint32_t sub = (uint32_t)(i % n_sub), p = (uint32_t)(i / ((size_t)prod_waves * n_sub));
        const uint32_t *seg = h_pool + i * cap_w;
        for (uint32_t k = 0; k < h_wave_cnt[i]; ++k) {
            const uint32_t b = rec_bin(seg[k], sub, bin_shift);
            if (b >= n_bins) return fail(LIME_ERR_ARG, "lime_partition_records_dev: record %u of segment %zu lies in bin %u of %u", k, i, b, n_bins);
            ++counts[(size_t)b * n_prod + p];
        }
    }
    const bool p64 = c->force_p64 || total >= 0xF0000000ull;
    *kernel = part_uses_lines(n_bins, p64, c->part_lines != 0) ? 1 : 0;
    c->last.valid = false;                                // no pass of lime_fused_dev: lime_get_stats has nothing to repeat
    rc = partition_records_run(c, n_prod, prod_waves, n_sub, cap_w, h_pool, h_wave_cnt, n_bins, bin_shift, d_out, counts, p64, h_binbase, st);
    const hipError_t e = hipStreamSynchronize(st);        // (also where the run failed half way: its copies read `counts`)
    if (rc) return rc;
    HIP_TRY(e);
    for (uint32_t b = 0; b <= n_bins; ++b) h_binbase[b] -= c->p64_test_base;
    return LIME_OK;
}

extern "C" int lime_detect_dev(lime_ctx *c, const uint32_t *d_lcp, const uint32_t *d_da, uint64_t n_own,
                               uint64_t n_avail, int eof, uint64_t pos_base, uint32_t n_reads, uint32_t alpha,
                               const lime_cluster_t **d_clusters, uint64_t *n_clusters, uint64_t *max_len,
                               void *stream)
{
    int rc = check_ctx(c, "lime_detect_dev"); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!d_clusters || !n_clusters || !max_len) return fail(LIME_ERR_ARG, "lime_detect_dev: NULL output");
    *d_clusters = nullptr; *n_clusters = 0; *max_len = 0;
    if (n_own > n_avail) return fail(LIME_ERR_ARG, "lime_detect_dev: n_own > n_avail");
    if (n_avail && (!d_lcp || !d_da)) return fail(LIME_ERR_ARG, "lime_detect_dev: NULL array");
    if (misaligned(d_lcp, 16) || misaligned(d_da, 16))
        return fail(LIME_ERR_ARG, "lime_detect_dev: device arrays must be 16-byte aligned");
    if (!n_avail) return LIME_OK;
    if ((rc = ensure_scratch(c, n_avail, true, false, st, nullptr))) return rc;
    c->last.valid = false;
    HIP_TRY(hipMemsetAsync(c->stats.p, 0, sizeof(DevStats), st));
    ScanArgs a = base_args(c, d_lcp, d_da, nullptr, n_own, n_avail, eof, n_reads, 1, alpha, nullptr);
    a.pos_base = pos_base;
    launch_tile(0, 1, a, c->max_blocks, st);
    launch_resolve(1, a, st);
    launch_scan_tiles(c->tile_cnt.p, c->tile_off.p, a.n_tiles, c->total.p, st);
    HIP_TRY(hipGetLastError());
    unsigned long long total = 0;
    lime_stats_t s;
    HIP_TRY(hipMemcpyAsync(&total, c->total.p, sizeof total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&s, c->stats.p, sizeof s, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = flags_to_rc(s.flags & LIME_FLAG_HALO))) return rc;
    if (total != s.n_clusters) return fail(LIME_ERR_HIP, "internal: record count %llu != counter %llu", total, (unsigned long long)s.n_clusters);
    if (total > c->out.cap && (rc = c->out.grow((size_t)total + (size_t)total / 8 + 1024, nullptr))) return rc;      // (the stream has just been waited for)
    if (total) {
        a.out = c->out.p;
        launch_emit(a, st);
        HIP_TRY(hipGetLastError());
    }
    *d_clusters = c->out.p; *n_clusters = total; *max_len = s.max_len;
    return LIME_OK;
}

// pos_base: the collection position of d_da[0] (the records' pStart are collection positions)
int lime_host::score_dev_impl(lime_ctx *c, const uint32_t *d_da, const uint8_t *d_ebwt, uint64_t n,
                          const lime_cluster_t *d_clusters, uint64_t n_clusters, uint32_t n_reads,
                          uint32_t n_refs, uint8_t *d_sim, int zero_sim, uint64_t pos_base, hipStream_t st)
{
    int rc;
    if (!d_sim || (n && !d_da) || (n_clusters && !d_clusters)) return fail(LIME_ERR_ARG, "lime_score_dev: NULL array");
    if (misaligned(d_sim, 4)) return fail(LIME_ERR_ARG, "lime_score_dev: d_sim must be 4-byte aligned");
    if (!n_reads || !n_refs) return fail(LIME_ERR_ARG, "lime_score_dev: n_reads and n_refs must be > 0");
    if (n_refs >= MAX_REFS || (uint64_t)n_reads + n_refs > 0xFFFFFFF0ull)
        return fail(LIME_ERR_ARG, "lime_score_dev: n_refs must be < 2^%u and n_reads + n_refs <= 2^32 - 16", T_SHIFT);
    if ((rc = ensure_scratch(c, n, false, true, st, nullptr))) return rc;
    // every listed cluster longer than the in-tile limit lands in the big list
    if (n_clusters + 16 > 0xFFFFFFF0ull) return fail(LIME_ERR_ARG, "too many clusters for one call");
    if ((rc = c->big.ensure((size_t)n_clusters + 16, st, nullptr))) return rc;
    c->last.valid = false;
    const int ebwt = d_ebwt != nullptr;
    const size_t sim_bytes = lime_sim_bytes(n_reads, n_refs);
    uint64_t batches = (n_clusters + 255) / 256;          // 64 clusters per wave, 4 waves per workgroup
    // Binned updates for the list flow too (round 4; ClusterBWT_DA.cpp:301-340 with the arrays resident): the table is built from
    // scratch (zero_sim) and 16-byte aligned.  A pool that proves too small (the list says nothing about its update density) is found out right here --
    // the call waits for the pass -- and the list is scored again by compare-and-swap.
    bool binned = zero_sim && n_clusters && !pos_base && !misaligned(d_sim, 16) && sim_bytes >= (1u << 20) &&
                  sim_bytes <= ((size_t)BIN_MAX << BIN_SHIFT_MAX) && sim_bytes < (1ull << CELL_BITS) && sim_bytes <= ((uint64_t)MAX_SUB << 32) &&
                  c->upd_pref == 1;
    // (only when asked for, LIME_UPDATE_PATH=bin: measured with the arrays resident -- tools/bench_list.py, clustered generator, 306 MB table -- the
    // list flow is bound by its per-cluster gather of da / ebwt, not by its updates: 1e8 symbols, 1.7e7 updates 1.09 ms by compare-and-swap
    // against 1.33 binned; 4e8 symbols, 6.6e7 updates 4.25 against 4.56)
    for (int attempt = 0; attempt < 2; ++attempt) {
        {
            const bool zt = zero_sim && !binned && d_sim;
            launch_zero2(c->stats.p, sizeof(DevStats), zt ? d_sim : nullptr, zt ? (sim_bytes & ~(size_t)15) : 0, st);
            if (zt && (sim_bytes & 15)) HIP_TRY(hipMemsetAsync(d_sim + (sim_bytes & ~(size_t)15), 0, sim_bytes & 15, st));
        }
        if (!n_clusters) return LIME_OK;
        ScanArgs a = base_args(c, nullptr, d_da, d_ebwt, n, n, 1, n_reads, n_refs, 0, d_sim);
        a.pos_base = pos_base;
        uint32_t blocks = (uint32_t)(batches < c->list_blocks ? batches : c->list_blocks);
        uint32_t n_bins = 0, bin_shift = REGION_SHIFT, n_sub = 1, cap_w = 0;
        bool p64 = false;
        if (binned) {
            if (blocks > 1024u) blocks = 1024u;           // fewer, longer producers: a partition workgroup per scoring workgroup
            bin_layout(c, sim_bytes, &n_bins, &bin_shift);
            sub_layout(sim_bytes, n_refs, &n_sub, &a.sub_rb, &a.sub_gb);
            if ((rc = ensure_binned(c, n, blocks * (SCAN_WG / 64), blocks, n_bins, bin_shift, n_sub, sub_share(sim_bytes), &cap_w, &p64, st, nullptr))) return rc;
            a.upd_mode = 1; a.pool = c->pool.p; a.cap_w = cap_w; a.n_sub = n_sub; a.wave_cnt = c->wave_cnt.p; a.counts = c->counts.p;
            a.n_bins = n_bins; a.bin_shift = bin_shift; a.prod_waves = SCAN_WG / 64;
        }
        launch_score_list(ebwt, a, d_clusters, n_clusters, blocks, st);
        if (binned) {
            launch_bin_rowscan(c->counts.p, c->totals.p, n_bins, blocks, st);
            launch_scan_tiles(c->totals.p, c->binbase.p, n_bins, reinterpret_cast<unsigned long long *>(c->binbase.p + n_bins), st);
            launch_part(a, blocks, c->binbase.p, c->recs.p, st, p64, c->part_lines != 0);
            if (bin_shift > REGION_SHIFT) launch_apply_by_tiles(d_sim, sim_bytes, c->recs.p, c->binbase.p, n_bins, bin_shift, c->tbase.p, c->tidx.p,
                                                                reinterpret_cast<uint16_t *>(c->pool.p), many_records_of(c, 0.0), st, big_rows_of(c, 0.0));
            else launch_apply(d_sim, sim_bytes, c->recs.p, c->binbase.p, bin_shift, st);
        }
        launch_score_big(ebwt, a, c->big_scratch.p, st);  // (after the table is built: its compare-and-swaps add to it)
        HIP_TRY(hipGetLastError());
        if (!binned) break;
        lime_stats_t s;
        if ((rc = read_stats(c, &s, st))) return rc;      // waits for the pass
        if (!(s.flags & LIME_FLAG_POOL_FULL)) break;
        binned = false;                                   // the table is incomplete: again, by compare-and-swap
    }
    return LIME_OK;
}

extern "C" int lime_score_dev(lime_ctx *c, const uint32_t *d_da, const uint8_t *d_ebwt, uint64_t n,
                              const lime_cluster_t *d_clusters, uint64_t n_clusters, uint32_t n_reads,
                              uint32_t n_refs, uint8_t *d_sim, int zero_sim, void *stream)
{
    int rc = check_ctx(c, "lime_score_dev"); if (rc) return rc;
    return score_dev_impl(c, d_da, d_ebwt, n, d_clusters, n_clusters, n_reads, n_refs, d_sim, zero_sim, 0, (hipStream_t)stream);
}

extern "C" int lime_choose_dev(lime_ctx *c, const uint8_t *d_sim, uint32_t n_reads, uint32_t n_refs,
                               uint8_t *d_row_max, uint32_t *d_row_nnz, void *stream)
{
    int rc = check_ctx(c, "lime_choose_dev"); if (rc) return rc;
    if (!d_sim || !d_row_max || !d_row_nnz) return fail(LIME_ERR_ARG, "lime_choose_dev: NULL array");
    if (misaligned(d_sim, 16)) return fail(LIME_ERR_ARG, "lime_choose_dev: d_sim must be 16-byte aligned (and lime_sim_bytes() long)");
    if (!n_reads) return LIME_OK;
    launch_choose(d_sim, n_reads, n_refs, d_row_max, d_row_nnz, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return LIME_OK;
}

extern "C" int lime_synth_dev(lime_ctx *c, uint64_t seed, uint64_t i0, uint64_t count, uint32_t n_reads,
                              uint32_t n_refs, uint32_t alpha, uint32_t mode, uint32_t *d_lcp, uint32_t *d_da,
                              uint8_t *d_ebwt, void *stream)
{
    int rc = check_ctx(c, "lime_synth_dev"); if (rc) return rc;
    if (!n_reads || !n_refs) return fail(LIME_ERR_ARG, "lime_synth_dev: n_reads and n_refs must be > 0");
    if (!count) return LIME_OK;
    launch_synth(seed, i0, count, n_reads, n_refs, alpha, mode, d_lcp, d_da, d_ebwt, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return LIME_OK;
}

