// lime_api.cpp -- the core of the C ABI in include/lime_hip.h: error reporting, lime_init / lime_shutdown, the option table (set_option),
// timing and statistics (lime_get_stats repeats a pass whose record pool was too small), and the small host-only exports.  The passes themselves
// are in lime_pass.cpp, the host-pointer entry points in lime_stream.cpp, clusterChoose / Classify in lime_choose.cpp, the index builder in
// lime_build.cpp, the genome index and the merge into it in lime_merge.cpp, device memory in lime_alloc.cpp.  There is no CPU code path for the computation: every entry point needs a HIP device.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>

#include "lime_device.h"
#include "lime_ctx.h"

using namespace lime;
using namespace lime_host;

static thread_local std::string g_err;

int lime_host::fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char *lime_last_error(void) { return g_err.c_str(); }
extern "C" const char *lime_version(void) { return "lime_amd 0.1 (gfx950)"; }
extern "C" void lime_free(void *p) { free(p); }
extern "C" int lime_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
// the device with the most free memory; devices within 1 GiB of the best count as equally free and `salt`
// (a pid) picks among them, so that processes started together do not all land on device 0
extern "C" int lime_pick_device(unsigned salt)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 1) return 0;
    std::vector<size_t> fr(n, 0);
    size_t best = 0;
    for (int d = 0; d < n; ++d) {
        size_t f = 0, t = 0;
        if (hipSetDevice(d) == hipSuccess && hipMemGetInfo(&f, &t) == hipSuccess) fr[d] = f;
        if (fr[d] > best) best = fr[d];
    }
    std::vector<int> cand;
    for (int d = 0; d < n; ++d) if (fr[d] + ((size_t)1 << 30) >= best) cand.push_back(d);
    return cand.empty() ? 0 : cand[salt % cand.size()];
}

extern "C" size_t lime_sim_bytes(uint32_t n_reads, uint32_t n_refs)
{
    size_t b = (size_t)n_reads * n_refs;
    return (b + 15u) & ~(size_t)15u;
}

// ---- options: every tuning / test knob of the library, by name.  Nothing here changes a result; most change which kernels run.
static int set_option(lime_ctx *c, const char *key, const char *s)
{
    if (!key || !s) return fail(LIME_ERR_ARG, "lime_set_option: NULL argument");
    auto is = [&](const char *k) { return !strcmp(key, k); };
    const long v = atol(s);
    if (is("update_path")) c->upd_pref = !strcmp(s, "cas") ? 0 : !strcmp(s, "bin") ? 1 : -1;
    else if (is("bin_levels")) {
        unsigned a1 = 0, a2 = 0;
        if (!*s) { c->bin_one_level = BIN_ONE_LEVEL; c->bin_two_level = BIN_TWO_LEVEL; c->bin_levels_forced = false; }
        else if (sscanf(s, "%u,%u", &a1, &a2) == 2 && a1 >= 1 && a2 >= 1 && a1 <= BIN_MAX && a2 <= BIN_MAX) { c->bin_one_level = a1; c->bin_two_level = a2; c->bin_levels_forced = true; }
        else return fail(LIME_ERR_ARG, "bin_levels: want \"one,two\" with 1 <= one, two <= %u", BIN_MAX);
    }
    else if (is("pool_density")) { const double d = atof(s); if (d > 0) { c->pool_density = d; c->pool_density_fixed = true; } }      // tests: force a small pool
    else if (is("scan_static_pct")) c->scan_static_pct = v >= 0 && v <= 100 ? (int)v : -1;
    else if (is("second_level")) c->by_tiles = strcmp(s, "sweeps") != 0;
    else if (is("part_split")) { if (v >= 1 && v <= 16) c->part_split = (uint32_t)v; }
    else if (is("pool_slack")) { if (v >= 0) c->pool_slack = (uint32_t)v; }
    else if (is("no_probe")) c->probe = v == 0;
    else if (is("probe_min")) { const unsigned long long u = strtoull(s, nullptr, 0); c->probe_min = u < (1ull << 24) ? (1ull << 24) : u; }
    else if (is("force_p64")) c->force_p64 = v != 0;
    else if (is("p64_test_base")) { c->p64_test_base = strtoull(s, nullptr, 0) & ~15ull; if (c->p64_test_base) c->force_p64 = true; }
    else if (is("max_blocks")) c->max_blocks = v > 0 ? (uint32_t)v : 0u;
    else if (is("choose_free")) c->choose_free = *s ? (v != 0) : -1;
    else if (is("apply_wide")) c->apply_wide = *s ? (v != 0) : -1;
    else if (is("sort_nt")) c->sort_nt = *s ? (v != 0) : -1;
    else if (is("part_lines")) c->part_lines = *s ? (v != 0) : -1;
    else if (is("no_staging")) c->no_staging = v != 0 || !*s;
    else if (is("force_staging")) c->force_staging = v != 0 || !*s;
    else if (is("detect_chunk")) c->detect_chunk = strtoull(s, nullptr, 10);
    else if (is("score_chunk")) c->score_chunk = strtoull(s, nullptr, 10);
    else if (is("force_rccl")) c->force_rccl = v != 0 || !*s;
    else if (is("debug_stats")) c->debug_stats = v != 0 || !*s;
    else if (is("apply_group")) set_apply_group((uint32_t)v);
    else if (is("debug_alloc")) g_debug_alloc.store(v != 0 || !*s, std::memory_order_relaxed);
    else if (is("poison_cache")) g_poison_cache.store(v != 0 || !*s, std::memory_order_relaxed);
    else if (is("no_direct")) c->no_direct = v != 0 || !*s;
    else if (is("dense_min")) c->dense_min = *s ? (uint32_t)strtoul(s, nullptr, 0) : 64u;
    else if (is("flush_gran")) {
        if (!*s) c->flush_gran = 0;
        else if (v == 16 || v == 64) c->flush_gran = (uint32_t)v;
        else return fail(LIME_ERR_ARG, "flush_gran: want 16 or 64");
    }
    else if (is("io_threads")) c->io_threads = v >= 1 ? (v > 64 ? 64 : (int)v) : 0;
    else return fail(LIME_ERR_ARG, "lime_set_option: unknown option \"%s\"", key);
    return LIME_OK;
}
extern "C" int lime_set_option(lime_ctx *c, const char *key, const char *value)
{
    if (!c) return fail(LIME_ERR_ARG, "lime_set_option: ctx is NULL");
    return set_option(c, key, value);
}

extern "C" int lime_init(int device, lime_ctx **out)
{
    if (!out) return fail(LIME_ERR_ARG, "lime_init: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(LIME_ERR_HIP, "lime_init: no HIP device (%s); this library has no CPU path",
                    e == hipSuccess ? "count 0" : hipGetErrorString(e));
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    lime_ctx *c = new (std::nothrow) lime_ctx();
    if (!c) return fail(LIME_ERR_NOMEM, "lime_init: out of host memory");
    std::unique_ptr<lime_ctx, void (*)(lime_ctx *)> guard(c, lime_shutdown);      // every failure below releases the ctx and what it holds by then
    int rc;
    HIP_TRY(hipGetDevice(&c->device));
    if ((rc = c->stats.alloc(sizeof(DevStats) + 16))) return rc;
    c->d_sticky = reinterpret_cast<uint32_t *>(c->stats.p + 1);
    if ((rc = c->total.alloc(sizeof(unsigned long long)))) return rc;
    HIP_TRY(hipMemset(c->stats.p, 0, sizeof(DevStats) + 16));
    HIP_TRY(hipHostMalloc(&c->h_stats, sizeof(lime_stats_t) + 16));
    launch_preload();
#ifdef LIME_ABLATE_BUILD
    if (const char *s = getenv("LIME_ABLATE")) c->ablate = atoi(s);
#endif
    // The environment is read HERE and nowhere else, and only two kinds of variable: LIME_IO_THREADS (a resource limit the user sets, like the
    // reference's `threads` argument) always; the tuning / test knobs of lime_set_option only when LIME_TEST_HOOKS=1 says that this process is a
    // test or an experiment (tests/conftest.py sets it; bench.py refuses to run with it).  A release run takes no hidden switch.
    if (const char *s = getenv("LIME_IO_THREADS")) (void)set_option(c, "io_threads", s);
    if (const char *h = getenv("LIME_TEST_HOOKS")) if (atoi(h) != 0) {
        g_poison_cache.store(true, std::memory_order_relaxed);
        static const char *const hooks[][2] = {
            {"LIME_UPDATE_PATH", "update_path"}, {"LIME_BIN_LEVELS", "bin_levels"}, {"LIME_POOL_DENSITY", "pool_density"}, {"LIME_SCAN_STATIC_PCT", "scan_static_pct"},
            {"LIME_SECOND_LEVEL", "second_level"}, {"LIME_PART_SPLIT", "part_split"}, {"LIME_POOL_SLACK", "pool_slack"}, {"LIME_NO_PROBE", "no_probe"},
            {"LIME_PROBE_MIN", "probe_min"}, {"LIME_FORCE_P64", "force_p64"}, {"LIME_P64_TEST_BASE", "p64_test_base"}, {"LIME_MAX_BLOCKS", "max_blocks"},
            {"LIME_CHOOSE_FREE", "choose_free"}, {"LIME_APPLY_WIDE", "apply_wide"}, {"LIME_SORT_NT", "sort_nt"}, {"LIME_PART_LINES", "part_lines"},
            {"LIME_NO_STAGING", "no_staging"}, {"LIME_FORCE_STAGING", "force_staging"}, {"LIME_DETECT_CHUNK", "detect_chunk"}, {"LIME_SCORE_CHUNK", "score_chunk"},
            {"LIME_FORCE_RCCL", "force_rccl"}, {"LIME_DENSE_MIN", "dense_min"}, {"LIME_NO_DIRECT", "no_direct"}, {"LIME_FLUSH_GRAN", "flush_gran"}, {"LIME_DEBUG_STATS", "debug_stats"}, {"LIME_DEBUG_ALLOC", "debug_alloc"}, {"LIME_APPLY_GROUP", "apply_group"}};
        for (const auto &hk : hooks)
            if (const char *s = getenv(hk[0])) {
                if ((rc = set_option(c, hk[1], s))) return fail(rc, "lime_init: %s=%s: %s", hk[0], s, g_err.c_str());
            }
    }
    *out = guard.release();
    return LIME_OK;
}

extern "C" void lime_shutdown(lime_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    if (c->h_stats) (void)hipHostFree(c->h_stats);
    if (c->h_choose) (void)hipHostFree(c->h_choose);
    if (c->h_xoff) (void)hipHostFree(c->h_xoff);
    if (c->ev_xoff) (void)hipEventDestroy(c->ev_xoff);
    for (lime_lists *L : c->lists) delete L;
    for (lime_gindex *g : c->gidx) delete g;
    for (lime_seq_reader *r : c->readers) delete r;
    for (lime_docs *d : c->docs) delete d;
    delete c;                                            // (the device buffers go with their owners: DevArr / DevWords, lime_ctx.h)
}

int lime_host::flags_to_rc(uint32_t flags)
{
    if (flags & LIME_FLAG_INTERNAL) return fail(LIME_ERR_HIP, "the scan's window hand-out failed (a wave lost its chunk): the pass is invalid");
    if (flags & LIME_FLAG_BADCLUSTER) return fail(LIME_ERR_ARG, "a cluster record lies outside the arrays");
    if (flags & LIME_FLAG_OVERFLOW) return fail(LIME_ERR_NOMEM, "internal cluster list overflow");
    if (flags & LIME_FLAG_POOL_FULL) return fail(LIME_ERR_NOMEM, "update record pool too small (the pass could not be repeated)");
    if (flags & LIME_FLAG_MAXLEN) return fail(LIME_ERR_MAXLEN, "maximum cluster size is greater than %u (sizeMaxBuf)", LIME_MAX_CLUSTER);
    if (flags & LIME_FLAG_HALO) return fail(LIME_ERR_HALO, "a run owned by this shard does not close inside its halo");
    if (flags & LIME_FLAG_DOCID) return fail(LIME_ERR_DOCID, "a da value >= n_reads + n_refs was met while scoring");
    return LIME_OK;
}

extern "C" int lime_set_timing(lime_ctx *c, int on)
{
    int rc = check_ctx(c, "lime_set_timing"); if (rc) return rc;
    c->timing = on != 0; c->ev_used = 0;
    return LIME_OK;
}

int lime_host::timing_mark(lime_ctx *c, hipStream_t st)
{
    if (!c->timing) return LIME_OK;
    if (c->ev_used == c->ev.size()) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); c->ev.push_back(e); }
    HIP_TRY(hipEventRecord(c->ev[c->ev_used++], st));
    return LIME_OK;
}

extern "C" int lime_get_timing_ex(lime_ctx *c, double ms_avg[4], uint64_t *launches)
{
    int rc = check_ctx(c, "lime_get_timing_ex"); if (rc) return rc;
    double sum[4] = {0, 0, 0, 0}; uint64_t n = 0;
    for (size_t i = 0; i + 3 < c->ev_used; i += 4) {
        HIP_TRY(hipEventSynchronize(c->ev[i + 3]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[i + 1], c->ev[i + 2])); sum[0] += ms;     // the scan kernel
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 3])); sum[1] += ms;         // the whole pass
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[i + 2], c->ev[i + 3])); sum[2] += ms;     // after the scan
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1])); sum[3] += ms;         // before the scan (table clear)
        ++n;
    }
    c->ev_used = 0;
    if (ms_avg) for (int k = 0; k < 4; ++k) ms_avg[k] = n ? sum[k] / (double)n : 0.0;
    if (launches) *launches = n;
    return LIME_OK;
}

extern "C" int lime_get_host_times(lime_ctx *c, double out[8])
{
    int rc = check_ctx(c, "lime_get_host_times"); if (rc) return rc;
    if (!out) return fail(LIME_ERR_ARG, "lime_get_host_times: out is NULL");
    out[0] = c->alloc_ms; out[1] = c->probe_ms; out[2] = (double)c->n_probes; out[3] = (double)c->n_repeats; out[4] = (double)c->n_fallbacks;
    out[5] = c->density_known ? c->density : -1.0;
    out[6] = (double)c->n_table_free; out[7] = c->cls_ms;
    return LIME_OK;
}

extern "C" int lime_get_timing(lime_ctx *c, double *scan_ms_avg, uint64_t *launches)
{
    double ms[4];
    int rc = lime_get_timing_ex(c, ms, launches);
    if (!rc && scan_ms_avg) *scan_ms_avg = ms[0];
    return rc;
}

int lime_host::read_stats(lime_ctx *c, lime_stats_t *s, hipStream_t st, uint32_t *sticky)
{
    struct H { lime_stats_t s; uint32_t sticky[4]; };
    H *h = static_cast<H *>(c->h_stats);
    HIP_TRY(hipMemcpyAsync(h, c->stats.p, sizeof(lime_stats_t) + 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *s = h->s;
    if (sticky) *sticky = h->sticky[0];
    return LIME_OK;
}

extern "C" int lime_get_stats(lime_ctx *c, lime_stats_t *out, void *stream)
{
    int rc = check_ctx(c, "lime_get_stats"); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    lime_stats_t s;
    uint32_t unsettled = 0;
    if ((rc = read_stats(c, &s, st, &unsettled))) return rc;
    if (c->debug_stats) fprintf(stderr, "lime_get_stats: flags %u unsettled %u wave_records_max %u n_updates %llu\n", s.flags, unsettled, s.wave_records_max, (unsigned long long)s.n_updates);
    // A pass EARLIER than the last one overflowed its record pool and no lime_get_stats came before the next pass
    // (every pass clears the flags; the sticky word survives): that pass's table is short and cannot be repaired now.
    if (unsettled > ((s.flags & LIME_FLAG_POOL_FULL) ? 1u : 0u)) {
        HIP_TRY(hipMemsetAsync(c->d_sticky, 0, 4, st));
        if (out) *out = s;
        return fail(LIME_ERR_NOMEM, "an earlier lime_fused_dev pass on this ctx overflowed its update record pool and was followed by another "
                                    "pass before lime_get_stats: that pass's table is incomplete (call lime_get_stats after every pass)");
    }
    if (unsettled) HIP_TRY(hipMemsetAsync(c->d_sticky, 0, 4, st));
    // binned table updates: the record pool was too small for this pass -> the table is incomplete.  The pass
    // told how many records its busiest wave produced: repeat it with a pool sized for that (the caller's arrays
    // are still in place: nothing was reported to it yet), at most twice; then on the compare-and-swap path.
    lime_ctx::Last &l = c->last;
    for (int attempt = 0; (s.flags & LIME_FLAG_POOL_FULL) && l.valid && l.binned && attempt < 3; ++attempt) {
        const int pref = c->upd_pref;
        if (attempt == 2 && !l.records_only) c->upd_pref = 0;
        // (wave_records_max is the fullest SUB-REGION's count, sized for `share` of its wave's records)
        const double need = (double)s.wave_records_max * (double)l.n_waves / (double)(l.n_own ? l.n_own : 1) / (l.share > 0.0 ? l.share : 1.0);
        ++c->n_repeats;
        const double was = sizing_density(c);
        c->pool_density = need * 1.08 > was * 1.5 ? need * 1.08 : was * 1.5; c->pool_density_fixed = true;
        const bool timing = c->timing; c->timing = false;
        rc = fused_dev_impl(c, l.lcp, l.da, l.ebwt, l.n_own, l.n_avail, l.eof, l.n_reads, l.n_refs, l.alpha, l.sim, l.zero_sim,
                            false, l.st, nullptr, false, l.records_only);
        c->timing = timing; c->upd_pref = pref;
        if (rc) return rc;
        if ((rc = read_stats(c, &s, l.st, &unsettled))) return rc;
        if (unsettled) HIP_TRY(hipMemsetAsync(c->d_sticky, 0, 4, l.st));        // settled here (or reported through the flags below)
    }
    // records for an owner-partitioned exchange: the long clusters' updates (one 8-byte record per read x genome pair of every
    // cluster beyond the in-scan limit: a single cluster of 8 k symbols can make 16 million) did not fit their list -- treated
    // like the pool: the count went on past the capacity, so the list is regrown to it and the pass repeated
    if (l.valid && l.records_only && (s.flags & LIME_FLAG_OVERFLOW) && c->bigrec_n.p) {
        uint32_t nb = 0;
        HIP_TRY(hipMemcpyAsync(&nb, c->bigrec_n.p, sizeof nb, hipMemcpyDeviceToHost, l.st));
        HIP_TRY(hipStreamSynchronize(l.st));
        if (nb > c->bigrec.cap) {
            const uint64_t want = (uint64_t)nb + nb / 8u + 4096u;
            if (want > 0xFFFFFFF0ull) return fail(LIME_ERR_NOMEM, "%u update records of long clusters: too many for one shard's list", nb);
            DevArr<uint64_t> bigger;                      // (the new block first: if it cannot be had the ctx keeps its list)
            if ((rc = bigger.acquire((size_t)want))) return rc;
            c->bigrec.swap(bigger);
            bigger.release();                             // (the old block goes before the pass is repeated)
            const bool timing = c->timing; c->timing = false;
            rc = fused_dev_impl(c, l.lcp, l.da, l.ebwt, l.n_own, l.n_avail, l.eof, l.n_reads, l.n_refs, l.alpha, l.sim, l.zero_sim,
                                false, l.st, nullptr, false, true);
            c->timing = timing;
            if (rc) return rc;
            if ((rc = read_stats(c, &s, l.st, &unsettled))) return rc;
            if (unsettled) HIP_TRY(hipMemsetAsync(c->d_sticky, 0, 4, l.st));
        }
    }
    if (l.valid && l.own_total) { c->density = (double)s.n_updates / (double)l.own_total; c->density_known = true; }
    if (l.valid && l.fell_back) s.flags |= LIME_FLAG_CAS_FALLBACK;
    if (out) *out = s;
    if (c->big.cap && s.n_big > c->big.cap)
        return fail(LIME_ERR_NOMEM, "more clusters longer than %u symbols (%u) than the list holds (%u)", SMALL_MAX, s.n_big, (uint32_t)c->big.cap);
    if ((rc = flags_to_rc(s.flags))) return rc;
    if (s.edge & LIME_EDGE_OPEN)
        return fail(LIME_ERR_HALO, "a run owned by this shard is still open where its arrays end: whether it is a cluster is decided by "
                                   "the shards' edge words together (lime_combine_edges)");
    return LIME_OK;
}

extern "C" int lime_combine_edges(const uint32_t *edge, uint32_t n_shards)
{
    if (n_shards && !edge) return fail(LIME_ERR_ARG, "lime_combine_edges: edge is NULL");
    bool open = false, r = false, g = false;
    for (uint32_t k = 0; k < n_shards; ++k) {
        const uint32_t e = edge[k];
        if (open) {                                        // the run goes on through this shard's leading positions
            r = r || (e & LIME_EDGE_LEAD_R); g = g || (e & LIME_EDGE_LEAD_G);
            if ((e & LIME_EDGE_LEAD_HEAD) || k + 1 == n_shards) {          // closed by a head, or by the end of the collection
                if (r && g) return fail(LIME_ERR_MAXLEN, "maximum cluster size is greater than %u (sizeMaxBuf): a cluster crosses shard borders", LIME_MAX_CLUSTER);
                open = false;
            }
        }
        if (e & LIME_EDGE_OPEN) { open = true; r = (e & LIME_EDGE_OPEN_R) != 0; g = (e & LIME_EDGE_OPEN_G) != 0; }
    }
    return LIME_OK;
}

#ifdef LIME_DEBUG_CNT
// debug builds only: the per-window counts of accepted clusters the last scan left (see k_scan)
extern "C" int lime_debug_tile_counts(lime_ctx *c, uint32_t *out, uint32_t n)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, c->tile_cnt.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return LIME_OK;
}
#endif

// ---- pure host helpers ------------------------------------------------------------------
extern "C" uint8_t lime_sym_index(uint8_t b) { return (uint8_t)sym_index(b); }

extern "C" uint8_t lime_pair_score(const uint8_t cr[16], const uint8_t cg[16])
{
    uint32_t r[4] = {0, 0, 0, 0}, g[4] = {0, 0, 0, 0};
    for (int i = 0; i < 16; ++i) { r[i >> 2] |= (uint32_t)cr[i] << ((i & 3) * 8); g[i >> 2] |= (uint32_t)cg[i] << ((i & 3) * 8); }
    return (uint8_t)pair_score(r, g);
}

// The update records' arithmetic (lime_device.h) and the layout a table of n_reads x n_refs gets, without a device:
// what the scan stores for a scored pair and where the partition kernels put it.
extern "C" int lime_rec_layout(uint32_t n_reads, uint32_t n_refs, uint32_t one_level, uint32_t two_level, lime_rec_layout_t *out)
{
    if (!n_reads || !n_refs || !out) return fail(LIME_ERR_ARG, "lime_rec_layout: bad argument");
    const size_t sim_bytes = lime_sim_bytes(n_reads, n_refs);
    if (sim_bytes > ((size_t)BIN_MAX << BIN_SHIFT_MAX) || sim_bytes >= (1ull << CELL_BITS) || sim_bytes > ((uint64_t)MAX_SUB << 32))
        return fail(LIME_ERR_ARG, "lime_rec_layout: table too large for update records");
    const bool forced = one_level && two_level;                       // as LIME_BIN_LEVELS="a,b"
    bin_layout_of(forced ? one_level : BIN_ONE_LEVEL, forced ? two_level : BIN_TWO_LEVEL, forced, sim_bytes, &out->n_bins, &out->bin_shift);
    sub_layout(sim_bytes, n_refs, &out->n_sub, &out->sub_rb, &out->sub_gb);
    return LIME_OK;
}
extern "C" int lime_rec_valid(uint32_t gd, uint32_t n_refs) { return genome_ok(gd, n_refs) ? 1 : 0; }
extern "C" uint32_t lime_rec_of(uint32_t rd, uint32_t gd, uint32_t n_refs) { return rec_of(rd, gd, n_refs); }
extern "C" uint32_t lime_rec_sub2(uint32_t rd, uint32_t gd, uint32_t sub_rb, uint32_t sub_gb) { return rec_sub2(rd, gd, sub_rb, sub_gb); }
extern "C" uint32_t lime_rec_bin(uint32_t rec, uint32_t sub, uint32_t bin_shift) { return rec_bin(rec, sub, bin_shift); }
extern "C" void lime_scan_queue(lime_scan_queue_t *out)
{
    if (out) { out->cap = QCAP_SCAN; out->cap_short = QCAP_SCAN_SHORT; out->room_left = ROOM_LEFT; out->top_left = FLUSH_GRAN - 1u; }
}
// What the scan stores for each pair (read rd[i], genome index gd[i]) and where the partition kernels put it: valid[i] = genome_ok;
// stored[i] = 0: nothing (the pass ends in LIME_ERR_DOCID), else rec[i] / sub[i] = the record and its sub-region, bin[i] = rec_bin of them.
// `fixed_slot`: the pair's slot was given out before its id was looked at (score_small3, one sub-region): a bad id leaves the stand-in.
extern "C" int lime_rec_batch(const uint32_t *rd, const uint32_t *gd, uint64_t n, uint32_t n_refs, const lime_rec_layout_t *lay, int fixed_slot,
                              uint8_t *valid, uint8_t *stored, uint32_t *rec, uint32_t *sub, uint32_t *bin)
{
    if (!lay || !n_refs || (n && (!rd || !gd || !valid || !stored || !rec || !sub || !bin))) return fail(LIME_ERR_ARG, "lime_rec_batch: bad argument");
    for (uint64_t i = 0; i < n; ++i) {
        valid[i] = genome_ok(gd[i], n_refs);
        stored[i] = rec_stored(rd[i], gd[i], n_refs, lay->n_sub, lay->sub_rb, lay->sub_gb, fixed_slot != 0, rec[i], sub[i]);
        bin[i] = rec_bin(rec[i], sub[i], lay->bin_shift);
    }
    return LIME_OK;
}
