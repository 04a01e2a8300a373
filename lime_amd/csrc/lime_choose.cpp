// lime_choose.cpp -- clusterChoose and what follows it: the ctx's choose scratch, the lists objects left in HBM (lime_lists), the fused
// scan + choose with and without the table, the lists of genome shards made into one (lime_lists_concat_dev), Classify on the device and the taxonomy's device copy, and the calls that score a host
// cluster list and choose in one go (lime_score_choose, on several GPUs lime_score_choose_multi).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "lime_index.h"
#include "lime_classify.h"
#include "lime_ctx.h"

using namespace lime;
using namespace lime_host;

static int ensure_choose(lime_ctx *c, size_t dev_bytes, size_t host_bytes, hipStream_t st)
{
    int rc;
    if ((rc = c->choose.ensure(dev_bytes, st, nullptr))) return rc;
    if (host_bytes > c->h_choose_cap) {
        if (c->h_choose) { (void)hipHostFree(c->h_choose); c->h_choose = nullptr; c->h_choose_cap = 0; }
        HIP_TRY(hipHostMalloc(&c->h_choose, host_bytes));
        c->h_choose_cap = host_bytes;
    }
    return LIME_OK;
}
// the reference's test `float(max) / norm > beta`, in the reference's types (ClusterBWT_DA.cpp:404-406), once for each of the 256 values a row's
// maximum takes instead of once per read
static void choose_pass_table(uint32_t norm, float beta, bool pass[256])
{
    for (uint32_t v = 0; v < 256u; ++v) {
        const uint8_t mx = (uint8_t)v;
        const float top = static_cast<float>(mx) / norm;
        pass[v] = top > beta;
    }
}

// ---- clusterChoose results left in HBM (lime_lists) ---------------------------------------------------------------------
static void lists_release(lime_lists *L)
{
    if (!L) return;
    std::vector<lime_lists *> &v = L->ctx->lists;
    v.erase(std::remove(v.begin(), v.end(), L), v.end());
    delete L;
}
struct ListsGuard {                                      // releases a lists object on an error path
    lime_lists *L = nullptr;
    ~ListsGuard() { lists_release(L); }
    lime_lists *take() { lime_lists *r = L; L = nullptr; return r; }
};
// a lists object for rows whose offsets the host has made: the offsets (and, with_max, the maxima) are uploaded, the pairs' block is
// allocated for the caller's kernel to fill
static int lists_new(lime_ctx *c, uint32_t n_reads, uint32_t norm, float beta, const uint8_t *row_max, const uint64_t *row_off, bool with_max,
                     hipStream_t st, ListsGuard &g)
{
    lime_lists *L = new (std::nothrow) lime_lists();
    if (!L) return fail(LIME_ERR_NOMEM, "clusterChoose lists: out of host memory");
    L->ctx = c; L->n_reads = n_reads; L->norm = norm; L->beta = beta; L->n_pairs = row_off[n_reads];
    c->lists.push_back(L);
    g.L = L;
    const size_t off_bytes = ((size_t)n_reads + 1) * 8;
    int rc;
    if ((rc = L->rows.acquire(off_bytes + n_reads + 16))) return rc;
    if (L->n_pairs && (rc = L->pairs.acquire((size_t)L->n_pairs))) return rc;
    HIP_TRY(hipMemcpyAsync(L->rows.p, row_off, off_bytes, hipMemcpyHostToDevice, st));
    if (with_max && n_reads) HIP_TRY(hipMemcpyAsync(L->rows.p + off_bytes, row_max, n_reads, hipMemcpyHostToDevice, st));
    return LIME_OK;
}
// the pairs of a lists object into freshly allocated host memory (what the host-returning calls hand out)
static int lists_pairs_to_host(lime_ctx *c, const lime_lists *L, lime_pair_t **pairs, uint64_t *n_pairs, hipStream_t st)
{
    *pairs = nullptr; *n_pairs = L->n_pairs;
    if (!L->n_pairs) { HIP_TRY(hipStreamSynchronize(st)); return LIME_OK; }
    lime_pair_t *h = (lime_pair_t *)malloc((size_t)L->n_pairs * sizeof(lime_pair_t));
    if (!h) return fail(LIME_ERR_NOMEM, "clusterChoose lists: out of host memory");
    int rc = d2h_pageable(c, h, L->pairs.p, (size_t)L->n_pairs * sizeof(lime_pair_t), st);
    if (rc) { free(h); return rc; }
    *pairs = h;
    return LIME_OK;
}

// clusterChoose of a device table into a lists object; row_max / row_off (host, n_reads / n_reads + 1) receive the rows' maxima and offsets
static int choose_lists_impl(lime_ctx *c, const uint8_t *d_sim, uint32_t n_reads, uint32_t n_refs, uint32_t norm, float beta,
                             uint8_t *row_max, uint64_t *row_off, bool with_max, hipStream_t st, ListsGuard &g)
{
    int rc;
    row_off[0] = 0;
    if (!n_reads) return lists_new(c, 0, norm, beta, row_max, row_off, with_max, st, g);
    const size_t nz_off = ((size_t)n_reads + 15u) & ~(size_t)15u;      // row non-zero counts behind the row maxima, in both buffers
    if ((rc = ensure_choose(c, nz_off + (size_t)n_reads * 4, nz_off + (size_t)n_reads * 4, st))) return rc;
    launch_choose(d_sim, n_reads, n_refs, c->choose.p, reinterpret_cast<uint32_t *>(c->choose.p + nz_off), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_choose, c->choose.p, nz_off + (size_t)n_reads * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint8_t *hmx = static_cast<const uint8_t *>(c->h_choose);
    const uint32_t *nnz = reinterpret_cast<const uint32_t *>(hmx + nz_off);
    bool pass[256];
    choose_pass_table(norm, beta, pass);
    uint64_t total = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        const uint8_t mx = hmx[r];
        row_max[r] = mx;
        row_off[r] = total;
        if (pass[mx]) total += nnz[r];
    }
    row_off[n_reads] = total;
    if ((rc = lists_new(c, n_reads, norm, beta, row_max, row_off, with_max, st, g))) return rc;
    if (!total) return LIME_OK;
    launch_gather_pairs(d_sim, n_reads, n_refs, g.L->row_off(), g.L->pairs.p, st);
    HIP_TRY(hipGetLastError());
    return LIME_OK;
}

// clusterChoose on the device, compact results to the host: the lists, copied out
extern "C" int lime_choose_pairs_dev(lime_ctx *c, const uint8_t *d_sim, uint32_t n_reads, uint32_t n_refs,
                                     uint32_t norm, float beta, uint8_t *row_max, uint64_t *row_off,
                                     lime_pair_t **pairs, uint64_t *n_pairs, void *stream)
{
    int rc = check_ctx(c, "lime_choose_pairs_dev"); if (rc) return rc;
    if (norm == LIME_NORM_PER_READ) return fail(LIME_ERR_ARG, "lime_choose_pairs_dev: LIME_NORM_PER_READ is taken by the sample calls only (lime_classify_sample_*); this call needs one norm");
    if (!pairs || !n_pairs || !row_off || (n_reads && (!d_sim || !row_max)))
        return fail(LIME_ERR_ARG, "lime_choose_pairs_dev: NULL array");
    *pairs = nullptr; *n_pairs = 0; row_off[0] = 0;
    if (!n_reads) return LIME_OK;
    if (misaligned(d_sim, 16)) return fail(LIME_ERR_ARG, "lime_choose_pairs_dev: d_sim must be 16-byte aligned (and lime_sim_bytes() long)");
    hipStream_t st = (hipStream_t)stream;
    ListsGuard g;
    if ((rc = choose_lists_impl(c, d_sim, n_reads, n_refs, norm, beta, row_max, row_off, false, st, g))) return rc;
    return lists_pairs_to_host(c, g.L, pairs, n_pairs, st);
}

extern "C" int lime_choose_lists_dev(lime_ctx *c, const uint8_t *d_sim, uint32_t n_reads, uint32_t n_refs, uint32_t norm, float beta,
                                     lime_lists **out, void *stream)
{
    int rc = check_ctx(c, "lime_choose_lists_dev"); if (rc) return rc;
    if (norm == LIME_NORM_PER_READ) return fail(LIME_ERR_ARG, "lime_choose_lists_dev: LIME_NORM_PER_READ is taken by the sample calls only (lime_classify_sample_*); this call needs one norm");
    if (!out || (n_reads && !d_sim)) return fail(LIME_ERR_ARG, "lime_choose_lists_dev: NULL argument");
    *out = nullptr;
    if (misaligned(d_sim, 16)) return fail(LIME_ERR_ARG, "lime_choose_lists_dev: d_sim must be 16-byte aligned (and lime_sim_bytes() long)");
    hipStream_t st = (hipStream_t)stream;
    std::vector<uint8_t> mx((size_t)n_reads + 1);
    std::vector<uint64_t> off((size_t)n_reads + 1);
    ListsGuard g;
    if ((rc = choose_lists_impl(c, d_sim, n_reads, n_refs, norm, beta, mx.data(), off.data(), true, st, g))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    *out = g.take();
    return LIME_OK;
}

// ClusterLCP scan + clusterAnalyze + clusterChoose on device-resident arrays in one call.  Where the binned update path serves the pass with its
// second level by tiles (tables beyond 64 MB) the TABLE IS NEVER WRITTEN: the pass stops at the binned records (the long clusters' updates as
// records of their own, bucketed by region), k_sort_tiles sorts them into tile rows once, and k_apply_tiles builds every 64 KB region in LDS
// twice -- first for the rows' maxima and non-zero counts (clusterChoose's row scan, ClusterBWT_DA.cpp:385-402), then, after the host's test
// `float(max) / norm > beta` (:404-406), for the passing rows' (idRef, sim) lists (:408-423; regions without a passing row are skipped).  Against
// table + k_choose + k_gather_pairs that saves writing T bytes and reading them once or twice.  Elsewhere (small tables, short passes, n_refs < 256):
// the table is built and scanned as before.  Outputs as lime_choose_pairs_dev; *stats (may be NULL) as lime_get_stats.
static int fused_choose_lists_impl(lime_ctx *c, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt, uint64_t n,
                                   uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint32_t norm, float beta,
                                   uint8_t *row_max, uint64_t *row_off, bool with_max, lime_stats_t *stats, hipStream_t st, ListsGuard &g)
{
    int rc;
    void *stream = st;
    row_off[0] = 0;
    const size_t sim_bytes = lime_sim_bytes(n_reads, n_refs);
    const bool bin_fits = !(sim_bytes > ((size_t)BIN_MAX << BIN_SHIFT_MAX) || sim_bytes >= (1ull << CELL_BITS) || sim_bytes > ((uint64_t)MAX_SUB << 32));
    uint32_t n_bins = 0, bin_shift = REGION_SHIFT;
    if (bin_fits) bin_layout(c, sim_bytes, &n_bins, &bin_shift);
    // (lime_set_option "choose_free": 1 = without the table wherever the layout has a second level, 0 = never)
    bool table_free = bin_fits && c->by_tiles && bin_shift > REGION_SHIFT && n && c->upd_pref != 0 && n_refs < MAX_REFS &&
                      (c->choose_free >= 0 ? c->choose_free != 0 : (n_refs >= 256u && n >= (1u << 24)));
    lime_stats_t s;
    memset(&s, 0, sizeof s);
    if (!table_free) {
        DevBuf ds;
        if ((rc = ds.alloc(sim_bytes))) return rc;
        if ((rc = lime_fused_dev(c, d_lcp, d_da, d_ebwt, n, n, 1, n_reads, n_refs, alpha, (uint8_t *)ds.p, 1, stream))) return rc;
        rc = lime_get_stats(c, &s, stream);
        if (stats) *stats = s;
        if (rc) return rc;
        if (misaligned(ds.p, 16)) return fail(LIME_ERR_ARG, "lime_fused_choose_dev: misaligned table");
        if ((rc = choose_lists_impl(c, (const uint8_t *)ds.p, n_reads, n_refs, norm, beta, row_max, row_off, with_max, st, g))) return rc;
        HIP_TRY(hipStreamSynchronize(st));                  // (before the table goes)
        return LIME_OK;
    }
    ++c->n_table_free;
    if ((rc = fused_dev_impl(c, d_lcp, d_da, d_ebwt, n, n, 1, n_reads, n_refs, alpha, nullptr, 1, false, st, nullptr, false, true))) return rc;
    rc = lime_get_stats(c, &s, stream);                          // (waits; repeats the pass if the record pool or the long clusters' list was too small)
    if (stats) *stats = s;
    if (rc) return rc;
    uint32_t nb = 0;
    HIP_TRY(hipMemcpyAsync(&nb, c->bigrec_n.p, sizeof nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (nb > c->bigrec.cap) return fail(LIME_ERR_NOMEM, "more update records of long clusters (%u) than their list holds (%u)", nb, (uint32_t)c->bigrec.cap);
    const uint32_t n_regions = (uint32_t)((sim_bytes + ((size_t)1 << REGION_SHIFT) - 1) >> REGION_SHIFT);
    DevBuf bcnt, bcur, boff, bout;
    // the ctx's scratch: [region words 16 R][row max 4 n][row nnz 4 n][last nnz 4 R]; the rows' two arrays come back in one copy
    const size_t rows_off = (size_t)n_regions * 16, rows_bytes = (size_t)n_reads * 8, last_off = rows_off + rows_bytes;
    if ((rc = ensure_choose(c, last_off + (size_t)n_regions * 4, rows_bytes, st))) return rc;
    uint32_t *dmax = reinterpret_cast<uint32_t *>(c->choose.p + rows_off), *dnnz = dmax + n_reads;
    void *drr = c->choose.p;
    HIP_TRY(hipMemsetAsync(dmax, 0, rows_bytes, st));
    ApplyFin fin;
    memset(&fin, 0, sizeof fin);
    fin.n_refs = n_refs; fin.table_bytes = (uint64_t)n_reads * n_refs;
    fin.row_max = dmax; fin.row_nnz = dnnz; fin.last_nnz = reinterpret_cast<uint32_t *>(c->choose.p + last_off);
    fin.region_rows = (const uint4 *)drr;
    launch_region_rows(n_regions, n_refs, fin.table_bytes, nullptr, drr, st);
    if (nb) {
        if ((rc = bcnt.alloc((size_t)n_regions * 4)) || (rc = bcur.alloc((size_t)n_regions * 4)) || (rc = boff.alloc(((size_t)n_regions + 1) * 8)) ||
            (rc = bout.alloc((size_t)nb * 8))) return rc;
        launch_bigrec_buckets(c->bigrec.p, nb, n_regions, (uint32_t *)bcnt.p, (uint32_t *)bcur.p, (uint64_t *)boff.p, (uint64_t *)bout.p, st);
        fin.big_off = (const uint64_t *)boff.p; fin.bigrecs = (const uint64_t *)bout.p;
    }
    const double expect = (double)s.n_updates;
    uint16_t *rows = reinterpret_cast<uint16_t *>(c->pool.p);
    launch_sort_tiles(c->recs.p, c->binbase.p, n_bins, bin_shift, c->tbase.p, c->tidx.p, rows, st, big_rows_of(c, expect));      // (k_tile_bases inside: the pass stopped at the records and numbered no tiles)
    launch_apply_tiles_fin(1, sim_bytes, bin_shift, c->tbase.p, c->tidx.p, rows, many_records_of(c, expect), fin, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_choose, dmax, rows_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint32_t *hm = static_cast<const uint32_t *>(c->h_choose), *hz = hm + n_reads;
    bool pass[256];
    choose_pass_table(norm, beta, pass);                         // the reference's test, in the reference's types (ClusterBWT_DA.cpp:404-406)
    uint64_t total = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        const uint8_t mx = (uint8_t)hm[r];
        row_max[r] = mx;
        row_off[r] = total;
        if (pass[mx]) total += hz[r];
    }
    row_off[n_reads] = total;
    if ((rc = lists_new(c, n_reads, norm, beta, row_max, row_off, with_max, st, g))) return rc;
    if (total) {
        fin.row_off = g.L->row_off(); fin.pairs = g.L->pairs.p;
        launch_region_rows(n_regions, n_refs, fin.table_bytes, fin.row_off, drr, st);      // (now with the regions that have nothing to gather marked)
        launch_apply_tiles_fin(2, sim_bytes, bin_shift, c->tbase.p, c->tidx.p, rows, many_records_of(c, expect), fin, st);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));                      // (before the scratch of this call goes)
    return LIME_OK;
}

// scan + clusterAnalyze + clusterChoose, results on the host: the lists, copied out
extern "C" int lime_fused_choose_dev(lime_ctx *c, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt, uint64_t n,
                                     uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint32_t norm, float beta,
                                     uint8_t *row_max, uint64_t *row_off, lime_pair_t **pairs, uint64_t *n_pairs,
                                     lime_stats_t *stats, void *stream)
{
    int rc = check_ctx(c, "lime_fused_choose_dev"); if (rc) return rc;
    if (norm == LIME_NORM_PER_READ) return fail(LIME_ERR_ARG, "lime_fused_choose_dev: LIME_NORM_PER_READ is taken by the sample calls only (lime_classify_sample_*); this call needs one norm");
    if (!pairs || !n_pairs || !row_off || !row_max) return fail(LIME_ERR_ARG, "lime_fused_choose_dev: NULL output");
    if (!n_reads || !n_refs) return fail(LIME_ERR_ARG, "lime_fused_choose_dev: n_reads and n_refs must be > 0");
    *pairs = nullptr; *n_pairs = 0; row_off[0] = 0;
    hipStream_t st = (hipStream_t)stream;
    ListsGuard g;
    if ((rc = fused_choose_lists_impl(c, d_lcp, d_da, d_ebwt, n, n_reads, n_refs, alpha, norm, beta, row_max, row_off, false, stats, st, g))) return rc;
    return lists_pairs_to_host(c, g.L, pairs, n_pairs, st);
}

extern "C" int lime_fused_choose_lists_dev(lime_ctx *c, const uint32_t *d_lcp, const uint32_t *d_da, const uint8_t *d_ebwt, uint64_t n,
                                           uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint32_t norm, float beta, lime_lists **out,
                                           lime_stats_t *stats, void *stream)
{
    int rc = check_ctx(c, "lime_fused_choose_lists_dev"); if (rc) return rc;
    if (norm == LIME_NORM_PER_READ) return fail(LIME_ERR_ARG, "lime_fused_choose_lists_dev: LIME_NORM_PER_READ is taken by the sample calls only (lime_classify_sample_*); this call needs one norm");
    if (!out) return fail(LIME_ERR_ARG, "lime_fused_choose_lists_dev: NULL output");
    *out = nullptr;
    if (!n_reads || !n_refs) return fail(LIME_ERR_ARG, "lime_fused_choose_lists_dev: n_reads and n_refs must be > 0");
    std::vector<uint8_t> mx((size_t)n_reads + 1);
    std::vector<uint64_t> off((size_t)n_reads + 1);
    ListsGuard g;
    if ((rc = fused_choose_lists_impl(c, d_lcp, d_da, d_ebwt, n, n_reads, n_refs, alpha, norm, beta, mx.data(), off.data(), true, stats,
                                      (hipStream_t)stream, g))) return rc;
    *out = g.take();
    return LIME_OK;
}

extern "C" int lime_lists_info(const lime_lists *L, uint32_t *n_reads, uint64_t *n_pairs, uint32_t *norm, float *beta)
{
    if (!L) return fail(LIME_ERR_ARG, "lime_lists_info: lists is NULL");
    if (n_reads) *n_reads = L->n_reads;
    if (n_pairs) *n_pairs = L->n_pairs;
    if (norm) *norm = L->norm;
    if (beta) *beta = L->beta;
    return LIME_OK;
}

extern "C" int lime_lists_get(const lime_lists *L, uint8_t *row_max, uint64_t *row_off, lime_pair_t **pairs, uint64_t *n_pairs)
{
    if (!L) return fail(LIME_ERR_ARG, "lime_lists_get: lists is NULL");
    if (!row_off || !pairs || !n_pairs || (L->n_reads && !row_max)) return fail(LIME_ERR_ARG, "lime_lists_get: NULL output");
    int rc = check_ctx(L->ctx, "lime_lists_get"); if (rc) return rc;
    HIP_TRY(hipMemcpy(row_off, L->row_off(), ((size_t)L->n_reads + 1) * 8, hipMemcpyDeviceToHost));
    if (L->n_reads) HIP_TRY(hipMemcpy(row_max, L->row_max(), L->n_reads, hipMemcpyDeviceToHost));
    return lists_pairs_to_host(L->ctx, L, pairs, n_pairs, nullptr);
}

extern "C" void lime_lists_free(lime_lists *L)
{
    if (!L) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(L->ctx->device);
    lists_release(L);
    (void)hipSetDevice(cur);
}

// ---- lists of column shards of one table made into the whole table's list (lime_listcat_kernel.hip) ------------------------------
// A table column depends on its genome and the reads alone, so the lists of genome shards, each made with a
// test every non-zero row passes, hold the whole table's non-zero cells; clusterChoose's test is applied here once, on the maximum over
// the parts.  Passes: k_lc_rows (maxima and lengths), one 64-bit prefix sum, the total (8 bytes) to the host, k_lc_copy.
// d_norms == NULL: lime_lists_concat_dev, one norm (the parts').  Else lime_lists_concat_norms_dev: the test by pass[norm[r]][max] (k_rn_rows,
// lime_readnorm_kernel.hip), and *out owns a copy of the norms
static int lists_concat_impl(const char *who, lime_ctx *c, uint32_t n_parts, const lime_lists *const *parts, const uint32_t *id_base,
                             const uint32_t *n_refs_part, const uint8_t *d_norms, bool per_read, float beta, lime_lists **out, void *stream)
{
    if (!c) return fail(LIME_ERR_ARG, "%s: ctx is NULL", who);
    if (!out) return fail(LIME_ERR_ARG, "%s: NULL output", who);
    *out = nullptr;
    if (!n_parts) return fail(LIME_ERR_ARG, "%s: n_parts is 0", who);
    if (!parts || !id_base || !n_refs_part) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    for (uint32_t p = 0; p < n_parts; ++p) {
        if (!parts[p]) return fail(LIME_ERR_ARG, "%s: part %u is NULL", who, p);
        if (parts[p]->ctx != c) return fail(LIME_ERR_ARG, "%s: part %u belongs to another context", who, p);
        if (parts[p]->n_reads != parts[0]->n_reads)
            return fail(LIME_ERR_ARG, "%s: the parts hold different numbers of reads (%u in part 0, %u in part %u)", who, parts[0]->n_reads, parts[p]->n_reads, p);
        if (parts[p]->norm != parts[0]->norm)
            return fail(LIME_ERR_ARG, "%s: the parts were made with different norms (%u in part 0, %u in part %u)", who, parts[0]->norm, parts[p]->norm, p);
        if (p && (uint64_t)id_base[p] < (uint64_t)id_base[p - 1] + n_refs_part[p - 1])
            return fail(LIME_ERR_ARG, "%s: id_base must ascend: part %u starts at genome %u, part %u ends at %llu", who, p, id_base[p], p - 1,
                        (unsigned long long)id_base[p - 1] + n_refs_part[p - 1]);
        if ((uint64_t)id_base[p] + n_refs_part[p] > 0xFFFFFFFFull)
            return fail(LIME_ERR_ARG, "%s: part %u: genome ids from %u on for %u genomes pass 2^32 - 1", who, p, id_base[p], n_refs_part[p]);
        if (!per_read && parts[p]->per_read())
            return fail(LIME_ERR_ARG, "%s: part %u holds a norm per read (lime_lists_concat_norms_dev takes such parts)", who, p);
    }
    if (per_read && parts[0]->n_reads && !d_norms) return fail(LIME_ERR_ARG, "%s: d_norms is NULL", who);
    int rc = check_ctx(c, who); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_reads = parts[0]->n_reads;
    const size_t off_bytes = ((size_t)n_reads + 1) * 8;

    ListsGuard g;
    lime_lists *L = new (std::nothrow) lime_lists();
    if (!L) return fail(LIME_ERR_NOMEM, "%s: out of host memory", who);
    L->ctx = c; L->n_reads = n_reads; L->norm = per_read ? 0u : parts[0]->norm; L->beta = beta;
    c->lists.push_back(L);
    g.L = L;
    if ((rc = L->rows.acquire(off_bytes + n_reads + 16))) return rc;
    if (per_read) {
        if ((rc = L->norms.acquire((size_t)n_reads + 16))) return rc;
        if (n_reads) HIP_TRY(hipMemcpyAsync(L->norms.p, d_norms, n_reads, hipMemcpyDeviceToDevice, st));
    }
    const size_t pass_bytes = per_read ? 65536 : 256;

    // scratch: the parts' table, the pass table, the rows' lengths, rocPRIM's
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t tab_bytes = up((size_t)n_parts * sizeof(LcPart));
    size_t tmp_bytes = 0;
    HIP_TRY(idx_scan_sum64(nullptr, &tmp_bytes, nullptr, nullptr, (size_t)n_reads + 1, st));
    DevBuf scratch;
    if ((rc = scratch.alloc(tab_bytes + pass_bytes + up(off_bytes) + up(tmp_bytes))))
        return fail(rc, "%s: no device memory for %u parts of %u reads: %s", who, n_parts, n_reads, lime_last_error());
    uint8_t *at = static_cast<uint8_t *>(scratch.p);
    LcPart *d_parts = reinterpret_cast<LcPart *>(at);
    uint8_t *d_pass = at + tab_bytes;
    uint64_t *d_len = reinterpret_cast<uint64_t *>(at + tab_bytes + pass_bytes);
    void *tmp = at + tab_bytes + pass_bytes + up(off_bytes);
    std::vector<uint8_t> h(tab_bytes + pass_bytes, 0);
    LcPart *hp = reinterpret_cast<LcPart *>(h.data());
    for (uint32_t p = 0; p < n_parts; ++p) {
        hp[p].row_off = parts[p]->row_off(); hp[p].row_max = parts[p]->row_max();
        hp[p].pairs = parts[p]->n_pairs ? parts[p]->pairs.p : nullptr;
        hp[p].id_base = id_base[p]; hp[p].pad = 0;
    }
    bool pass[256];
    if (!per_read) {
        choose_pass_table(L->norm, beta, pass);                 // the reference's test, in the reference's types (ClusterBWT_DA.cpp:404-406)
        for (int v = 0; v < 256; ++v) h[tab_bytes + v] = pass[v] ? 1 : 0;
    } else {
        for (uint32_t n = 1; n < 256u; ++n) {                   // the same expression once per norm a byte holds; row 0 stays all false
            choose_pass_table(n, beta, pass);
            for (int v = 0; v < 256; ++v) h[tab_bytes + n * 256u + v] = pass[v] ? 1 : 0;
        }
    }
    HIP_TRY(hipMemcpy(scratch.p, h.data(), h.size(), hipMemcpyHostToDevice));
    uint64_t *d_off = reinterpret_cast<uint64_t *>(L->rows.p);
    struct Events {                                             // timing on: the rows' pass, the prefix sum, the copy
        hipEvent_t e[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    if (c->timing) for (hipEvent_t &x : ev.e) HIP_TRY(hipEventCreate(&x));
    c->lc_info[0] = c->lc_info[1] = c->lc_info[2] = c->lc_info[3] = 0.0;
    if (c->timing) HIP_TRY(hipEventRecord(ev.e[0], st));
    if (per_read) launch_rn_rows(d_parts, n_parts, n_reads, L->norms.p, d_pass, L->rows.p + off_bytes, d_len, st);
    else launch_lc_rows(d_parts, n_parts, n_reads, d_pass, L->rows.p + off_bytes, d_len, st);
    HIP_TRY(hipGetLastError());
    if (c->timing) HIP_TRY(hipEventRecord(ev.e[1], st));
    HIP_TRY(idx_scan_sum64(tmp, &tmp_bytes, d_len, d_off, (size_t)n_reads + 1, st));
    if (c->timing) HIP_TRY(hipEventRecord(ev.e[2], st));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_off + n_reads, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                          // (the total sizes the pairs' block)
    L->n_pairs = total;
    if (total) {
        if ((rc = L->pairs.acquire((size_t)total))) return fail(rc, "%s: no device memory for %llu pairs: %s", who, (unsigned long long)total, lime_last_error());
        if (c->timing) HIP_TRY(hipEventRecord(ev.e[3], st));
        launch_lc_copy(d_parts, n_parts, n_reads, d_off, L->pairs.p, st);
        HIP_TRY(hipGetLastError());
        if (c->timing) HIP_TRY(hipEventRecord(ev.e[4], st));
        HIP_TRY(hipStreamSynchronize(st));                      // (the scratch goes back when this returns)
    }
    if (c->timing) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) c->lc_info[0] = ms;
        if (hipEventElapsedTime(&ms, ev.e[1], ev.e[2]) == hipSuccess) c->lc_info[1] = ms;
        if (total && hipEventElapsedTime(&ms, ev.e[3], ev.e[4]) == hipSuccess) c->lc_info[2] = ms;
    }
    c->lc_info[3] = (double)total;
    *out = g.take();
    return LIME_OK;
}

extern "C" int lime_lists_concat_dev(lime_ctx *c, uint32_t n_parts, const lime_lists *const *parts, const uint32_t *id_base,
                                     const uint32_t *n_refs_part, float beta, lime_lists **out, void *stream)
{
    return lists_concat_impl("lime_lists_concat_dev", c, n_parts, parts, id_base, n_refs_part, nullptr, false, beta, out, stream);
}

extern "C" int lime_lists_concat_norms_dev(lime_ctx *c, uint32_t n_parts, const lime_lists *const *parts, const uint32_t *id_base,
                                           const uint32_t *n_refs_part, const uint8_t *d_norms, float beta, lime_lists **out, void *stream)
{
    return lists_concat_impl("lime_lists_concat_norms_dev", c, n_parts, parts, id_base, n_refs_part, d_norms, true, beta, out, stream);
}

extern "C" int lime_lists_get_norms(const lime_lists *L, uint8_t *norms)
{
    if (!L) return fail(LIME_ERR_ARG, "lime_lists_get_norms: lists is NULL");
    if (!L->per_read()) return fail(LIME_ERR_ARG, "lime_lists_get_norms: the lists were made with one norm (%u)", L->norm);
    if (L->n_reads && !norms) return fail(LIME_ERR_ARG, "lime_lists_get_norms: NULL output");
    int rc = check_ctx(L->ctx, "lime_lists_get_norms"); if (rc) return rc;
    if (L->n_reads) HIP_TRY(hipMemcpy(norms, L->norms.p, L->n_reads, hipMemcpyDeviceToHost));
    return LIME_OK;
}

extern "C" int lime_get_concat_info(lime_ctx *c, double out[4])
{
    if (!c || !out) return fail(LIME_ERR_ARG, "lime_get_concat_info: NULL argument");
    for (int k = 0; k < 4; ++k) out[k] = c->lc_info[k];
    return LIME_OK;
}

// ---- Classify on the device over lists in HBM (lime_classify_kernel.hip) -------------------------------------------------
static std::mutex g_tax_mu;                              // a taxonomy's device copy is made on first use: contexts of several threads may share one
static void taxonomy_release_dev(lime_taxonomy *tx)
{
    if (!tx->d_tab) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(tx->dev);
    dev_release(tx->d_tab);
    (void)hipSetDevice(cur);
    tx->d_tab = nullptr; tx->dev = -1;
}

// The tables of a list with per-read norms: value_tables for the norms 1 .. 255 at one beta, float[256][2][256] (row 0: zeros, a norm no
// read has).  The .res.txt values (binary == 0) cost a print and a parse per entry, 65 280 of them, and a sample in batches asks for the same
// block per batch: the last few blocks are kept, process-wide.
static std::mutex g_normtab_mu;
static const std::vector<float> &norm_tables(float beta, int binary, std::vector<float> &own)
{
    struct Entry { float beta; int binary; std::vector<float> tab; };
    static std::vector<Entry> cache;
    uint32_t key = 0, kb = 0;
    memcpy(&key, &beta, 4);
    std::lock_guard<std::mutex> lock(g_normtab_mu);
    for (const Entry &e : cache) { memcpy(&kb, &e.beta, 4); if (kb == key && e.binary == (binary != 0)) { own = e.tab; return own; } }
    own.assign((size_t)256 * 512, 0.0f);
    for (uint32_t n = 1; n < 256u; ++n) lime_cls::value_tables(n, beta, binary, &own[(size_t)n * 512], &own[(size_t)n * 512 + 256]);
    if (cache.size() >= 4) cache.erase(cache.begin());
    cache.push_back(Entry{beta, binary != 0, own});
    return own;
}

extern "C" int lime_classify_lists_dev(lime_ctx *c, uint32_t n_lists, const lime_lists *const *lists, uint32_t n_targ,
                                       const lime_taxonomy *tx_in, int binary, lime_verdict_t *verdicts, uint64_t counts[4], void *stream)
{
    int rc = check_ctx(c, "lime_classify_lists_dev"); if (rc) return rc;
    uint64_t local[4];
    if (!counts) counts = local;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (n_lists != 2 && n_lists != 4)
        return fail(LIME_ERR_ARG, "lime_classify_lists_dev: n_lists is %u; the allowed number of lists is 2 (single-end reads) or 4 (paired-end reads)", n_lists);
    if (!lists || !tx_in) return fail(LIME_ERR_ARG, "lime_classify_lists_dev: NULL argument");
    for (uint32_t i = 0; i < n_lists; ++i) {
        if (!lists[i]) return fail(LIME_ERR_ARG, "lime_classify_lists_dev: list %u is NULL", i);
        if (lists[i]->ctx != c) return fail(LIME_ERR_ARG, "lime_classify_lists_dev: list %u belongs to another context", i);
        if (lists[i]->n_reads != lists[0]->n_reads)
            return fail(LIME_ERR_ARG, "lime_classify_lists_dev: the lists hold different numbers of reads (%u in list 0, %u in list %u)",
                        lists[0]->n_reads, lists[i]->n_reads, i);
    }
    if (!n_targ || tx_in->n_targ != n_targ)
        return fail(LIME_ERR_ARG, "lime_classify_lists_dev: the taxonomy holds %u genomes, numGenomes is %u", tx_in->n_targ, n_targ);
    const uint32_t n_reads = lists[0]->n_reads;
    if (!n_reads) return LIME_OK;
    if (!verdicts) return fail(LIME_ERR_ARG, "lime_classify_lists_dev: verdicts is NULL");
    hipStream_t st = (hipStream_t)stream;
    // the taxonomy's device copy, made once per device: at_rank[n_targ], then with HIGHER higher[6][n_targ]
    lime_taxonomy *tx = const_cast<lime_taxonomy *>(tx_in);
    std::lock_guard<std::mutex> tax_lock(g_tax_mu);           // (held for the call: a copy for another device replaces this one only after it)
    if (tx->d_tab && tx->dev != c->device) taxonomy_release_dev(tx);
    if (!tx->d_tab) {
        const size_t words = (size_t)n_targ * (tx->higher ? 7u : 1u);
        std::vector<uint32_t> h(words, 0u);
        std::copy(tx->host.at_rank.begin(), tx->host.at_rank.end(), h.begin());
        if (tx->higher)
            for (int q = 0; q < lime_cls::N_RANKS; ++q) std::copy(tx->host.higher[q].begin(), tx->host.higher[q].end(), h.begin() + (size_t)(q + 1) * n_targ);
        void *p = nullptr;
        HIP_TRY(dev_acquire(&p, words * 4));
        tx->d_tab = p; tx->dev = c->device; tx->release = taxonomy_release_dev;
        HIP_TRY(hipMemcpy(p, h.data(), words * 4, hipMemcpyHostToDevice));
    }
    // per list the 256 values the writer's expression gives a count (and the record tops), built here so that the device divides nothing
    bool per_read = false;
    for (uint32_t i = 0; i < n_lists; ++i) per_read = per_read || lists[i]->per_read();
    DevBuf dt, dv;
    size_t tab_bytes = 0;
    ClsNormArgs na;
    memset(&na, 0, sizeof na);
    ClsArgs &a = na.a;
    if (!per_read) {
        std::vector<float> tabs(4 * 2 * 256, 0.0f);
        for (uint32_t i = 0; i < n_lists; ++i) lime_cls::value_tables(lists[i]->norm, lists[i]->beta, binary, &tabs[i * 512], &tabs[i * 512 + 256]);
        tab_bytes = tabs.size() * 4;
        if ((rc = dt.alloc(tab_bytes + 16)) || (rc = dv.alloc((size_t)n_reads * sizeof(lime_verdict_t)))) return rc;
        HIP_TRY(hipMemcpy(dt.p, tabs.data(), tab_bytes, hipMemcpyHostToDevice));
    } else {
        // a block of 256 tables per distinct (per-read, beta) and per (norm, beta) of the lists with one norm, which read row 0 of theirs
        const size_t block_bytes = (size_t)256 * 512 * 4;
        uint32_t n_blocks = 0, of[4] = {0, 0, 0, 0};
        for (uint32_t i = 0; i < n_lists; ++i) {
            uint32_t j = 0;
            for (; j < i; ++j)
                if (lists[j]->per_read() == lists[i]->per_read() && lists[j]->norm == lists[i]->norm && memcmp(&lists[j]->beta, &lists[i]->beta, 4) == 0) break;
            of[i] = j < i ? of[j] : n_blocks++;
            na.block |= of[i] << (8u * i);
            na.norms[i] = lists[i]->per_read() ? lists[i]->norms.p : nullptr;
        }
        tab_bytes = block_bytes * n_blocks;
        if ((rc = dt.alloc(tab_bytes + 16)) || (rc = dv.alloc((size_t)n_reads * sizeof(lime_verdict_t)))) return rc;
        std::vector<float> own;
        for (uint32_t i = 0, done = 0; i < n_lists; ++i) {
            if (of[i] != done) continue;                      // (blocks are numbered in the order of their first list)
            ++done;
            uint8_t *dst = static_cast<uint8_t *>(dt.p) + block_bytes * of[i];
            if (lists[i]->per_read()) {
                const std::vector<float> &t = norm_tables(lists[i]->beta, binary, own);
                HIP_TRY(hipMemcpy(dst, t.data(), block_bytes, hipMemcpyHostToDevice));
            } else {
                float one[512];
                lime_cls::value_tables(lists[i]->norm, lists[i]->beta, binary, one, one + 256);
                HIP_TRY(hipMemcpy(dst, one, sizeof one, hipMemcpyHostToDevice));
            }
        }
    }
    uint32_t *d_err = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(dt.p) + tab_bytes);
    HIP_TRY(hipMemsetAsync(d_err, 0, 4, st));
    for (uint32_t i = 0; i < n_lists; ++i) { a.row_max[i] = lists[i]->row_max(); a.row_off[i] = lists[i]->row_off(); a.pairs[i] = lists[i]->pairs.p; }
    a.tabs = static_cast<const float *>(dt.p);
    a.at_rank = static_cast<const uint32_t *>(tx->d_tab);
    a.higher = tx->higher ? a.at_rank + n_targ : nullptr;
    a.n_lists = n_lists; a.n_reads = n_reads; a.n_targ = n_targ; a.rank_lo = tx->higher ? (uint32_t)(tx->rank - 1) : 6u;
    a.out = static_cast<lime_verdict_t *>(dv.p); a.err = d_err;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->timing) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventRecord(e0, st)); }
    if (per_read) launch_classify_norms(na, st); else launch_classify(a, st);
    HIP_TRY(hipGetLastError());
    if (c->timing) HIP_TRY(hipEventRecord(e1, st));
    uint32_t err = 0;
    rc = d2h_pageable(c, verdicts, dv.p, (size_t)n_reads * sizeof(lime_verdict_t), st);
    if (!rc && hipMemcpy(&err, d_err, 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(LIME_ERR_HIP, "lime_classify_lists_dev: reading the error word");
    if (c->timing) {
        float ms = 0.0f;
        if (!rc && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) c->cls_ms = ms;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    if (rc) return rc;
    if (err) return fail(LIME_ERR_ARG, "lime_classify_lists_dev: genome index beyond numGenomes (%u) in the lists", n_targ);
    for (uint32_t r = 0; r < n_reads; ++r)
        switch (verdicts[r].type) { case 'C': ++counts[0]; break; case 'U': ++counts[1]; break; case 'A': ++counts[2]; break; default: ++counts[3]; }
    return LIME_OK;
}

extern "C" int lime_score_choose(lime_ctx *c, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                                 const lime_cluster_t *clusters, uint64_t n_clusters, uint32_t n_reads,
                                 uint32_t n_refs, uint32_t norm, float beta, uint8_t *row_max, uint64_t *row_off,
                                 lime_pair_t **pairs, uint64_t *n_pairs, uint8_t *sim)
{
    int rc = check_ctx(c, "lime_score_choose"); if (rc) return rc;
    if (norm == LIME_NORM_PER_READ) return fail(LIME_ERR_ARG, "lime_score_choose: LIME_NORM_PER_READ is taken by the sample calls only (lime_classify_sample_*); this call needs one norm");
    if ((n && !da) || (n_clusters && !clusters)) return fail(LIME_ERR_ARG, "lime_score_choose: NULL array");
    if (!n_reads || !n_refs) return fail(LIME_ERR_ARG, "lime_score_choose: n_reads and n_refs must be > 0");
    DevBuf ds;
    if ((rc = ds.alloc(lime_sim_bytes(n_reads, n_refs)))) return rc;
    if ((rc = score_in_chunks(c, da, ebwt, n, clusters, n_clusters, n_reads, n_refs, (uint8_t *)ds.p))) return rc;
    if ((rc = lime_choose_pairs_dev(c, (const uint8_t *)ds.p, n_reads, n_refs, norm, beta, row_max, row_off, pairs,
                                    n_pairs, nullptr))) return rc;
    if (sim && (rc = d2h_pageable(c, sim, ds.p, (size_t)n_reads * n_refs, nullptr))) return rc;
    return LIME_OK;
}

// ---- clusterAnalyze + clusterChoose on several GPUs of one process ------------------------------------
// The cluster list is cut by position into n_dev parts of equal symbol counts (the reference cuts it by cluster
// count over OpenMP threads, ClusterBWT_DA.cpp:641-648; any cut gives the same table); device k scores its part
// into its own table; ONE reduce-scatter (RCCL, sum modulo 256) leaves device k with the block of read rows
// [k * rpd, (k+1) * rpd); each device runs the row scan and the list compaction on its block; the host appends
// the blocks' results in row order.  A host thread per device does the uploads and launches.

extern "C" int lime_score_choose_multi(int n_dev, const int *devices, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                                       const lime_cluster_t *clusters, uint64_t n_clusters, uint32_t n_reads, uint32_t n_refs,
                                       uint32_t norm, float beta, uint8_t *row_max, uint64_t *row_off, lime_pair_t **pairs,
                                       uint64_t *n_pairs)
{
    if (n_dev < 1 || !pairs || !n_pairs || !row_off || (n_reads && !row_max) || (n && !da) || (n_clusters && !clusters))
        return fail(LIME_ERR_ARG, "lime_score_choose_multi: bad argument");
    if (norm == LIME_NORM_PER_READ) return fail(LIME_ERR_ARG, "lime_score_choose_multi: LIME_NORM_PER_READ is taken by the sample calls only (lime_classify_sample_*); this call needs one norm");
    if (!n_reads || !n_refs) return fail(LIME_ERR_ARG, "lime_score_choose_multi: n_reads and n_refs must be > 0");
    if (n_dev > lime_device_count()) return fail(LIME_ERR_ARG, "lime_score_choose_multi: %d devices asked, %d visible", n_dev, lime_device_count());
    *pairs = nullptr; *n_pairs = 0; row_off[0] = 0;
    std::vector<int> devs(n_dev);
    for (int k = 0; k < n_dev; ++k) devs[k] = devices ? devices[k] : k;
    // row blocks: a multiple of 16 rows each, so that every block starts 16-byte aligned whatever n_refs is
    const uint64_t rpd = (((uint64_t)n_reads + n_dev - 1) / n_dev + 15u) & ~15ull;
    const size_t blk = (size_t)rpd * n_refs, tbl = blk * (size_t)n_dev;
    // the clusters in position order, cut where the running symbol count passes k/n_dev of the total
    std::vector<lime_cluster_t> order;
    const lime_cluster_t *cl = clusters;
    bool sorted = true;
    uint64_t total_len = 0;
    for (uint64_t i = 0; i < n_clusters; ++i) { if (i && clusters[i].pStart < clusters[i - 1].pStart) sorted = false; total_len += clusters[i].len; }
    if (!sorted) {
        order.assign(clusters, clusters + n_clusters);
        std::sort(order.begin(), order.end(), [](const lime_cluster_t &x, const lime_cluster_t &y) { return x.pStart < y.pStart; });
        cl = order.data();
    }
    std::vector<uint64_t> cut(n_dev + 1, n_clusters);
    cut[0] = 0;
    { uint64_t run = 0; int k = 1; for (uint64_t i = 0; i < n_clusters && k < n_dev; ++i) { run += cl[i].len; while (k < n_dev && run * (uint64_t)n_dev >= total_len * (uint64_t)k) cut[k++] = i + 1; } }
    struct Dev { lime_ctx *ctx = nullptr; uint8_t *sim = nullptr, *blkp = nullptr; int rc = LIME_OK; std::string err; };
    std::vector<Dev> dv(n_dev);
    auto cleanup = [&]() {
        for (int k = 0; k < n_dev; ++k) { (void)hipSetDevice(devs[k]); (void)hipFree(dv[k].sim); (void)hipFree(dv[k].blkp); if (dv[k].ctx) lime_shutdown(dv[k].ctx); }
    };
    std::vector<std::thread> th;
    for (int k = 0; k < n_dev; ++k)
        th.emplace_back([&, k]() {
            Dev &d = dv[k];
            auto bad = [&](int rc, const char *what) { d.rc = rc; d.err = std::string(what) + ": " + lime_last_error(); };
            if (hipSetDevice(devs[k]) != hipSuccess) { d.rc = LIME_ERR_HIP; d.err = "hipSetDevice"; return; }
            int rc = lime_init(devs[k], &d.ctx);
            if (rc) { bad(rc, "lime_init"); return; }
            if (hipMalloc(&d.sim, tbl + 16) != hipSuccess || hipMalloc(&d.blkp, blk + 16) != hipSuccess) { d.rc = LIME_ERR_NOMEM; d.err = "hipMalloc of the table"; return; }
            if (hipMemset(d.sim, 0, tbl + 16) != hipSuccess) { d.rc = LIME_ERR_HIP; d.err = "hipMemset"; return; }
            rc = score_in_chunks(d.ctx, da, ebwt, n, cl + cut[k], cut[k + 1] - cut[k], n_reads, n_refs, d.sim);
            if (rc) { bad(rc, "scoring"); return; }
            if (hipDeviceSynchronize() != hipSuccess) { d.rc = LIME_ERR_HIP; d.err = "hipDeviceSynchronize"; }
        });
    for (auto &t : th) t.join();
    for (int k = 0; k < n_dev; ++k) if (dv[k].rc) { const int rc = dv[k].rc; const std::string e = dv[k].err; cleanup(); return fail(rc, "device %d: %s", devs[k], e.c_str()); }
    int rc = LIME_OK;
    if (n_dev > 1 || dv[0].ctx->force_rccl) {
        std::vector<uint8_t *> sims(n_dev), blks(n_dev);
        for (int k = 0; k < n_dev; ++k) { sims[k] = dv[k].sim; blks[k] = dv[k].blkp; }
        if ((rc = lime_internal_reduce_scatter(n_dev, devs.data(), sims.data(), blks.data(), blk))) { cleanup(); return fail(rc, "%s", lime_comm_error()); }
    } else {
        (void)hipSetDevice(devs[0]);
        if (hipMemcpy(dv[0].blkp, dv[0].sim, blk, hipMemcpyDeviceToDevice) != hipSuccess) { cleanup(); return fail(LIME_ERR_HIP, "hipMemcpy"); }
    }
    // row scan + compaction per block, appended in row order
    std::vector<lime_pair_t *> pp(n_dev, nullptr);
    std::vector<uint64_t> np(n_dev, 0);
    std::vector<std::vector<uint64_t>> off(n_dev);
    uint64_t total = 0;
    for (int k = 0; k < n_dev && !rc; ++k) {
        const uint64_t r0 = rpd * (uint64_t)k;
        if (r0 >= n_reads) break;
        const uint32_t rows = (uint32_t)(n_reads - r0 < rpd ? n_reads - r0 : rpd);
        off[k].resize((size_t)rows + 2);
        (void)hipSetDevice(devs[k]);
        rc = lime_choose_pairs_dev(dv[k].ctx, dv[k].blkp, rows, n_refs, norm, beta, row_max + r0, off[k].data(), &pp[k], &np[k], nullptr);
        if (!rc) { for (uint32_t r = 0; r < rows; ++r) row_off[r0 + r] = total + off[k][r]; total += np[k]; }
    }
    std::string err = rc ? lime_last_error() : "";
    if (!rc) {
        row_off[n_reads] = total;
        lime_pair_t *all = total ? (lime_pair_t *)malloc((size_t)total * sizeof(lime_pair_t)) : nullptr;
        if (total && !all) { rc = LIME_ERR_NOMEM; err = "out of host memory"; }
        else {
            uint64_t at = 0;
            for (int k = 0; k < n_dev; ++k) if (np[k]) { memcpy(all + at, pp[k], (size_t)np[k] * sizeof(lime_pair_t)); at += np[k]; }
            *pairs = all; *n_pairs = total;
        }
    }
    for (int k = 0; k < n_dev; ++k) free(pp[k]);
    cleanup();
    return rc ? fail(rc, "%s", err.c_str()) : LIME_OK;
}

// lime_fused_choose_lists_dev from host arrays or mapped files (the drop-in LiME_paired): the arrays come in through the staging ring
extern "C" int lime_fused_choose_lists(lime_ctx *c, const uint32_t *lcp, const uint32_t *da, const uint8_t *ebwt, uint64_t n,
                                       uint32_t n_reads, uint32_t n_refs, uint32_t alpha, uint32_t norm, float beta, lime_lists **out,
                                       lime_stats_t *stats)
{
    int rc = check_ctx(c, "lime_fused_choose_lists"); if (rc) return rc;
    if (norm == LIME_NORM_PER_READ) return fail(LIME_ERR_ARG, "lime_fused_choose_lists: LIME_NORM_PER_READ is taken by the sample calls only (lime_classify_sample_*); this call needs one norm");
    if (!out || (n && (!lcp || !da))) return fail(LIME_ERR_ARG, "lime_fused_choose_lists: NULL argument");
    *out = nullptr;
    DevBuf dl, dd, de;
    if ((rc = dl.alloc(n * 4 + 16)) || (rc = dd.alloc(n * 4 + 16)) || (ebwt && (rc = de.alloc(n + 16)))) return rc;
    const void *src[3] = {lcp, da, ebwt};
    void *dst[3] = {dl.p, dd.p, de.p};
    const size_t bytes[3] = {(size_t)n * 4, (size_t)n * 4, (size_t)n};
    if ((rc = lime_internal_upload(ebwt ? 3 : 2, src, dst, bytes, nullptr))) return rc;
    return lime_fused_choose_lists_dev(c, (const uint32_t *)dl.p, (const uint32_t *)dd.p, ebwt ? (const uint8_t *)de.p : nullptr, n, n_reads,
                                       n_refs, alpha, norm, beta, out, stats, nullptr);
}
