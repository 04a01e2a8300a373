// lime_merge.cpp -- a genome collection's index that stays in HBM (lime_gindex: built by the index builder of lime_build.cpp, saved to and
// loaded from one file) and the merge of a read set into it (lime_merge_index_dev: the reads sorted alone, then the kernels of
// lime_merge_kernel.hip in order), with the host-array front ends.  include/lime_hip.h states the contract and the file's layout.
#include <hip/hip_runtime.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "lime_index.h"
#include "lime_ctx.h"

using namespace lime;
using namespace lime_host;

// ---- the handle ---------------------------------------------------------------------------------------------------------
static void gindex_release(lime_gindex *g)
{
    if (!g) return;
    std::vector<lime_gindex *> &v = g->ctx->gidx;
    v.erase(std::remove(v.begin(), v.end(), g), v.end());
    delete g;
}
namespace {
struct GindexGuard {                                     // releases a handle on an error path
    lime_gindex *g = nullptr;
    ~GindexGuard() { gindex_release(g); }
    lime_gindex *take() { lime_gindex *r = g; g = nullptr; return r; }
};
}

static int check_positions(const char *who, uint64_t n_text, uint32_t n_docs)
{
    if (n_text > 0xFFFFFFFFull || n_text + n_docs > 0xFFFFFFFFull)
        return fail(LIME_ERR_ARG, "%s: %llu symbols + %u terminators exceed 2^32 - 1 positions (one GPU, 32-bit suffix positions)", who,
                    (unsigned long long)n_text, n_docs);
    if (!n_docs && n_text) return fail(LIME_ERR_ARG, "%s: %llu symbols in no document", who, (unsigned long long)n_text);
    return LIME_OK;
}

// doc_off by lime_build_index's rules: starts at 0, never decreases (and, n_text known, ends there)
static int check_doc_off(const char *who, const uint64_t *doc_off, uint32_t n_docs, const uint64_t *n_text)
{
    if (!doc_off) return fail(LIME_ERR_ARG, "%s: doc_off is NULL", who);
    if (doc_off[0] != 0) return fail(LIME_ERR_ARG, "%s: doc_off[0] is %llu, not 0", who, (unsigned long long)doc_off[0]);
    for (uint32_t k = 0; k < n_docs; ++k)
        if (doc_off[k + 1] < doc_off[k]) return fail(LIME_ERR_ARG, "%s: doc_off decreases at document %u", who, k);
    if (n_text && doc_off[n_docs] != *n_text)
        return fail(LIME_ERR_ARG, "%s: doc_off ends at %llu, not at n_text (%llu)", who, (unsigned long long)doc_off[n_docs], (unsigned long long)*n_text);
    return LIME_OK;
}

// a handle with its block, nothing in it yet
static int gindex_new(lime_ctx *c, const char *who, uint32_t n_docs, uint64_t n_text, uint8_t term, uint32_t lcp_cap, GindexGuard &gg)
{
    lime_gindex *g = new (std::nothrow) lime_gindex();
    if (!g) return fail(LIME_ERR_NOMEM, "%s: out of host memory", who);
    g->ctx = c; g->n_docs = n_docs; g->n_text = n_text; g->term = term; g->lcp_cap = lcp_cap;
    c->gidx.push_back(g);
    gg.g = g;
    int rc = g->blk.acquire((size_t)g->body_bytes() + 16);
    if (rc) return fail(rc, "%s: no device memory for the index of %llu positions (14 bytes each): %s", who, (unsigned long long)g->n(), lime_last_error());
    return LIME_OK;
}

// the handle's text and doc_off are in place: sort, keeping the suffix array
static int gindex_sort(lime_gindex *g, const char *who, hipStream_t st)
{
    // the padding between the sections is written once, so that a saved file does not depend on what the block held before
    HIP_TRY(hipMemsetAsync(g->blk.p + g->off_sa(), 0, (size_t)(g->off_text() - g->off_sa()), st));
    HIP_TRY(hipMemsetAsync(g->blk.p + g->off_ebwt(), 0, (size_t)(g->body_bytes() - g->off_ebwt()), st));
    return build_index_impl(g->ctx, who, g->text(), g->doc_off(), g->n_docs, g->n_text, g->term, g->lcp_cap, g->ebwt(), g->lcp(), g->da(), g->sa(), st);
}

extern "C" int lime_gindex_build_dev(lime_ctx *c, const uint8_t *d_text, const uint64_t *d_doc_off, uint32_t n_docs, uint64_t n_text,
                                     uint8_t term, uint32_t lcp_cap, void *stream, lime_gindex **out)
{
    const char *who = "lime_gindex_build_dev";
    if (!c || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    int rc = check_positions(who, n_text, n_docs); if (rc) return rc;
    if (!d_doc_off || (n_text && !d_text)) return fail(LIME_ERR_ARG, "%s: NULL array", who);
    if ((rc = check_ctx(c, who))) return rc;
    hipStream_t st = (hipStream_t)stream;
    GindexGuard gg;
    if ((rc = gindex_new(c, who, n_docs, n_text, term, lcp_cap, gg))) return rc;
    lime_gindex *g = gg.g;
    HIP_TRY(hipMemsetAsync(g->blk.p + g->off_text(), 0, (size_t)(g->off_ebwt() - g->off_text()), st));
    HIP_TRY(hipMemsetAsync(g->blk.p, 0, (size_t)g->off_sa(), st));
    HIP_TRY(hipMemcpyAsync(g->doc_off(), d_doc_off, ((size_t)n_docs + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (n_text) HIP_TRY(hipMemcpyAsync(g->text(), d_text, (size_t)n_text, hipMemcpyDeviceToDevice, st));
    if ((rc = gindex_sort(g, who, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    *out = gg.take();
    return LIME_OK;
}

extern "C" int lime_gindex_build(lime_ctx *c, const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, uint8_t term, uint32_t lcp_cap,
                                 lime_gindex **out)
{
    const char *who = "lime_gindex_build";
    if (!c || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    int rc = check_doc_off(who, doc_off, n_docs, nullptr); if (rc) return rc;
    const uint64_t n_text = doc_off[n_docs];
    if ((rc = check_positions(who, n_text, n_docs))) return rc;
    if (n_text && !text) return fail(LIME_ERR_ARG, "%s: text is NULL", who);
    if ((rc = check_ctx(c, who))) return rc;
    GindexGuard gg;
    if ((rc = gindex_new(c, who, n_docs, n_text, term, lcp_cap, gg))) return rc;
    lime_gindex *g = gg.g;
    HIP_TRY(hipMemset(g->blk.p + g->off_text(), 0, (size_t)(g->off_ebwt() - g->off_text())));
    HIP_TRY(hipMemset(g->blk.p, 0, (size_t)g->off_sa()));
    HIP_TRY(hipMemcpy(g->doc_off(), doc_off, ((size_t)n_docs + 1) * 8, hipMemcpyHostToDevice));
    if (n_text) HIP_TRY(hipMemcpy(g->text(), text, (size_t)n_text, hipMemcpyHostToDevice));
    if ((rc = gindex_sort(g, who, nullptr))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    *out = gg.take();
    return LIME_OK;
}

extern "C" int lime_gindex_info(const lime_gindex *g, uint32_t *n_docs, uint64_t *n_text, uint32_t *lcp_cap, uint8_t *term)
{
    if (!g) return fail(LIME_ERR_ARG, "lime_gindex_info: the index is NULL");
    if (n_docs) *n_docs = g->n_docs;
    if (n_text) *n_text = g->n_text;
    if (lcp_cap) *lcp_cap = g->lcp_cap;
    if (term) *term = g->term;
    return LIME_OK;
}

extern "C" void lime_gindex_free(lime_gindex *g)
{
    if (!g) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(g->ctx->device);
    gindex_release(g);
    (void)hipSetDevice(cur);
}

// ---- the file ------------------------------------------------------------------------------------------------------------
namespace {
constexpr size_t GIDX_HEADER = 64;
constexpr uint16_t GIDX_VERSION = 1;
const char GIDX_MAGIC[4] = {'L', 'G', 'I', 'X'};

template <typename T> void put(uint8_t *h, size_t at, T v) { for (size_t k = 0; k < sizeof(T); ++k) h[at + k] = (uint8_t)((uint64_t)v >> (8 * k)); }
template <typename T> T get(const uint8_t *h, size_t at) { uint64_t v = 0; for (size_t k = 0; k < sizeof(T); ++k) v |= (uint64_t)h[at + k] << (8 * k); return (T)v; }

struct FileGuard { FILE *f = nullptr; ~FileGuard() { if (f) fclose(f); } };

// the header of an open file and the file's length against it -> the sizes in *g (no device, no allocation)
int read_header(const char *who, FILE *f, const char *path, lime_gindex *g)
{
    uint8_t h[GIDX_HEADER];
    struct stat sb;
    if (fstat(fileno(f), &sb) != 0) return fail(LIME_ERR_IO, "%s: cannot stat %s", who, path);
    if (fread(h, 1, GIDX_HEADER, f) != GIDX_HEADER) return fail(LIME_ERR_IO, "%s: %s is shorter than its header (%zu bytes)", who, path, GIDX_HEADER);
    if (memcmp(h, GIDX_MAGIC, 4) != 0) return fail(LIME_ERR_ARG, "%s: %s is not a genome index file (magic)", who, path);
    const uint16_t version = get<uint16_t>(h, 4);
    if (version != GIDX_VERSION) return fail(LIME_ERR_ARG, "%s: %s has format version %u, this library reads version %u", who, path, version, GIDX_VERSION);
    if (h[7] != 0) return fail(LIME_ERR_ARG, "%s: %s: reserved header byte is %u", who, path, h[7]);
    g->term = h[6];
    g->n_docs = get<uint32_t>(h, 8);
    g->lcp_cap = get<uint32_t>(h, 12);
    g->n_text = get<uint64_t>(h, 16);
    if (check_positions(who, g->n_text, g->n_docs)) return LIME_ERR_ARG;
    const uint64_t n = g->n();
    const uint64_t have[6] = {get<uint64_t>(h, 24), get<uint64_t>(h, 32), get<uint64_t>(h, 40), get<uint64_t>(h, 48), get<uint32_t>(h, 56), get<uint32_t>(h, 60)};
    const uint64_t want[6] = {((uint64_t)g->n_docs + 1) * 8, n * 4, n * 4, n * 4, g->n_text, n};
    const char *name[6] = {"doc_off", "sa", "lcp", "da", "text", "ebwt"};
    for (int k = 0; k < 6; ++k)
        if (have[k] != want[k])
            return fail(LIME_ERR_ARG, "%s: %s: section %s has %llu bytes, %u documents and %llu symbols need %llu", who, path, name[k],
                        (unsigned long long)have[k], g->n_docs, (unsigned long long)g->n_text, (unsigned long long)want[k]);
    const uint64_t len = GIDX_HEADER + g->body_bytes();
    if ((uint64_t)sb.st_size < len)
        return fail(LIME_ERR_IO, "%s: %s is short: %llu bytes, its header asks for %llu", who, path, (unsigned long long)sb.st_size, (unsigned long long)len);
    if ((uint64_t)sb.st_size > len)
        return fail(LIME_ERR_ARG, "%s: %s has %llu bytes, its header asks for %llu", who, path, (unsigned long long)sb.st_size, (unsigned long long)len);
    return LIME_OK;
}
}

extern "C" int lime_gindex_probe(const char *path, uint32_t *n_docs, uint64_t *n_text, uint32_t *lcp_cap, uint8_t *term)
{
    if (!path) return fail(LIME_ERR_ARG, "lime_gindex_probe: path is NULL");
    FileGuard fg; fg.f = fopen(path, "rb");
    if (!fg.f) return fail(LIME_ERR_IO, "lime_gindex_probe: cannot open %s", path);
    lime_gindex g;
    int rc = read_header("lime_gindex_probe", fg.f, path, &g); if (rc) return rc;
    if (n_docs) *n_docs = g.n_docs;
    if (n_text) *n_text = g.n_text;
    if (lcp_cap) *lcp_cap = g.lcp_cap;
    if (term) *term = g.term;
    return LIME_OK;
}

extern "C" int lime_gindex_save(const lime_gindex *g, const char *path)
{
    const char *who = "lime_gindex_save";
    if (!g || !path) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    int rc = check_ctx(g->ctx, who); if (rc) return rc;
    const size_t body = (size_t)g->body_bytes();
    std::unique_ptr<uint8_t[]> buf(new (std::nothrow) uint8_t[GIDX_HEADER + body]);
    if (!buf) return fail(LIME_ERR_NOMEM, "%s: out of host memory (%zu bytes)", who, GIDX_HEADER + body);
    uint8_t *h = buf.get();
    memset(h, 0, GIDX_HEADER);
    memcpy(h, GIDX_MAGIC, 4);
    const uint64_t n = g->n();
    put<uint16_t>(h, 4, GIDX_VERSION); h[6] = g->term;
    put<uint32_t>(h, 8, g->n_docs); put<uint32_t>(h, 12, g->lcp_cap); put<uint64_t>(h, 16, g->n_text);
    put<uint64_t>(h, 24, ((uint64_t)g->n_docs + 1) * 8); put<uint64_t>(h, 32, n * 4); put<uint64_t>(h, 40, n * 4); put<uint64_t>(h, 48, n * 4);
    put<uint32_t>(h, 56, (uint32_t)g->n_text); put<uint32_t>(h, 60, (uint32_t)n);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h + GIDX_HEADER, g->blk.p, body, hipMemcpyDeviceToHost));
    const std::string tmp = std::string(path) + ".tmp" + std::to_string((long)getpid());
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(LIME_ERR_IO, "%s: cannot create %s", who, tmp.c_str());
    const bool wrote = fwrite(h, 1, GIDX_HEADER + body, f) == GIDX_HEADER + body;
    const bool closed = fclose(f) == 0;
    if (!wrote || !closed || rename(tmp.c_str(), path) != 0) {
        (void)remove(tmp.c_str());
        return fail(LIME_ERR_IO, "%s: cannot write %s", who, path);
    }
    return LIME_OK;
}

extern "C" int lime_gindex_load(lime_ctx *c, const char *path, lime_gindex **out)
{
    const char *who = "lime_gindex_load";
    if (!c || !path || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    FileGuard fg; fg.f = fopen(path, "rb");
    if (!fg.f) return fail(LIME_ERR_IO, "%s: cannot open %s", who, path);
    lime_gindex hd;
    int rc = read_header(who, fg.f, path, &hd); if (rc) return rc;
    const size_t body = (size_t)hd.body_bytes();
    std::unique_ptr<uint8_t[]> buf(new (std::nothrow) uint8_t[body ? body : 1]);
    if (!buf) return fail(LIME_ERR_NOMEM, "%s: out of host memory (%zu bytes)", who, body);
    if (fread(buf.get(), 1, body, fg.f) != body) return fail(LIME_ERR_IO, "%s: cannot read %s", who, path);
    // doc_off is checked here, on the host, before anything on the device indexes with it
    if ((rc = check_doc_off(who, reinterpret_cast<const uint64_t *>(buf.get()), hd.n_docs, &hd.n_text))) return rc;
    if ((rc = check_ctx(c, who))) return rc;
    GindexGuard gg;
    if ((rc = gindex_new(c, who, hd.n_docs, hd.n_text, hd.term, hd.lcp_cap, gg))) return rc;
    HIP_TRY(hipMemcpy(gg.g->blk.p, buf.get(), body, hipMemcpyHostToDevice));
    *out = gg.take();
    return LIME_OK;
}

// ---- the merge -------------------------------------------------------------------------------------------------------------
extern "C" uint64_t lime_merge_size(const lime_gindex *g, const uint64_t *reads_doc_off, uint32_t n_reads)
{
    return (g ? g->n() : 0) + (reads_doc_off ? reads_doc_off[n_reads] + n_reads : 0);
}

extern "C" int lime_get_merge_info(lime_ctx *c, double out[8])
{
    if (!c || !out) return fail(LIME_ERR_ARG, "lime_get_merge_info: NULL argument");
    for (int k = 0; k < 8; ++k) out[k] = c->mrg_info[k];
    return LIME_OK;
}

// what both front ends refuse before anything is allocated or launched
static int check_merge(const char *who, lime_ctx *c, const lime_gindex *g, uint32_t n_reads, uint64_t n_reads_text, uint32_t lcp_cap)
{
    if (!c) return fail(LIME_ERR_ARG, "%s: ctx is NULL", who);
    if (!g) return fail(LIME_ERR_ARG, "%s: the genome index is NULL", who);
    if (g->ctx != c) return fail(LIME_ERR_ARG, "%s: the genome index belongs to another context", who);
    int rc = check_positions(who, n_reads_text, n_reads); if (rc) return rc;
    if (n_reads_text + n_reads + g->n() > 0xFFFFFFFFull)
        return fail(LIME_ERR_ARG, "%s: %llu read positions + %llu genome positions exceed 2^32 - 1 (one GPU, 32-bit suffix positions)", who,
                    (unsigned long long)(n_reads_text + n_reads), (unsigned long long)g->n());
    if (g->lcp_cap && (lcp_cap == 0 || lcp_cap > g->lcp_cap))
        return fail(LIME_ERR_ARG, "%s: lcp_cap %u cannot be served from an index built with lcp_cap %u (1 .. %u can)", who, lcp_cap, g->lcp_cap, g->lcp_cap);
    return LIME_OK;
}

extern "C" int lime_merge_index_dev(lime_ctx *c, const uint8_t *d_reads_text, const uint64_t *d_reads_doc_off, uint32_t n_reads,
                                    uint64_t n_reads_text, const lime_gindex *g, uint32_t lcp_cap, uint8_t *d_ebwt, uint32_t *d_lcp,
                                    uint32_t *d_da, void *stream)
{
    const char *who = "lime_merge_index_dev";
    int rc = check_merge(who, c, g, n_reads, n_reads_text, lcp_cap); if (rc) return rc;
    if (!d_reads_doc_off || (n_reads_text && !d_reads_text)) return fail(LIME_ERR_ARG, "%s: NULL array", who);
    if ((rc = check_ctx(c, who))) return rc;
    for (double &v : c->mrg_info) v = 0.0;
    const uint32_t nr = (uint32_t)(n_reads_text + n_reads), ng = (uint32_t)g->n();
    if (!nr && !ng) return LIME_OK;
    hipStream_t st = (hipStream_t)stream;

    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int k = 0; k < 4; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } ev_guard{ev};
    if (c->timing) { for (auto &e : ev) HIP_TRY(hipEventCreate(&e)); HIP_TRY(hipEventRecord(ev[0], st)); }

    // 17 bytes per read position: the reads' own sa, da, lcp, ebwt and j
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t r4 = up((size_t)nr * 4), r1 = up((size_t)nr);
    DevBuf rblk;
    if ((rc = rblk.alloc(4 * r4 + r1)))
        return fail(rc, "%s: no device memory for %u read positions (17 bytes each): %s", who, nr, lime_last_error());
    uint8_t *at = static_cast<uint8_t *>(rblk.p);
    auto take = [&](size_t b) { uint8_t *p = at; at += b; return p; };
    uint32_t *sa_r = (uint32_t *)take(r4), *da_r = (uint32_t *)take(r4), *lcp_r = (uint32_t *)take(r4), *j = (uint32_t *)take(r4);
    uint8_t *ebwt_r = take(r1);
    // 1: the reads alone (the builder's 52 bytes per position are back when it returns)
    if (nr) {
        rc = build_index_impl(c, who, d_reads_text, d_reads_doc_off, n_reads, n_reads_text, g->term, lcp_cap,
                              d_ebwt ? ebwt_r : nullptr, d_lcp ? lcp_r : nullptr, da_r, sa_r, st);
        if (rc) return rc;
    }
    c->mrg_info[0] = nr ? c->idx_info[0] : 0.0; c->mrg_info[1] = (double)nr;
    if (c->timing) HIP_TRY(hipEventRecord(ev[1], st));

    // 8 bytes per genome position: the words the running maximum is taken of, and c; + rocPRIM's storage + the runs' counter
    size_t tmp_bytes = 0;
    HIP_TRY(idx_scan_max(nullptr, &tmp_bytes, nullptr, nullptr, (size_t)ng + 1, st));
    const size_t g4 = up(((size_t)ng + 1) * 4);
    DevBuf gblk;
    if ((rc = gblk.alloc(2 * g4 + up(tmp_bytes) + 256)))
        return fail(rc, "%s: no device memory for %u genome positions (8 bytes each): %s", who, ng, lime_last_error());
    at = static_cast<uint8_t *>(gblk.p);
    uint32_t *end = (uint32_t *)take(g4), *cnt = (uint32_t *)take(g4);
    void *tmp = take(up(tmp_bytes));
    uint32_t *runs = (uint32_t *)take(256);

    const MrgSide rs = {d_reads_text, d_reads_doc_off, sa_r, da_r, d_ebwt ? ebwt_r : nullptr, d_lcp ? lcp_r : nullptr, n_reads_text, n_reads, nr};
    const MrgSide gs = {g->text(), g->doc_off(), g->sa(), g->da(), g->ebwt(), g->lcp(), g->n_text, g->n_docs, ng};
    // 2: the rank of every read suffix among the genome suffixes
    mrg_launch_rank(rs, gs, j, st);
    HIP_TRY(hipGetLastError());
    if (c->timing) HIP_TRY(hipEventRecord(ev[2], st));
    // 3: c[k] = read suffixes with j <= k, from the last read suffix of every run
    HIP_TRY(hipMemsetAsync(end, 0, ((size_t)ng + 1) * 4, st));
    HIP_TRY(hipMemsetAsync(runs, 0, 4, st));
    mrg_launch_ends(j, nr, ng, end, runs, st);
    HIP_TRY(idx_scan_max(tmp, &tmp_bytes, end, cnt, (size_t)ng + 1, st));
    // 4: both sides to their slots
    mrg_launch_write_reads(rs, gs, j, lcp_cap, d_ebwt, d_lcp, d_da, st);
    mrg_launch_write_genomes(rs, gs, cnt, lcp_cap, d_ebwt, d_lcp, d_da, st);
    HIP_TRY(hipGetLastError());
    if (c->timing) HIP_TRY(hipEventRecord(ev[3], st));
    uint32_t h_runs = 0;
    HIP_TRY(hipMemcpyAsync(&h_runs, runs, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                                   // (the scratch goes back when this returns)
    c->mrg_info[2] = (double)h_runs;
    if (c->timing)
        for (int k = 0; k < 3; ++k) { float ms = 0.0f; if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) c->mrg_info[3 + k] = ms; }
    return LIME_OK;
}

extern "C" int lime_merge_index(lime_ctx *c, const uint8_t *reads_text, const uint64_t *reads_doc_off, uint32_t n_reads,
                                const lime_gindex *g, uint32_t lcp_cap, uint8_t *ebwt, uint32_t *lcp, uint32_t *da)
{
    const char *who = "lime_merge_index";
    if (!c) return fail(LIME_ERR_ARG, "%s: ctx is NULL", who);
    int rc = check_doc_off(who, reads_doc_off, n_reads, nullptr); if (rc) return rc;
    const uint64_t n_text = reads_doc_off[n_reads];
    if ((rc = check_merge(who, c, g, n_reads, n_text, lcp_cap))) return rc;
    if (n_text && !reads_text) return fail(LIME_ERR_ARG, "%s: text is NULL", who);
    if ((rc = check_ctx(c, who))) return rc;
    const uint64_t n = n_text + n_reads + g->n();
    if (!n) return LIME_OK;
    DevBuf dt, df, de, dl, dd;
    if ((rc = dt.upload(reads_text, n_text)) || (rc = df.upload(reads_doc_off, ((size_t)n_reads + 1) * 8))) return rc;
    if ((ebwt && (rc = de.alloc(n))) || (lcp && (rc = dl.alloc(n * 4))) || (da && (rc = dd.alloc(n * 4)))) return rc;
    rc = lime_merge_index_dev(c, (const uint8_t *)dt.p, (const uint64_t *)df.p, n_reads, n_text, g, lcp_cap,
                              (uint8_t *)de.p, (uint32_t *)dl.p, (uint32_t *)dd.p, nullptr);
    if (rc) return rc;
    if (ebwt && (rc = d2h_pageable(c, ebwt, de.p, n, nullptr))) return rc;
    if (lcp && (rc = d2h_pageable(c, lcp, dl.p, n * 4, nullptr))) return rc;
    if (da && (rc = d2h_pageable(c, da, dd.p, n * 4, nullptr))) return rc;
    return LIME_OK;
}
