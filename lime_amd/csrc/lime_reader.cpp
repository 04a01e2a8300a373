// lime_reader.cpp -- a reads file in batches of records (lime_seq_reader: a raw device window that is refilled through two pinned buffers,
// cut into whole records by the kernels of lime_seqcut_kernel.hip and parsed up to the cut by lime_docs.cpp's passes), and a sample of
// any size classified batch by batch (lime_classify_sample_stream).  include/lime_hip.h states the contract.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>

#include "lime_index.h"
#include "lime_ctx.h"
#include "lime_classify.h"

using namespace lime;
using namespace lime_host;

namespace {
constexpr uint64_t WINDOW_DEFAULT = 64ull << 20, WINDOW_MAX = 0xFFFFFFFFull;
constexpr size_t STAGE_BYTES = 8u << 20, STAGE_MIN = 64u << 10;
struct DocsPair {                                        // a batch's documents, one per mate
    lime_docs *d[2] = {nullptr, nullptr};
    ~DocsPair() { release(); }
    void release() { for (lime_docs *&x : d) { lime_docs_free(x); x = nullptr; } }
};
}

// ---- the cut ------------------------------------------------------------------------------------------------------------
static int seq_cut(const char *who, const uint8_t *d_bytes, uint64_t n, int format, uint32_t max_reads, int eof, hipStream_t st, uint64_t out[3])
{
    out[0] = out[1] = out[2] = 0;
    if (!n) return LIME_OK;                              // (no byte, no marker, no record)
    const uint32_t nb = (uint32_t)((n + LIME_FASTA_BLOCK - 1) / LIME_FASTA_BLOCK);
    size_t tmp_bytes = 0;
    HIP_TRY(idx_scan_sum(nullptr, &tmp_bytes, nullptr, nullptr, (size_t)nb + 1, false, st));
    WordScratch scratch;
    int rc = scratch.alloc(2, nb, tmp_bytes);
    if (rc) return fail(rc, "%s: no device memory for the cut of %llu bytes: %s", who, (unsigned long long)n, lime_last_error());
    uint32_t *cnt = scratch.words(0), *off = scratch.words(1);             // the blocks' markers with a 0 behind the last block's; their exclusive sum
    uint64_t *d_out = (uint64_t *)scratch.cell();
    void *tmp = scratch.tmp();
    HIP_TRY(hipMemsetAsync(cnt, 0, scratch.stride, st));
    if (format) fq_launch_lines(d_bytes, n, nb, cnt, st);
    else sc_launch_headers(d_bytes, n, nb, cnt, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(idx_scan_sum(tmp, &tmp_bytes, cnt, off, (size_t)nb + 1, false, st));
    sc_launch_select(d_bytes, n, nb, off, format, max_reads, eof, d_out, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                   // (the scratch goes back when this returns)
    return LIME_OK;
}

extern "C" int lime_seq_cut_dev(lime_ctx *c, const uint8_t *d_bytes, uint64_t n, int format, uint32_t max_reads, int eof, void *stream,
                                uint64_t *cut, uint64_t *n_records, uint64_t *n_markers)
{
    const char *who = "lime_seq_cut_dev";
    if (!c) return fail(LIME_ERR_ARG, "%s: ctx is NULL", who);
    if (n > WINDOW_MAX) return fail(LIME_ERR_ARG, "%s: %llu bytes of input; the cut counts in 32 bits (at most 2^32 - 1 bytes)", who, (unsigned long long)n);
    if (n && !d_bytes) return fail(LIME_ERR_ARG, "%s: NULL array", who);
    if (format != 0 && format != 1) return fail(LIME_ERR_ARG, "%s: format is %d; 0 is FASTA, 1 is FASTQ", who, format);
    if (!max_reads) return fail(LIME_ERR_ARG, "%s: max_reads is 0", who);
    int rc = check_ctx(c, who); if (rc) return rc;
    uint64_t out[3];
    if ((rc = seq_cut(who, d_bytes, n, format, max_reads, eof != 0, (hipStream_t)stream, out))) return rc;
    if (cut) *cut = out[0];
    if (n_records) *n_records = out[1];
    if (n_markers) *n_markers = out[2];
    return LIME_OK;
}

// ---- the reader ---------------------------------------------------------------------------------------------------------
lime_seq_reader::~lime_seq_reader()
{
    for (int k = 0; k < 2; ++k) { if (ev[k]) (void)hipEventDestroy(ev[k]); if (pin[k]) (void)hipHostFree(pin[k]); }
    if (f) fclose(f);
    if (mate) mate->mate = nullptr;                      // (lime_seq_reader_set_overlap: the other reader stays, unlinked)
}

static void reader_release(lime_seq_reader *r)
{
    if (!r) return;
    std::vector<lime_seq_reader *> &v = r->ctx->readers;
    v.erase(std::remove(v.begin(), v.end(), r), v.end());
    delete r;
}

namespace {
struct ReaderGuard {
    lime_seq_reader *r = nullptr;
    ~ReaderGuard() { reader_release(r); }
    lime_seq_reader *take() { lime_seq_reader *x = r; r = nullptr; return x; }
};
}

// the window and the pinned pair of a reader whose source is set
static int reader_setup(lime_seq_reader *r, const char *who, uint64_t window_bytes)
{
    uint64_t w = window_bytes ? window_bytes : std::min<uint64_t>(WINDOW_DEFAULT, std::max<uint64_t>(r->src_size, 1));
    if (w > WINDOW_MAX) return fail(LIME_ERR_ARG, "%s: a window of %llu bytes; the parser counts in 32 bits (at most 2^32 - 1 bytes)", who, (unsigned long long)w);
    int rc = r->win.acquire((size_t)w + 16);
    if (rc) return fail(rc, "%s: no device memory for a window of %llu bytes: %s", who, (unsigned long long)w, lime_last_error());
    r->win.cap = (size_t)w;                              // (the 16 bytes of slack are not the window's)
    r->pin_bytes = (size_t)std::min<uint64_t>(STAGE_BYTES, std::max<uint64_t>(w, STAGE_MIN));       // (a small window may grow)
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(hipHostMalloc(&r->pin[k], r->pin_bytes));
        HIP_TRY(hipEventCreateWithFlags(&r->ev[k], hipEventDisableTiming));
    }
    return LIME_OK;
}

static int reader_new(lime_ctx *c, const char *who, ReaderGuard &rg)
{
    lime_seq_reader *r = new (std::nothrow) lime_seq_reader();
    if (!r) return fail(LIME_ERR_NOMEM, "%s: out of host memory", who);
    r->ctx = c;
    c->readers.push_back(r);
    rg.r = r;
    return LIME_OK;
}

extern "C" int lime_seq_reader_open(lime_ctx *c, const char *path, uint64_t window_bytes, lime_seq_reader **out)
{
    const char *who = "lime_seq_reader_open";
    if (!c || !path || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    int format = 0;
    if (lime_seq_format(path, &format) != LIME_OK) return fail(LIME_ERR_IO, "%s: cannot open %s", who, path);
    int rc = check_ctx(c, who); if (rc) return rc;
    ReaderGuard rg;
    if ((rc = reader_new(c, who, rg))) return rc;
    lime_seq_reader *r = rg.r;
    r->format = format;
    r->f = fopen(path, "rb");
    if (!r->f) return fail(LIME_ERR_IO, "%s: cannot open %s", who, path);
    if (fseeko(r->f, 0, SEEK_END) != 0) return fail(LIME_ERR_IO, "%s: cannot seek in %s", who, path);
    const off_t size = ftello(r->f);
    if (size < 0 || fseeko(r->f, 0, SEEK_SET) != 0) return fail(LIME_ERR_IO, "%s: cannot seek in %s", who, path);
    r->src_size = (uint64_t)size;
    if ((rc = reader_setup(r, who, window_bytes))) return rc;
    *out = rg.take();
    return LIME_OK;
}

extern "C" int lime_seq_reader_open_bytes(lime_ctx *c, const uint8_t *bytes, uint64_t n, int format, uint64_t window_bytes, lime_seq_reader **out)
{
    const char *who = "lime_seq_reader_open_bytes";
    if (!c || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    if (n && !bytes) return fail(LIME_ERR_ARG, "%s: NULL array", who);
    if (format != 0 && format != 1) return fail(LIME_ERR_ARG, "%s: format is %d; 0 is FASTA, 1 is FASTQ", who, format);
    int rc = check_ctx(c, who); if (rc) return rc;
    ReaderGuard rg;
    if ((rc = reader_new(c, who, rg))) return rc;
    rg.r->format = format;
    rg.r->host = bytes;
    rg.r->src_size = n;
    if ((rc = reader_setup(rg.r, who, window_bytes))) return rc;
    *out = rg.take();
    return LIME_OK;
}

// the source's next bytes behind win[fill), until the window is full or the source at its end: one pinned buffer is filled while the
// other one's copy runs
static int reader_fill(lime_seq_reader *r, const char *who)
{
    while (r->fill < r->win.cap && r->src_pos < r->src_size) {
        const int k = r->pin_k;
        HIP_TRY(hipEventSynchronize(r->ev[k]));          // (an event that was never recorded is complete)
        const size_t want = (size_t)std::min<uint64_t>(std::min<uint64_t>(r->pin_bytes, r->win.cap - r->fill), r->src_size - r->src_pos);
        if (r->f) {
            const size_t got = fread(r->pin[k], 1, want, r->f);
            if (got != want)
                return fail(LIME_ERR_IO, "%s: cannot read the file (%llu of %llu bytes)", who, (unsigned long long)(r->src_pos + got), (unsigned long long)r->src_size);
        } else {
            memcpy(r->pin[k], r->host + r->src_pos, want);
        }
        HIP_TRY(hipMemcpyAsync(r->win.p + r->fill, r->pin[k], want, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipEventRecord(r->ev[k], nullptr));
        r->fill += want; r->src_pos += want;
        r->pin_k ^= 1;
    }
    return LIME_OK;
}

// win[start .. fill) to the front of a window of new_cap >= fill - start bytes.  Never an overlapping device copy: the tail goes to
// the front of the same block only where it is no longer than the gap in front of it, else to a new block that takes the window's place
static int reader_compact(lime_seq_reader *r, const char *who, uint64_t new_cap)
{
    const uint64_t tail = r->fill - r->start;
    if (new_cap == r->win.cap && tail <= r->start) {
        if (tail) HIP_TRY(hipMemcpyAsync(r->win.p, r->win.p + r->start, (size_t)tail, hipMemcpyDeviceToDevice, nullptr));
    } else {
        DevArr<uint8_t> next;
        int rc = next.acquire((size_t)new_cap + 16);
        if (rc) return fail(rc, "%s: no device memory for a window of %llu bytes: %s", who, (unsigned long long)new_cap, lime_last_error());
        next.cap = (size_t)new_cap;
        if (tail) HIP_TRY(hipMemcpyAsync(next.p, r->win.p + r->start, (size_t)tail, hipMemcpyDeviceToDevice, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));          // (the old block goes back when this returns)
        r->win.swap(next);
    }
    r->start = 0; r->fill = tail;
    return LIME_OK;
}

// out_qc: the batch handed out is added to the reader's OUT tables here (next_pair adds it behind its cut)
static int reader_next(lime_seq_reader *r, const char *who, uint32_t max_reads, lime_docs **docs, uint64_t *first_record, bool out_qc)
{
    for (;;) {
        int rc;
        if (r->start == r->fill) r->start = r->fill = 0;
        if (r->start == 0 && (rc = reader_fill(r, who))) return rc;
        const bool eof = r->src_pos == r->src_size;
        const uint64_t n = r->fill - r->start;
        if (!n && eof) return LIME_OK;                   // the end of the file
        uint64_t cut[3];
        if ((rc = seq_cut(who, r->win.p + r->start, n, r->format, max_reads, eof, nullptr, cut))) return rc;
        if (cut[1] < max_reads && !eof) {                // the records do not reach: more bytes, in a larger window where this one is full
            uint64_t cap = r->win.cap;
            if (r->start == 0) {
                if (cap >= WINDOW_MAX)
                    return fail(LIME_ERR_ARG, "%s: %u records do not fit a window of 2^32 - 1 bytes, the largest the parser counts in", who, max_reads);
                cap = std::min<uint64_t>(WINDOW_MAX, cap * 2);
            }
            if ((rc = reader_compact(r, who, cap))) return rc;
            if ((rc = reader_fill(r, who))) return rc;
            continue;
        }
        if (cut[0] > n) return fail(LIME_ERR_HIP, "%s: the cut lies behind the window", who);
        lime_docs *d = nullptr;
        const uint8_t *b = r->win.p + r->start;
        if (r->format) rc = docs_parse_fastq_dev(r->ctx, who, b, cut[0], r->n_lines, nullptr, &d, r->stages.needs_qual());
        else rc = docs_parse_fasta_dev(r->ctx, who, b, cut[0], nullptr, &d);
        if (rc) return rc;
        if ((rc = docs_stages(r->ctx, who, r->stages, &d))) return rc;         // the batch as it is handed out
        uint32_t nd = 0;
        lime_docs_info(d, &nd, nullptr);
        if (r->n_records + nd > 0xFFFFFFFFull) {
            lime_docs_free(d);
            return fail(LIME_ERR_ARG, "%s: more than 2^32 - 1 records", who);
        }
        if (first_record) *first_record = r->n_records;
        r->start += cut[0]; r->n_bytes += cut[0];
        r->n_records += nd;
        if (r->format) r->n_lines += 4ull * nd;
        if (!nd) { lime_docs_free(d); continue; }        // (FASTA without a header line up to the file's end: no record, the next turn ends)
        if (out_qc && (rc = docs_count_out(r->ctx, who, r->stages, &d))) return rc;
        *docs = d;
        return LIME_OK;
    }
}

static int seq_next(lime_seq_reader *r, uint32_t max_reads, lime_docs **docs, uint64_t *first_record, bool out_qc)
{
    const char *who = "lime_seq_reader_next";
    if (!r || !docs) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *docs = nullptr;
    if (!max_reads) return fail(LIME_ERR_ARG, "%s: max_reads is 0", who);
    if (r->failed) return fail(r->failed, "%s", r->failure.c_str());
    int rc = check_ctx(r->ctx, who); if (rc) return rc;
    r->asked = true;
    rc = reader_next(r, who, max_reads, docs, first_record, out_qc);
    if (rc == LIME_ERR_ARG) { r->failed = rc; r->failure = lime_last_error(); }     // a refusal of the file is final
    return rc;
}

extern "C" int lime_seq_reader_next(lime_seq_reader *r, uint32_t max_reads, lime_docs **docs, uint64_t *first_record)
{
    return seq_next(r, max_reads, docs, first_record, true);
}

extern "C" int lime_seq_reader_set_trim(lime_seq_reader *r, uint32_t q5, uint32_t q3)
{
    const char *who = "lime_seq_reader_set_trim";
    if (!r) return fail(LIME_ERR_ARG, "%s: the reader is NULL", who);
    if (!r->format) return fail(LIME_ERR_ARG, "%s: the reader's file is FASTA; only FASTQ holds qualities", who);
    if (q5 > 93 || q3 > 93) return fail(LIME_ERR_ARG, "%s: cutoffs %u,%u; a Phred+33 quality is 0 .. 93", who, q5, q3);
    if (r->asked) return fail(LIME_ERR_ARG, "%s: the reader has handed out records already; the trim is set before the first lime_seq_reader_next", who);
    r->stages.trim = true; r->stages.q5 = q5; r->stages.q3 = q3;
    return LIME_OK;
}

extern "C" int lime_seq_reader_trim_info(const lime_seq_reader *r, lime_trim_info_t *info)
{
    if (!r || !info) return fail(LIME_ERR_ARG, "lime_seq_reader_trim_info: NULL argument");
    *info = r->stages.trimmed;
    return LIME_OK;
}

extern "C" int lime_seq_reader_set_adapter(lime_seq_reader *r, const uint8_t *adapter, uint32_t m, uint32_t min_overlap, uint32_t max_err_pct)
{
    const char *who = "lime_seq_reader_set_adapter";
    if (!r) return fail(LIME_ERR_ARG, "%s: the reader is NULL", who);
    uint64_t masks[4];
    int rc = adapter_masks(who, adapter, m, min_overlap, max_err_pct, masks); if (rc) return rc;
    if (r->asked) return fail(LIME_ERR_ARG, "%s: the reader has handed out records already; the adapter is set before the first lime_seq_reader_next", who);
    MateStages &s = r->stages;
    s.adapter = true; s.ad_m = m; s.ad_overlap = min_overlap; s.ad_err = max_err_pct;
    memcpy(s.ad_masks, masks, sizeof masks);
    return LIME_OK;
}

extern "C" int lime_seq_reader_adapter_info(const lime_seq_reader *r, lime_trim_info_t *info)
{
    if (!r || !info) return fail(LIME_ERR_ARG, "lime_seq_reader_adapter_info: NULL argument");
    *info = r->stages.ad_trimmed;
    return LIME_OK;
}

extern "C" int lime_seq_reader_set_filter(lime_seq_reader *r, const lime_filter_t *filter)
{
    const char *who = "lime_seq_reader_set_filter";
    if (!r) return fail(LIME_ERR_ARG, "%s: the reader is NULL", who);
    int rc = filter_check(who, filter); if (rc) return rc;
    if (r->asked) return fail(LIME_ERR_ARG, "%s: the reader has handed out records already; the filter is set before the first lime_seq_reader_next", who);
    r->stages.filter = true; r->stages.fl = *filter;
    return LIME_OK;
}

extern "C" int lime_seq_reader_filter_info(const lime_seq_reader *r, lime_filter_info_t *info)
{
    if (!r || !info) return fail(LIME_ERR_ARG, "lime_seq_reader_filter_info: NULL argument");
    *info = r->stages.filtered;
    return LIME_OK;
}

// ---- per-position statistics of the batches as parsed and as handed out (lime_docs_qc_dev) ----
extern "C" int lime_seq_reader_set_qc(lime_seq_reader *r, uint32_t n_pos)
{
    const char *who = "lime_seq_reader_set_qc";
    if (!r) return fail(LIME_ERR_ARG, "%s: the reader is NULL", who);
    if (!n_pos || n_pos > LIME_QC_MAX_POS) return fail(LIME_ERR_ARG, "%s: %u positions; there are 1 .. %u", who, n_pos, LIME_QC_MAX_POS);
    if (r->asked) return fail(LIME_ERR_ARG, "%s: the reader has handed out records already; the statistics are set before the first lime_seq_reader_next", who);
    r->stages.n_pos = n_pos;
    r->stages.qc_raw.assign(LIME_QC_WORDS(n_pos), 0);
    r->stages.qc_out.assign(LIME_QC_WORDS(n_pos), 0);
    return LIME_OK;
}

extern "C" int lime_seq_reader_qc(const lime_seq_reader *r, int which, uint64_t *tables)
{
    const char *who = "lime_seq_reader_qc";
    if (!r || !tables) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (which != 0 && which != 1) return fail(LIME_ERR_ARG, "%s: tables %d; 0 is the batches as parsed, 1 as handed out", who, which);
    const MateStages &s = r->stages;
    if (!s.n_pos) { memset(tables, 0, 8 * LIME_QC_WORDS(1u)); return LIME_OK; }
    memcpy(tables, (which ? s.qc_out : s.qc_raw).data(), 8 * (size_t)LIME_QC_WORDS(s.n_pos));
    return LIME_OK;
}

// ---- the overlap cut over two readers' batches (lime_docs_trim_overlap_dev): the one stage that needs both mates ----
extern "C" int lime_seq_reader_set_overlap(lime_seq_reader *r1, lime_seq_reader *r2, uint32_t min_overlap, uint32_t max_err_pct)
{
    const char *who = "lime_seq_reader_set_overlap";
    if (!r1 || !r2) return fail(LIME_ERR_ARG, "%s: a reader is NULL", who);
    if (r1 == r2) return fail(LIME_ERR_ARG, "%s: the two mates are one reader", who);
    if (r1->ctx != r2->ctx) return fail(LIME_ERR_ARG, "%s: the readers belong to different contexts", who);
    int rc = overlap_check(who, min_overlap, max_err_pct); if (rc) return rc;
    if (r1->asked || r2->asked)
        return fail(LIME_ERR_ARG, "%s: a reader has handed out records already; the overlap is set before the first lime_seq_reader_next of either", who);
    if (r1->mate || r2->mate) return fail(LIME_ERR_ARG, "%s: a reader is linked already", who);
    r1->mate = r2; r2->mate = r1;
    r1->ov_overlap = r2->ov_overlap = min_overlap; r1->ov_err = r2->ov_err = max_err_pct;
    return LIME_OK;
}

// a batch from each of two linked readers, cut at the mates' overlap.  *uneven: the batches hold different numbers of records (one file has
// ended before the other); both are dropped, LIME_OK, and the caller words the refusal
static int next_pair_impl(const char *who, lime_seq_reader *r1, lime_seq_reader *r2, uint32_t max_reads, lime_docs **docs1, lime_docs **docs2,
                          uint64_t *first_record, bool *uneven, uint32_t got[2])
{
    *uneven = false;
    got[0] = got[1] = 0;
    DocsPair batch;
    uint64_t first = 0;
    int rc;
    if ((rc = seq_next(r1, max_reads, &batch.d[0], &first, false))) return rc;      // (the batches are counted behind the cut)
    if ((rc = seq_next(r2, max_reads, &batch.d[1], nullptr, false))) return rc;
    for (int m = 0; m < 2; ++m) if (batch.d[m]) lime_docs_info(batch.d[m], &got[m], nullptr);
    if (got[0] != got[1]) { *uneven = true; return LIME_OK; }
    if (!got[0]) return LIME_OK;                         // the end of both files
    lime_overlap_info_t oi;
    if ((rc = docs_overlap_impl(r1->ctx, who, batch.d[0], batch.d[1], r1->ov_overlap, r1->ov_err, nullptr, nullptr, docs1, docs2, &oi))) return rc;
    add_info(r1->overlapped, oi);
    r2->overlapped = r1->overlapped;
    if ((rc = docs_count_out(r1->ctx, who, r1->stages, docs1, docs2))) return rc;     // the batches as they are handed out, behind the cut
    if ((rc = docs_count_out(r2->ctx, who, r2->stages, docs2, docs1))) return rc;
    if (first_record) *first_record = first;
    return LIME_OK;
}

extern "C" int lime_seq_reader_next_pair(lime_seq_reader *r1, lime_seq_reader *r2, uint32_t max_reads, lime_docs **docs1, lime_docs **docs2,
                                         uint64_t *first_record)
{
    const char *who = "lime_seq_reader_next_pair";
    if (docs1) *docs1 = nullptr;
    if (docs2) *docs2 = nullptr;
    if (!r1 || !r2 || !docs1 || !docs2) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (r1 == r2 || r1->mate != r2 || r2->mate != r1)
        return fail(LIME_ERR_ARG, "%s: the readers are not linked to each other (lime_seq_reader_set_overlap)", who);
    if (!max_reads) return fail(LIME_ERR_ARG, "%s: max_reads is 0", who);
    bool uneven = false;
    uint32_t got[2];
    int rc = next_pair_impl(who, r1, r2, max_reads, docs1, docs2, first_record, &uneven, got); if (rc) return rc;
    if (uneven)
        return fail(LIME_ERR_ARG, "%s: the read sets hold different numbers of reads (a batch of %u records in set 0, of %u in set 1)", who, got[0], got[1]);
    return LIME_OK;
}

extern "C" int lime_seq_reader_overlap_info(const lime_seq_reader *r, lime_overlap_info_t *info)
{
    if (!r || !info) return fail(LIME_ERR_ARG, "lime_seq_reader_overlap_info: NULL argument");
    *info = r->overlapped;
    return LIME_OK;
}

extern "C" int lime_seq_reader_info(const lime_seq_reader *r, int *format, uint64_t *n_records, uint64_t *n_lines, uint64_t *n_bytes, uint64_t *window_bytes)
{
    if (!r) return fail(LIME_ERR_ARG, "lime_seq_reader_info: the reader is NULL");
    if (format) *format = r->format;
    if (n_records) *n_records = r->n_records;
    if (n_lines) *n_lines = r->n_lines;
    if (n_bytes) *n_bytes = r->n_bytes;
    if (window_bytes) *window_bytes = r->win.cap;
    return LIME_OK;
}

extern "C" void lime_seq_reader_close(lime_seq_reader *r)
{
    if (!r) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(r->ctx->device);
    (void)hipStreamSynchronize(nullptr);                 // (a copy out of the pinned buffers may still run)
    reader_release(r);
    (void)hipSetDevice(cur);
}

// ---- a sample, batch by batch -----------------------------------------------------------------------------------------------
// the records a reader still holds, read to the end and dropped
static int drain(lime_seq_reader *r, uint32_t batch_reads)
{
    for (;;) {
        lime_docs *d = nullptr;
        int rc = lime_seq_reader_next(r, batch_reads, &d, nullptr);
        if (rc) return rc;
        if (!d) return LIME_OK;
        lime_docs_free(d);
    }
}

// lime_classify_sample_stream (one shard) and lime_classify_sample_stream_shards
static int sample_stream_impl(const char *who, lime_ctx *c, uint32_t n_mates, lime_seq_reader *const *readers, uint32_t n_shards,
                              const lime_gindex *const *shards, const lime_taxonomy *tx, uint32_t alpha, uint32_t norm, float beta, int use_ebwt,
                              int binary, uint32_t lcp_cap, uint32_t batch_reads, lime_verdict_sink sink, void *user, uint64_t counts[4],
                              uint64_t *n_reads, uint64_t *n_batches, void *stream)
{
    uint64_t local[4];
    if (!counts) counts = local;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (n_reads) *n_reads = 0;
    if (n_batches) *n_batches = 0;
    // the sample call's refusals, in its order, before any read
    if (!c) return fail(LIME_ERR_ARG, "%s: ctx is NULL", who);
    if (n_mates != 1 && n_mates != 2) return fail(LIME_ERR_ARG, "%s: n_mates is %u; a sample has 1 (single-end) or 2 (paired-end) read sets", who, n_mates);
    if (!readers || !shards || (n_shards == 1 && !shards[0]) || !tx) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    int rc = sample_check_shards(who, c, n_shards, shards); if (rc) return rc;
    for (uint32_t m = 0; m < n_mates; ++m) {
        if (!readers[m]) return fail(LIME_ERR_ARG, "%s: reader %u is NULL", who, m);
        if (readers[m]->ctx != c) return fail(LIME_ERR_ARG, "%s: reader %u belongs to another context", who, m);
    }
    if (n_mates == 2 && readers[0] == readers[1]) return fail(LIME_ERR_ARG, "%s: the two read sets are one reader", who);
    for (uint32_t m = 0; m < n_mates; ++m)
        if (readers[m]->mate && (n_mates != 2 || readers[m]->mate != readers[1 - m]))
            return fail(LIME_ERR_ARG, "%s: reader %u is linked to a reader that is not in the call (lime_seq_reader_set_overlap)", who, m);
    const bool linked = n_mates == 2 && readers[0]->mate == readers[1];       // the batches are cut at the mates' overlap
    uint32_t n_refs = 0, cap = 0;
    if ((rc = sample_check_rules(who, n_shards, shards, tx, alpha, lcp_cap, &n_refs, &cap))) return rc;
    if (!batch_reads) return fail(LIME_ERR_ARG, "%s: batch_reads is 0", who);
    if ((rc = check_ctx(c, who))) return rc;

    std::vector<lime_verdict_t> verdicts;
    std::vector<lime_stats_t> stats((size_t)n_shards * 4);
    uint64_t total = 0, batches = 0;
    for (;;) {
        DocsPair batch;
        uint32_t got[2] = {0, 0};
        bool uneven = false;
        if (linked) {
            if ((rc = next_pair_impl(who, readers[0], readers[1], batch_reads, &batch.d[0], &batch.d[1], nullptr, &uneven, got))) return rc;
        } else {
            for (uint32_t m = 0; m < n_mates; ++m) {
                if ((rc = lime_seq_reader_next(readers[m], batch_reads, &batch.d[m], nullptr))) return rc;
                if (batch.d[m]) lime_docs_info(batch.d[m], &got[m], nullptr);
            }
            uneven = n_mates == 2 && got[0] != got[1];
        }
        if (uneven) {          // one mate has ended before the other: both counts, from the files' ends
            batch.release();
            for (uint32_t m = 0; m < 2; ++m) if ((rc = drain(readers[m], batch_reads))) return rc;
            return fail(LIME_ERR_ARG, "%s: the read sets hold different numbers of reads (%llu in set 0, %llu in set 1)", who,
                        (unsigned long long)readers[0]->n_records, (unsigned long long)readers[1]->n_records);
        }
        if (!got[0]) break;
        if (verdicts.size() < got[0]) verdicts.resize(got[0]);
        uint64_t part[4];
        rc = classify_sample_at(n_shards == 1 ? "lime_classify_sample_dev" : "lime_classify_sample_shards_dev", c, n_mates, batch.d, n_shards, shards, tx, alpha,
                                norm, beta, use_ebwt, binary, lcp_cap, verdicts.data(), part, stats.data(), stream, total);
        if (rc) return rc;
        batch.release();
        for (int k = 0; k < 4; ++k) counts[k] += part[k];
        if (sink && (rc = sink(user, total, verdicts.data(), got[0], stats.data()))) return rc;
        total += got[0]; ++batches;
        if (n_reads) *n_reads = total;
        if (n_batches) *n_batches = batches;
    }
    if (!total) return fail(LIME_ERR_ARG, "%s: the read sets hold no reads", who);
    return LIME_OK;
}

extern "C" int lime_classify_sample_stream(lime_ctx *c, uint32_t n_mates, lime_seq_reader *const *readers, const lime_gindex *gi,
                                           const lime_taxonomy *tx, uint32_t alpha, uint32_t norm, float beta, int use_ebwt, int binary,
                                           uint32_t lcp_cap, uint32_t batch_reads, lime_verdict_sink sink, void *user, uint64_t counts[4],
                                           uint64_t *n_reads, uint64_t *n_batches, void *stream)
{
    return sample_stream_impl("lime_classify_sample_stream", c, n_mates, readers, 1, &gi, tx, alpha, norm, beta, use_ebwt, binary, lcp_cap, batch_reads,
                              sink, user, counts, n_reads, n_batches, stream);
}

extern "C" int lime_classify_sample_stream_shards(lime_ctx *c, uint32_t n_mates, lime_seq_reader *const *readers, uint32_t n_shards,
                                                  const lime_gindex *const *shards, const lime_taxonomy *tx, uint32_t alpha, uint32_t norm,
                                                  float beta, int use_ebwt, int binary, uint32_t lcp_cap, uint32_t batch_reads,
                                                  lime_verdict_sink sink, void *user, uint64_t counts[4], uint64_t *n_reads, uint64_t *n_batches,
                                                  void *stream)
{
    return sample_stream_impl("lime_classify_sample_stream_shards", c, n_mates, readers, n_shards, shards, tx, alpha, norm, beta, use_ebwt, binary,
                              lcp_cap, batch_reads, sink, user, counts, n_reads, n_batches, stream);
}
