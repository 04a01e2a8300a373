// lime_docs.cpp -- document collections that stay in HBM (lime_docs: made from the raw bytes of a FASTA or FASTQ file by the kernels of
// lime_fasta_kernel.hip / lime_fastq_kernel.hip, or copied from parsed arrays), their reverse complements, FASTQ reads with their quality strings and
// the quality trim (lime_fqtrim_kernel.hip), the adapter trim (lime_adapter_kernel.hip), the read filter (lime_filter_kernel.hip), the overlap cut (lime_overlap_kernel.hip), the per-position statistics (lime_qc_kernel.hip), and a whole sample from documents to verdicts
// (lime_classify_sample_dev: per collection the merge into the genome index, the scan and clusterChoose, then Classify over the lists).
// include/lime_hip.h states the contract.
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

// ---- the handle ---------------------------------------------------------------------------------------------------------
static void docs_release(lime_docs *d)
{
    if (!d) return;
    std::vector<lime_docs *> &v = d->ctx->docs;
    v.erase(std::remove(v.begin(), v.end(), d), v.end());
    delete d;
}
namespace {
struct DocsGuard {                                       // releases a handle on an error path
    lime_docs *d = nullptr;
    ~DocsGuard() { docs_release(d); }
    lime_docs *take() { lime_docs *r = d; d = nullptr; return r; }
};
struct ListsGuard {                                      // the lists of a sample's collections
    lime_lists *l[4] = {nullptr, nullptr, nullptr, nullptr};
    ~ListsGuard() { for (lime_lists *x : l) lime_lists_free(x); }
};
struct PinnedPair {                                      // two pinned staging buffers and the events that say when a copy out of them is done
    void *buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~PinnedPair() { for (int k = 0; k < 2; ++k) { if (ev[k]) (void)hipEventDestroy(ev[k]); if (buf[k]) (void)hipHostFree(buf[k]); } }
};
struct FileGuard { FILE *f = nullptr; ~FileGuard() { if (f) fclose(f); } };
constexpr size_t STAGE_BYTES = 8u << 20;
}

// a handle with room for n_text symbols and n_docs + 1 offsets, nothing in them yet
static int docs_new(lime_ctx *c, const char *who, uint32_t n_docs, uint64_t n_text, DocsGuard &dg)
{
    lime_docs *d = new (std::nothrow) lime_docs();
    if (!d) return fail(LIME_ERR_NOMEM, "%s: out of host memory", who);
    d->ctx = c; d->n_docs = n_docs; d->n_text = n_text;
    c->docs.push_back(d);
    dg.d = d;
    int rc;
    if ((rc = d->text.acquire((size_t)n_text + 16)) || (rc = d->doc_off.acquire((size_t)n_docs + 1)))
        return fail(rc, "%s: no device memory for %llu symbols in %u documents: %s", who, (unsigned long long)n_text, n_docs, lime_last_error());
    return LIME_OK;
}

static int check_input_size(const char *who, uint64_t n)
{
    if (n > 0xFFFFFFFFull)
        return fail(LIME_ERR_ARG, "%s: %llu bytes of input; the parser counts in 32 bits (at most 2^32 - 1 bytes, and the builder indexes no more)", who,
                    (unsigned long long)n);
    return LIME_OK;
}

// d_bytes[0 .. n) -> a handle; the parse's scratch (24 bytes per block of LIME_FASTA_BLOCK input bytes + rocPRIM's) goes back before this returns
int lime_host::docs_parse_fasta_dev(lime_ctx *c, const char *who, const uint8_t *d_bytes, uint64_t n, hipStream_t st, lime_docs **out)
{
    const uint32_t nb = (uint32_t)((n + LIME_FASTA_BLOCK - 1) / LIME_FASTA_BLOCK);
    uint32_t totals[2] = {0, 0};                         // kept bytes, header starts
    WordScratch scratch;
    uint32_t *cum_lf = nullptr, *off_keep = nullptr, *off_hdr = nullptr, *first_hdr = nullptr;
    if (nb) {
        size_t t_max = 0, t_sum = 0;
        HIP_TRY(idx_scan_max(nullptr, &t_max, nullptr, nullptr, nb, st));
        HIP_TRY(idx_scan_sum(nullptr, &t_sum, nullptr, nullptr, (size_t)nb + 1, false, st));
        size_t tmp_bytes = std::max(t_max, t_sum);
        int rc = scratch.alloc(6, nb, tmp_bytes);
        if (rc) return fail(rc, "%s: no device memory for the parse of %llu bytes: %s", who, (unsigned long long)n, lime_last_error());
        uint32_t *last_lf = scratch.words(0);
        cum_lf = scratch.words(1);
        uint32_t *cnt_keep = scratch.words(2), *cnt_hdr = scratch.words(3);  // kept bytes, then header starts: each with a 0 behind the last block's
        off_keep = scratch.words(4); off_hdr = scratch.words(5);
        first_hdr = (uint32_t *)scratch.cell();
        void *tmp = scratch.tmp();
        HIP_TRY(hipMemsetAsync(cnt_keep, 0, 2 * scratch.stride, st));
        HIP_TRY(hipMemsetAsync(first_hdr, 0xFF, 4, st));
        fa_launch_lines(d_bytes, n, nb, last_lf, first_hdr, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(idx_scan_max(tmp, &tmp_bytes, last_lf, cum_lf, nb, st));
        fa_launch_count(d_bytes, n, nb, cum_lf, first_hdr, cnt_keep, cnt_hdr, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(idx_scan_sum(tmp, &tmp_bytes, cnt_keep, off_keep, (size_t)nb + 1, false, st));
        HIP_TRY(idx_scan_sum(tmp, &tmp_bytes, cnt_hdr, off_hdr, (size_t)nb + 1, false, st));
        HIP_TRY(hipMemcpyAsync(&totals[0], off_keep + nb, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&totals[1], off_hdr + nb, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));               // (the totals size the handle)
    }
    DocsGuard dg;
    int rc = docs_new(c, who, totals[1], totals[0], dg); if (rc) return rc;
    if (nb) {
        fa_launch_write(d_bytes, n, nb, cum_lf, first_hdr, off_keep, off_hdr, dg.d->text.p, dg.d->doc_off.p, st);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(dg.d->doc_off.p, 0, 8, st));
    }
    HIP_TRY(hipStreamSynchronize(st));                   // (the scratch goes back when this returns)
    *out = dg.take();
    return LIME_OK;
}

// the same for four-line FASTQ: 24 bytes per block + rocPRIM's + one error word.  The error word comes back with the copy the write pass
// is waited for anyway: two synchronisations, like parse_dev.  line_base: the lines in front of d_bytes[0] (a batch of lime_seq_reader), added to
// the line a refusal names
// with_qual: the quality bytes too, by a fourth pass (lime_fqtrim_kernel.hip) into n_keep + 16 bytes of which only the first n_keep are written
int lime_host::docs_parse_fastq_dev(lime_ctx *c, const char *who, const uint8_t *d_bytes, uint64_t n, uint64_t line_base, hipStream_t st, lime_docs **out,
                                    bool with_qual)
{
    static const char *const reason[4] = {"record does not start with '@'", "separator line does not start with '+'",
                                          "quality length differs from sequence length", "truncated record"};
    const uint32_t nb = (uint32_t)((n + LIME_FASTA_BLOCK - 1) / LIME_FASTA_BLOCK);
    uint32_t n_keep = 0, n_lines = 0;
    uint64_t err_word = ~0ull;                           // line * 4 + reason of the lowest offence
    WordScratch scratch;
    uint32_t *line0 = nullptr, *off_keep = nullptr, *off_diff = nullptr;
    uint64_t *err = nullptr;
    if (nb) {
        size_t tmp_bytes = 0;
        HIP_TRY(idx_scan_sum(nullptr, &tmp_bytes, nullptr, nullptr, (size_t)nb + 1, false, st));
        int rc = scratch.alloc(6, nb, tmp_bytes);
        if (rc) return fail(rc, "%s: no device memory for the parse of %llu bytes: %s", who, (unsigned long long)n, lime_last_error());
        // '\n', kept bytes, kept minus quality bytes: each with a 0 behind the last block's
        uint32_t *cnt_lf = scratch.words(0), *cnt_keep = scratch.words(1), *cnt_diff = scratch.words(2);
        line0 = scratch.words(3); off_keep = scratch.words(4); off_diff = scratch.words(5);
        err = (uint64_t *)scratch.cell();                // the error word, then n_lines
        uint32_t *d_lines = (uint32_t *)(err + 1);
        void *tmp = scratch.tmp();
        HIP_TRY(hipMemsetAsync(cnt_lf, 0, 3 * scratch.stride, st));
        HIP_TRY(hipMemsetAsync(err, 0xFF, 8, st));
        fq_launch_lines(d_bytes, n, nb, cnt_lf, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(idx_scan_sum(tmp, &tmp_bytes, cnt_lf, line0, (size_t)nb + 1, false, st));
        fq_launch_count(d_bytes, n, nb, line0, cnt_keep, cnt_diff, err, d_lines, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(idx_scan_sum(tmp, &tmp_bytes, cnt_keep, off_keep, (size_t)nb + 1, false, st));
        HIP_TRY(idx_scan_sum(tmp, &tmp_bytes, cnt_diff, off_diff, (size_t)nb + 1, false, st));
        HIP_TRY(hipMemcpyAsync(&n_keep, off_keep + nb, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&n_lines, d_lines, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));               // (the totals size the handle)
    }
    DocsGuard dg;
    int rc = docs_new(c, who, n_lines / 4, n_keep, dg); if (rc) return rc;
    if (with_qual && (rc = dg.d->qual.acquire((size_t)n_keep + 16)))
        return fail(rc, "%s: no device memory for %u quality bytes: %s", who, n_keep, lime_last_error());
    if (nb) {
        fq_launch_write(d_bytes, n, nb, line0, off_keep, off_diff, n_lines / 4, dg.d->text.p, dg.d->doc_off.p, err, st);
        HIP_TRY(hipGetLastError());
        if (with_qual) {
            fqt_launch_qual(d_bytes, n, nb, line0, off_keep, off_diff, dg.d->qual.p, n_keep, st);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(&err_word, err, 8, hipMemcpyDeviceToHost, st));
    } else {
        HIP_TRY(hipMemsetAsync(dg.d->doc_off.p, 0, 8, st));
    }
    HIP_TRY(hipStreamSynchronize(st));                   // (the scratch goes back when this returns)
    if (err_word != ~0ull) return fail(LIME_ERR_ARG, "%s: line %llu: %s", who, (unsigned long long)((err_word >> 2) + line_base), reason[err_word & 3u]);
    *out = dg.take();
    return LIME_OK;
}

static int parse_dev(lime_ctx *c, const char *who, const uint8_t *d_bytes, uint64_t n, hipStream_t st, lime_docs **out)
{
    return docs_parse_fasta_dev(c, who, d_bytes, n, st, out);
}
static int parse_fastq_dev(lime_ctx *c, const char *who, const uint8_t *d_bytes, uint64_t n, hipStream_t st, lime_docs **out)
{
    return docs_parse_fastq_dev(c, who, d_bytes, n, 0, st, out);
}

static int parse_fastq_qual_dev(lime_ctx *c, const char *who, const uint8_t *d_bytes, uint64_t n, hipStream_t st, lime_docs **out)
{
    return docs_parse_fastq_dev(c, who, d_bytes, n, 0, st, out, true);
}

typedef int (*ParseFn)(lime_ctx *, const char *, const uint8_t *, uint64_t, hipStream_t, lime_docs **);

static int from_bytes_dev(lime_ctx *c, const char *who, ParseFn parse, const uint8_t *d_bytes, uint64_t n, void *stream, lime_docs **out)
{
    if (!c || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    int rc = check_input_size(who, n); if (rc) return rc;
    if (n && !d_bytes) return fail(LIME_ERR_ARG, "%s: NULL array", who);
    if ((rc = check_ctx(c, who))) return rc;
    return parse(c, who, d_bytes, n, (hipStream_t)stream, out);
}

static int from_bytes(lime_ctx *c, const char *who, ParseFn parse, const uint8_t *bytes, uint64_t n, lime_docs **out)
{
    if (!c || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    int rc = check_input_size(who, n); if (rc) return rc;
    if (n && !bytes) return fail(LIME_ERR_ARG, "%s: NULL array", who);
    if ((rc = check_ctx(c, who))) return rc;
    DevBuf raw;
    if ((rc = raw.upload(bytes, (size_t)n))) return rc;
    return parse(c, who, (const uint8_t *)raw.p, n, nullptr, out);       // (raw goes back when this returns)
}

static int from_path(lime_ctx *c, const char *who, ParseFn parse, const char *path, lime_docs **out)
{
    if (!c || !path || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    FileGuard fg; fg.f = fopen(path, "rb");
    if (!fg.f) return fail(LIME_ERR_IO, "%s: cannot open %s", who, path);
    if (fseeko(fg.f, 0, SEEK_END) != 0) return fail(LIME_ERR_IO, "%s: cannot seek in %s", who, path);
    const off_t size = ftello(fg.f);
    if (size < 0 || fseeko(fg.f, 0, SEEK_SET) != 0) return fail(LIME_ERR_IO, "%s: cannot seek in %s", who, path);
    int rc = check_input_size(who, (uint64_t)size); if (rc) return rc;
    if ((rc = check_ctx(c, who))) return rc;
    DevBuf raw;
    if ((rc = raw.alloc((size_t)size + 16))) return fail(rc, "%s: no device memory for the %lld bytes of %s: %s", who, (long long)size, path, lime_last_error());
    // the file through two pinned buffers: one is read into while the other one's copy runs
    PinnedPair pin;
    const size_t stage = (size_t)std::min<uint64_t>(STAGE_BYTES, (uint64_t)size);
    uint64_t n = 0;
    for (int k = 0; (uint64_t)size > n; k ^= 1) {
        if (!pin.buf[k]) { HIP_TRY(hipHostMalloc(&pin.buf[k], stage)); HIP_TRY(hipEventCreateWithFlags(&pin.ev[k], hipEventDisableTiming)); }
        else HIP_TRY(hipEventSynchronize(pin.ev[k]));
        const size_t want = (size_t)std::min<uint64_t>(stage, (uint64_t)size - n);
        const size_t got = fread(pin.buf[k], 1, want, fg.f);
        if (got != want) return fail(LIME_ERR_IO, "%s: cannot read %s (%llu of %lld bytes)", who, path, (unsigned long long)(n + got), (long long)size);
        HIP_TRY(hipMemcpyAsync((uint8_t *)raw.p + n, pin.buf[k], got, hipMemcpyHostToDevice, nullptr));
        HIP_TRY(hipEventRecord(pin.ev[k], nullptr));
        n += got;
    }
    return parse(c, who, (const uint8_t *)raw.p, n, nullptr, out);       // synchronises: the copies are done before the buffers go
}

extern "C" int lime_docs_from_bytes_dev(lime_ctx *c, const uint8_t *d_bytes, uint64_t n, void *stream, lime_docs **out)
{
    return from_bytes_dev(c, "lime_docs_from_bytes_dev", parse_dev, d_bytes, n, stream, out);
}
extern "C" int lime_docs_from_bytes(lime_ctx *c, const uint8_t *bytes, uint64_t n, lime_docs **out) { return from_bytes(c, "lime_docs_from_bytes", parse_dev, bytes, n, out); }
extern "C" int lime_docs_from_fasta(lime_ctx *c, const char *path, lime_docs **out) { return from_path(c, "lime_docs_from_fasta", parse_dev, path, out); }

extern "C" int lime_docs_from_fastq_bytes_dev(lime_ctx *c, const uint8_t *d_bytes, uint64_t n, void *stream, lime_docs **out)
{
    return from_bytes_dev(c, "lime_docs_from_fastq_bytes_dev", parse_fastq_dev, d_bytes, n, stream, out);
}
extern "C" int lime_docs_from_fastq_bytes(lime_ctx *c, const uint8_t *bytes, uint64_t n, lime_docs **out)
{
    return from_bytes(c, "lime_docs_from_fastq_bytes", parse_fastq_dev, bytes, n, out);
}
extern "C" int lime_docs_from_fastq(lime_ctx *c, const char *path, lime_docs **out) { return from_path(c, "lime_docs_from_fastq", parse_fastq_dev, path, out); }

extern "C" int lime_docs_from_fastq_qual_bytes_dev(lime_ctx *c, const uint8_t *d_bytes, uint64_t n, void *stream, lime_docs **out)
{
    return from_bytes_dev(c, "lime_docs_from_fastq_qual_bytes_dev", parse_fastq_qual_dev, d_bytes, n, stream, out);
}
extern "C" int lime_docs_from_fastq_qual_bytes(lime_ctx *c, const uint8_t *bytes, uint64_t n, lime_docs **out)
{
    return from_bytes(c, "lime_docs_from_fastq_qual_bytes", parse_fastq_qual_dev, bytes, n, out);
}
extern "C" int lime_docs_from_fastq_qual(lime_ctx *c, const char *path, lime_docs **out)
{
    return from_path(c, "lime_docs_from_fastq_qual", parse_fastq_qual_dev, path, out);
}

// the one place a sequence file's format is decided (lime_seq_format: the first byte)
extern "C" int lime_docs_from_file(lime_ctx *c, const char *path, lime_docs **out)
{
    const char *who = "lime_docs_from_file";
    if (!c || !path || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    int format = 0;
    if (lime_seq_format(path, &format) != LIME_OK) return fail(LIME_ERR_IO, "%s: cannot open %s", who, path);
    return format == 1 ? lime_docs_from_fastq(c, path, out) : lime_docs_from_fasta(c, path, out);
}

extern "C" int lime_docs_from_arrays_dev(lime_ctx *c, const uint8_t *d_text, const uint64_t *d_doc_off, uint32_t n_docs, uint64_t n_text,
                                         void *stream, lime_docs **out)
{
    const char *who = "lime_docs_from_arrays_dev";
    if (!c || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    if (n_text > 0xFFFFFFFFull || n_text + n_docs > 0xFFFFFFFFull)
        return fail(LIME_ERR_ARG, "%s: %llu symbols + %u terminators exceed 2^32 - 1 positions", who, (unsigned long long)n_text, n_docs);
    if (!n_docs && n_text) return fail(LIME_ERR_ARG, "%s: %llu symbols in no document", who, (unsigned long long)n_text);
    if (!d_doc_off || (n_text && !d_text)) return fail(LIME_ERR_ARG, "%s: NULL array", who);
    int rc = check_ctx(c, who); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    DevBuf err;
    if ((rc = err.alloc(16))) return rc;
    HIP_TRY(hipMemsetAsync(err.p, 0, 4, st));
    fa_launch_check_off(d_doc_off, n_docs, n_text, (uint32_t *)err.p, st);
    HIP_TRY(hipGetLastError());
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, err.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(LIME_ERR_ARG, "%s: doc_off must start at 0, never decrease and end at n_text (%llu)", who, (unsigned long long)n_text);
    DocsGuard dg;
    if ((rc = docs_new(c, who, n_docs, n_text, dg))) return rc;
    HIP_TRY(hipMemcpyAsync(dg.d->doc_off.p, d_doc_off, ((size_t)n_docs + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (n_text) HIP_TRY(hipMemcpyAsync(dg.d->text.p, d_text, (size_t)n_text, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out = dg.take();
    return LIME_OK;
}

extern "C" int lime_docs_revcomp(lime_ctx *c, const lime_docs *in, void *stream, lime_docs **out)
{
    const char *who = "lime_docs_revcomp";
    if (!c || !in || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    if (in->ctx != c) return fail(LIME_ERR_ARG, "%s: the documents belong to another context", who);
    int rc = check_ctx(c, who); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    DocsGuard dg;
    if ((rc = docs_new(c, who, in->n_docs, in->n_text, dg))) return rc;
    HIP_TRY(hipMemcpyAsync(dg.d->doc_off.p, in->doc_off.p, ((size_t)in->n_docs + 1) * 8, hipMemcpyDeviceToDevice, st));
    fa_launch_revcomp(in->text.p, in->doc_off.p, in->n_docs, in->n_text, dg.d->text.p, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    *out = dg.take();
    return LIME_OK;
}

extern "C" int lime_docs_info(const lime_docs *d, uint32_t *n_docs, uint64_t *n_text)
{
    if (!d) return fail(LIME_ERR_ARG, "lime_docs_info: the documents are NULL");
    if (n_docs) *n_docs = d->n_docs;
    if (n_text) *n_text = d->n_text;
    return LIME_OK;
}

extern "C" int lime_docs_device(const lime_docs *d, const uint8_t **d_text, const uint64_t **d_doc_off)
{
    if (!d) return fail(LIME_ERR_ARG, "lime_docs_device: the documents are NULL");
    if (d_text) *d_text = d->text.p;
    if (d_doc_off) *d_doc_off = d->doc_off.p;
    return LIME_OK;
}

extern "C" int lime_docs_get(const lime_docs *d, uint8_t *text, uint64_t *doc_off)
{
    const char *who = "lime_docs_get";
    if (!d) return fail(LIME_ERR_ARG, "%s: the documents are NULL", who);
    int rc = check_ctx(d->ctx, who); if (rc) return rc;
    if (text && d->n_text && (rc = d2h_pageable(d->ctx, text, d->text.p, (size_t)d->n_text, nullptr))) return rc;
    if (doc_off && (rc = d2h_pageable(d->ctx, doc_off, d->doc_off.p, ((size_t)d->n_docs + 1) * 8, nullptr))) return rc;
    return LIME_OK;
}

extern "C" int lime_docs_qual_device(const lime_docs *d, const uint8_t **d_qual)
{
    if (!d || !d_qual) return fail(LIME_ERR_ARG, "lime_docs_qual_device: NULL argument");
    *d_qual = d->qual.p;                                 // (NULL: documents without qualities)
    return LIME_OK;
}

extern "C" int lime_docs_get_qual(const lime_docs *d, uint8_t *qual)
{
    const char *who = "lime_docs_get_qual";
    if (!d) return fail(LIME_ERR_ARG, "%s: the documents are NULL", who);
    if (!d->qual.p) return fail(LIME_ERR_ARG, "%s: the documents hold no qualities (lime_docs_from_fastq_qual* keeps them)", who);
    int rc = check_ctx(d->ctx, who); if (rc) return rc;
    if (qual && d->n_text && (rc = d2h_pageable(d->ctx, qual, d->qual.p, (size_t)d->n_text, nullptr))) return rc;
    return LIME_OK;
}

// ---- the quality trim (lime_fqtrim_kernel.hip: k_trim_bounds, k_trim_copy) and the adapter trim (lime_adapter_kernel.hip: k_adapter_bounds) ----
// Scratch: 12 bytes per read (lo, length, new offset) + rocPRIM's + the counter cell (two counters for a trim, five for the read filter
// further down), given back before either returns.  The new lengths' total sizes the handle: two synchronisations, like the parse
namespace {
struct TrimScratch : WordScratch {                       // what a bounds kernel fills and trim_finish reads
    uint32_t *lo32() const { return words(0); }
    uint32_t *len32() const { return words(1); }
    uint32_t *new_off() const { return words(2); }
    uint64_t *d_counts() const { return (uint64_t *)cell(); }
};
}

// nd >= 1 reads: the arrays, with the 0 behind the last read's length and the n_counts counters cleared
static int trim_begin(const char *who, uint32_t nd, hipStream_t st, TrimScratch &ts, uint32_t n_counts = 2)
{
    size_t tmp_bytes = 0;
    HIP_TRY(idx_scan_sum(nullptr, &tmp_bytes, nullptr, nullptr, (size_t)nd + 1, false, st));
    int rc = ts.alloc(3, nd, tmp_bytes);
    if (rc) return fail(rc, "%s: no device memory for the trim of %u reads: %s", who, nd, lime_last_error());
    HIP_TRY(hipMemsetAsync(ts.len32() + nd, 0, 4, st));  // (the 0 behind the last read's length: the sum's last entry is the total)
    HIP_TRY(hipMemsetAsync(ts.d_counts(), 0, 8 * n_counts, st));
    return LIME_OK;
}

// behind a bounds kernel's launch (none for no reads): the prefix sum, the total, the handle and the copy; -> counts[0 .. n_counts) as the
// kernel left them in the counter cell (zeros for no reads) and *symbols_out
static int trim_finish_counts(lime_ctx *c, const char *who, const lime_docs *docs, TrimScratch &ts, hipStream_t st, lime_docs **out, uint64_t *counts,
                              uint32_t n_counts, uint64_t *symbols_out)
{
    const uint32_t nd = docs->n_docs;
    uint32_t n_out = 0;
    memset(counts, 0, 8 * n_counts);
    if (nd) {
        HIP_TRY(hipGetLastError());
        HIP_TRY(idx_scan_sum(ts.tmp(), &ts.tmp_bytes, ts.len32(), ts.new_off(), (size_t)nd + 1, false, st));
        HIP_TRY(hipMemcpyAsync(&n_out, ts.new_off() + nd, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(counts, ts.d_counts(), 8 * n_counts, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));               // (the total sizes the handle)
    }
    DocsGuard dg;
    int rc = docs_new(c, who, nd, n_out, dg); if (rc) return rc;
    if (nd) {
        fqt_launch_copy(docs->text.p, docs->doc_off.p, nd, ts.lo32(), ts.len32(), ts.new_off(), dg.d->text.p, dg.d->doc_off.p, st);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(dg.d->doc_off.p, 0, 8, st));
    }
    HIP_TRY(hipStreamSynchronize(st));                   // (the scratch goes back when the caller returns)
    *symbols_out = n_out;
    *out = dg.take();
    return LIME_OK;
}

// the same for the two trims, whose kernels count the reads changed and the reads emptied
static int trim_finish(lime_ctx *c, const char *who, const lime_docs *docs, TrimScratch &ts, hipStream_t st, lime_docs **out, lime_trim_info_t *info)
{
    lime_trim_info_t ti = {docs->n_docs, 0, 0, docs->n_text, 0};
    uint64_t counts[2];
    int rc = trim_finish_counts(c, who, docs, ts, st, out, counts, 2, &ti.symbols_out); if (rc) return rc;
    ti.n_changed = counts[0]; ti.n_empty = counts[1];
    if (info) *info = ti;
    return LIME_OK;
}

// lime_docs_trim_dev without its argument checks (the three stages' impl functions are called by their public wrappers and by docs_stages)
static int docs_trim_impl(lime_ctx *c, const char *who, const lime_docs *docs, uint32_t q5, uint32_t q3, hipStream_t st, lime_docs **out, lime_trim_info_t *info)
{
    const uint32_t nd = docs->n_docs;
    TrimScratch ts;
    if (nd) {
        int rc = trim_begin(who, nd, st, ts); if (rc) return rc;
        fqt_launch_bounds(docs->qual.p, docs->doc_off.p, nd, q5, q3, ts.lo32(), ts.len32(), ts.d_counts(), st);
    }
    return trim_finish(c, who, docs, ts, st, out, info);
}

// the adapter's refusals, shared by lime_adapter_trim's callers on the device side; -> masks[b]: bit j set where symbol j is "ACGT"[b]
int lime_host::adapter_masks(const char *who, const uint8_t *adapter, uint32_t m, uint32_t min_overlap, uint32_t max_err_pct, uint64_t masks[4])
{
    masks[0] = masks[1] = masks[2] = masks[3] = 0;
    if (!adapter) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (!m || m > 64) return fail(LIME_ERR_ARG, "%s: an adapter of %u symbols; it holds 1 .. 64", who, m);
    for (uint32_t j = 0; j < m; ++j) {
        const char *at = static_cast<const char *>(memchr("ACGT", adapter[j] & 0xDF, 4));
        if (!at) return fail(LIME_ERR_ARG, "%s: adapter symbol %u is byte %u; an adapter holds A, C, G and T only", who, j, (unsigned)adapter[j]);
        masks[at - "ACGT"] |= 1ull << j;
    }
    if (!min_overlap || min_overlap > m) return fail(LIME_ERR_ARG, "%s: a minimum overlap of %u with an adapter of %u symbols; it is 1 .. %u", who, min_overlap, m, m);
    if (max_err_pct > 50) return fail(LIME_ERR_ARG, "%s: an error rate of %u percent; it is 0 .. 50", who, max_err_pct);
    return LIME_OK;
}

static int docs_adapter_impl(lime_ctx *c, const char *who, const lime_docs *docs, const uint64_t masks[4], uint32_t m, uint32_t min_overlap,
                             uint32_t max_err_pct, hipStream_t st, lime_docs **out, lime_trim_info_t *info)
{
    const uint32_t nd = docs->n_docs;
    TrimScratch ts;
    if (nd) {
        int rc = trim_begin(who, nd, st, ts); if (rc) return rc;
        ad_launch_bounds(docs->text.p, docs->doc_off.p, nd, masks, m, min_overlap, max_err_pct, ts.lo32(), ts.len32(), ts.d_counts(), st);
    }
    return trim_finish(c, who, docs, ts, st, out, info);
}

extern "C" int lime_docs_trim_adapter_dev(lime_ctx *c, const lime_docs *docs, const uint8_t *adapter, uint32_t m, uint32_t min_overlap, uint32_t max_err_pct,
                                          void *stream, lime_docs **out, lime_trim_info_t *info)
{
    const char *who = "lime_docs_trim_adapter_dev";
    if (info) memset(info, 0, sizeof *info);
    if (out) *out = nullptr;
    if (!c || !docs || !adapter || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (docs->ctx != c) return fail(LIME_ERR_ARG, "%s: the documents belong to another context", who);
    uint64_t masks[4];
    int rc = adapter_masks(who, adapter, m, min_overlap, max_err_pct, masks); if (rc) return rc;
    if ((rc = check_ctx(c, who))) return rc;
    return docs_adapter_impl(c, who, docs, masks, m, min_overlap, max_err_pct, (hipStream_t)stream, out, info);
}

// ---- the read filter (lime_filter_kernel.hip: k_filter_bounds), through the trims' prefix sum and copy ----
static int docs_filter_impl(lime_ctx *c, const char *who, const lime_docs *docs, const lime_filter_t *f, hipStream_t st, lime_docs **out, lime_filter_info_t *info)
{
    const uint32_t nd = docs->n_docs;
    TrimScratch ts;
    if (nd) {
        int rc = trim_begin(who, nd, st, ts, 5); if (rc) return rc;
        fl_launch_bounds(docs->text.p, docs->doc_off.p, nd, f, ts.lo32(), ts.len32(), ts.d_counts(), st);
    }
    lime_filter_info_t fi = {nd, 0, 0, 0, 0, 0, docs->n_text, 0};
    uint64_t counts[5];
    int rc = trim_finish_counts(c, who, docs, ts, st, out, counts, 5, &fi.symbols_out); if (rc) return rc;
    fi.n_polyx = counts[0]; fi.n_capped = counts[1]; fi.n_short = counts[2]; fi.n_many_n = counts[3]; fi.n_low_complexity = counts[4];
    if (info) *info = fi;
    return LIME_OK;
}

extern "C" int lime_docs_filter_dev(lime_ctx *c, const lime_docs *docs, const lime_filter_t *f, void *stream, lime_docs **out, lime_filter_info_t *info)
{
    const char *who = "lime_docs_filter_dev";
    if (info) memset(info, 0, sizeof *info);
    if (out) *out = nullptr;
    if (!c || !docs || !f || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (docs->ctx != c) return fail(LIME_ERR_ARG, "%s: the documents belong to another context", who);
    int rc = filter_check(who, f); if (rc) return rc;
    if ((rc = check_ctx(c, who))) return rc;
    return docs_filter_impl(c, who, docs, f, (hipStream_t)stream, out, info);
}

// ---- per-position statistics (lime_qc_kernel.hip: k_qc_reads): the tables cleared on the device, the kernel, the copy back, the sum ----
static int docs_qc_impl(lime_ctx *c, const char *who, const lime_docs *docs, uint32_t n_pos, hipStream_t st, uint64_t *tables)
{
    (void)c;
    const uint32_t nd = docs->n_docs;
    if (!nd) return LIME_OK;
    const size_t n_words = LIME_QC_WORDS(n_pos);
    DevBuf d_tables;
    int rc = d_tables.alloc(n_words * 8);
    if (rc) return fail(rc, "%s: no device memory for the tables of %u positions: %s", who, n_pos, lime_last_error());
    std::vector<uint64_t> part(n_words);
    HIP_TRY(hipMemsetAsync(d_tables.p, 0, n_words * 8, st));
    qc_launch_reads(docs->text.p, docs->qual.p, docs->doc_off.p, nd, n_pos, static_cast<uint64_t *>(d_tables.p), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(part.data(), d_tables.p, n_words * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                   // (the tables go back when this returns)
    for (size_t k = 0; k < n_words; ++k) tables[k] += part[k];
    return LIME_OK;
}

extern "C" int lime_docs_qc_dev(lime_ctx *c, const lime_docs *docs, uint32_t n_pos, void *stream, uint64_t *tables)
{
    const char *who = "lime_docs_qc_dev";
    if (!c || !docs || !tables) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (docs->ctx != c) return fail(LIME_ERR_ARG, "%s: the documents belong to another context", who);
    if (!n_pos || n_pos > LIME_QC_MAX_POS) return fail(LIME_ERR_ARG, "%s: %u positions; there are 1 .. %u", who, n_pos, LIME_QC_MAX_POS);
    int rc = check_ctx(c, who); if (rc) return rc;
    return docs_qc_impl(c, who, docs, n_pos, (hipStream_t)stream, tables);
}

// ---- the overlap cut (lime_overlap_kernel.hip: k_overlap_bounds): one kernel over the pairs, then per mate the trims' prefix sum and copy ----
// The two counters stand in mate 1's cell; mate 2's cell stays as trim_begin cleared it
int lime_host::docs_overlap_impl(lime_ctx *c, const char *who, const lime_docs *docs1, const lime_docs *docs2, uint32_t min_overlap, uint32_t max_err_pct,
                                 uint32_t *d_insert, hipStream_t st, lime_docs **out1, lime_docs **out2, lime_overlap_info_t *info)
{
    const uint32_t nd = docs1->n_docs;
    TrimScratch ts1, ts2;
    if (nd) {
        int rc = trim_begin(who, nd, st, ts1); if (rc) return rc;
        if ((rc = trim_begin(who, nd, st, ts2))) return rc;
        ov_launch_bounds(docs1->text.p, docs1->doc_off.p, docs2->text.p, docs2->doc_off.p, nd, min_overlap, max_err_pct, ts1.lo32(), ts1.len32(), ts2.lo32(),
                         ts2.len32(), d_insert, ts1.d_counts(), st);
    }
    lime_overlap_info_t oi = {nd, 0, 0, docs1->n_text + docs2->n_text, 0};
    uint64_t counts[2], none[2], sym1 = 0, sym2 = 0;
    DocsGuard g1;
    int rc = trim_finish_counts(c, who, docs1, ts1, st, &g1.d, counts, 2, &sym1); if (rc) return rc;
    lime_docs *o2 = nullptr;
    if ((rc = trim_finish_counts(c, who, docs2, ts2, st, &o2, none, 2, &sym2))) return rc;       // (g1 gives mate 1's documents back)
    oi.n_overlap = counts[0]; oi.n_cut = counts[1]; oi.symbols_out = sym1 + sym2;
    *out1 = g1.take(); *out2 = o2;
    if (info) *info = oi;
    return LIME_OK;
}

extern "C" int lime_docs_trim_overlap_dev(lime_ctx *c, const lime_docs *docs1, const lime_docs *docs2, uint32_t min_overlap, uint32_t max_err_pct,
                                          uint32_t *d_insert, void *stream, lime_docs **out1, lime_docs **out2, lime_overlap_info_t *info)
{
    const char *who = "lime_docs_trim_overlap_dev";
    if (info) memset(info, 0, sizeof *info);
    if (out1) *out1 = nullptr;
    if (out2) *out2 = nullptr;
    if (!c || !docs1 || !docs2 || !out1 || !out2) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (docs1->ctx != c || docs2->ctx != c) return fail(LIME_ERR_ARG, "%s: the documents belong to another context", who);
    if (docs1->n_docs != docs2->n_docs)
        return fail(LIME_ERR_ARG, "%s: the mates hold different numbers of reads (%u and %u)", who, docs1->n_docs, docs2->n_docs);
    int rc = overlap_check(who, min_overlap, max_err_pct); if (rc) return rc;
    if ((rc = check_ctx(c, who))) return rc;
    return docs_overlap_impl(c, who, docs1, docs2, min_overlap, max_err_pct, d_insert, (hipStream_t)stream, out1, out2, info);
}

extern "C" int lime_docs_trim_dev(lime_ctx *c, const lime_docs *docs, uint32_t q5, uint32_t q3, void *stream, lime_docs **out, lime_trim_info_t *info)
{
    const char *who = "lime_docs_trim_dev";
    if (info) memset(info, 0, sizeof *info);
    if (!c || !docs || !out) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    *out = nullptr;
    if (docs->ctx != c) return fail(LIME_ERR_ARG, "%s: the documents belong to another context", who);
    if (q5 > 93 || q3 > 93) return fail(LIME_ERR_ARG, "%s: cutoffs %u,%u; a Phred+33 quality is 0 .. 93", who, q5, q3);
    if (!docs->qual.p) return fail(LIME_ERR_ARG, "%s: the documents hold no qualities (lime_docs_from_fastq_qual* keeps them)", who);
    int rc = check_ctx(c, who); if (rc) return rc;
    return docs_trim_impl(c, who, docs, q5, q3, (hipStream_t)stream, out, info);
}

// ---- one mate's stages, in their one order (lime_reader.cpp runs every batch through this) ----
// The documents replaced by a stage's output and the stage's counts added to their sum; the input goes back either way (NULL behind a failure)
template <typename Info, typename Stage> static int through(lime_docs *&d, Info &sum, Stage stage)
{
    lime_docs *next = nullptr;
    Info info;
    const int rc = stage(d, &next, &info);
    lime_docs_free(d);
    d = next;
    if (!rc) add_info(sum, info);
    return rc;
}

// THE ORDER OF A MATE'S STAGES.  A batch as parsed (with its qualities where s.needs_qual()) becomes the batch as it is handed out:
//   1. the `before` tables (s.n_pos): the batch as parsed; qualities that were parsed for the tables alone go back here
//   2. the quality trim (s.trim): its output holds no qualities
//   3. the adapter trim (s.adapter): second, as an outside trimmer does it
//   4. the read filter (s.filter): what the trims left
// The overlap cut comes behind this, on the pair (next_pair_impl), and the `after` tables behind that (docs_count_out).  Every stage costs
// what its public call costs: no stage is fused with its neighbour and no bounds are composed to save a copy.
int lime_host::docs_stages(lime_ctx *c, const char *who, MateStages &s, lime_docs **docs)
{
    lime_docs *d = *docs;
    *docs = nullptr;
    int rc;
    if (s.n_pos) {
        if ((rc = docs_qc_impl(c, who, d, s.n_pos, nullptr, s.qc_raw.data()))) { lime_docs_free(d); return rc; }
        if (!s.trim) d->qual.release();
    }
    if (s.trim && (rc = through(d, s.trimmed, [&](const lime_docs *in, lime_docs **out, lime_trim_info_t *ti) {
                       return docs_trim_impl(c, who, in, s.q5, s.q3, nullptr, out, ti); }))) return rc;
    if (s.adapter && (rc = through(d, s.ad_trimmed, [&](const lime_docs *in, lime_docs **out, lime_trim_info_t *ti) {
                          return docs_adapter_impl(c, who, in, s.ad_masks, s.ad_m, s.ad_overlap, s.ad_err, nullptr, out, ti); }))) return rc;
    if (s.filter && (rc = through(d, s.filtered, [&](const lime_docs *in, lime_docs **out, lime_filter_info_t *fi) {
                         return docs_filter_impl(c, who, in, &s.fl, nullptr, out, fi); }))) return rc;
    *docs = d;
    return LIME_OK;
}

int lime_host::docs_count_out(lime_ctx *c, const char *who, MateStages &s, lime_docs **batch, lime_docs **other)
{
    if (!s.n_pos) return LIME_OK;
    const int rc = docs_qc_impl(c, who, *batch, s.n_pos, nullptr, s.qc_out.data());
    if (rc) { lime_docs_free(*batch); *batch = nullptr; }
    if (rc && other) { lime_docs_free(*other); *other = nullptr; }
    return rc;
}

extern "C" void lime_docs_free(lime_docs *d)
{
    if (!d) return;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(d->ctx->device);
    docs_release(d);
    (void)hipSetDevice(cur);
}

// ---- a norm per read from the documents' lengths (lime_readnorm_kernel.hip: k_rn_norms) ----------------------------------------------
int lime_host::docs_norms_impl(lime_ctx *c, const lime_docs *docs, uint32_t alpha, uint8_t *d_norms, hipStream_t st, uint32_t *n_long, uint32_t *first,
                               uint64_t *first_len)
{
    *n_long = 0; *first = 0; *first_len = 0;
    if (!docs->n_docs) return LIME_OK;
    DevBuf info;
    int rc = info.alloc(16); if (rc) return rc;
    const uint32_t init[2] = {0u, 0xFFFFFFFFu};
    uint32_t got[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(info.p, init, 8, hipMemcpyHostToDevice, st));
    launch_rn_norms(docs->doc_off.p, docs->n_docs, alpha, d_norms, (uint32_t *)info.p, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(got, info.p, 8, hipMemcpyDeviceToHost, st));      // the 8 bytes that come back
    HIP_TRY(hipStreamSynchronize(st));
    if (!got[0]) return LIME_OK;
    uint64_t off[2] = {0, 0};                                                // (a refusal only: the offending read's bounds)
    HIP_TRY(hipMemcpy(off, docs->doc_off.p + got[1], 16, hipMemcpyDeviceToHost));
    *n_long = got[0]; *first = got[1]; *first_len = off[1] - off[0];
    return LIME_OK;
}

extern "C" int lime_docs_norms_dev(lime_ctx *c, const lime_docs *docs, uint32_t alpha, uint8_t *d_norms, void *stream)
{
    const char *who = "lime_docs_norms_dev";
    if (!c || !docs) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (docs->ctx != c) return fail(LIME_ERR_ARG, "%s: the documents belong to another context", who);
    if (!alpha) return fail(LIME_ERR_ARG, "%s: alpha is 0", who);
    if (docs->n_docs && !d_norms) return fail(LIME_ERR_ARG, "%s: d_norms is NULL", who);
    int rc = check_ctx(c, who); if (rc) return rc;
    uint32_t n_long = 0, first = 0;
    uint64_t len = 0;
    if ((rc = docs_norms_impl(c, docs, alpha, d_norms, (hipStream_t)stream, &n_long, &first, &len))) return rc;
    if (n_long)
        return fail(LIME_ERR_ARG, "%s: read %u holds %llu symbols (and %u reads in all more than 255): a norm is a byte, as the cells are", who, first,
                    (unsigned long long)len, n_long);
    return LIME_OK;
}

// ---- a sample: documents -> verdicts -----------------------------------------------------------------------------------------
// The refusals about the genome side that lime_classify_sample[_shards]_dev and lime_classify_sample_stream[_shards] share, in two steps
// (the read sets' own come between them): the shards are there and of this context; then alpha, shards that agree on term and lcp_cap, a
// taxonomy of the shards' genomes in all, a cap the indexes can serve.  One shard: the texts of the calls that take one index.
int lime_host::sample_check_shards(const char *who, lime_ctx *c, uint32_t n_shards, const lime_gindex *const *shards)
{
    if (!n_shards) return fail(LIME_ERR_ARG, "%s: n_shards is 0", who);
    for (uint32_t s = 0; s < n_shards; ++s) {
        if (!shards[s]) return fail(LIME_ERR_ARG, "%s: index shard %u is NULL", who, s);
        if (shards[s]->ctx != c)
            return n_shards == 1 ? fail(LIME_ERR_ARG, "%s: the genome index belongs to another context", who)
                                 : fail(LIME_ERR_ARG, "%s: index shard %u belongs to another context", who, s);
    }
    return LIME_OK;
}
int lime_host::sample_check_rules(const char *who, uint32_t n_shards, const lime_gindex *const *shards, const lime_taxonomy *tx, uint32_t alpha,
                                  uint32_t lcp_cap, uint32_t *n_refs, uint32_t *cap_out)
{
    if (!alpha) return fail(LIME_ERR_ARG, "%s: alpha is 0", who);
    uint64_t total = 0;
    for (uint32_t s = 0; s < n_shards; ++s) {
        if (shards[s]->term != shards[0]->term || shards[s]->lcp_cap != shards[0]->lcp_cap)
            return fail(LIME_ERR_ARG, "%s: index shard %u was built with term %u and lcp_cap %u, shard 0 with term %u and lcp_cap %u", who, s,
                        (unsigned)shards[s]->term, shards[s]->lcp_cap, (unsigned)shards[0]->term, shards[0]->lcp_cap);
        total += shards[s]->n_docs;
    }
    if (total > 0xFFFFFFFFull) return fail(LIME_ERR_ARG, "%s: the shards hold %llu genomes; ids are 32 bits", who, (unsigned long long)total);
    if (!total || tx->n_targ != total)
        return n_shards == 1 ? fail(LIME_ERR_ARG, "%s: the taxonomy holds %u genomes, the index %u", who, tx->n_targ, (uint32_t)total)
                             : fail(LIME_ERR_ARG, "%s: the taxonomy holds %u genomes, the %u index shards %u", who, tx->n_targ, n_shards, (uint32_t)total);
    const uint32_t gi_cap = shards[0]->lcp_cap, cap = lcp_cap ? lcp_cap : gi_cap;     // 0: the index's own
    if (gi_cap && cap > gi_cap)
        return fail(LIME_ERR_ARG, "%s: lcp_cap %u cannot be served from an index built with lcp_cap %u (1 .. %u can)", who, cap, gi_cap, gi_cap);
    if (cap && cap < alpha) return fail(LIME_ERR_ARG, "%s: lcp values capped at %u cannot show clusters of alpha = %u", who, cap, alpha);
    *n_refs = (uint32_t)total; *cap_out = cap;
    return LIME_OK;
}

namespace {
struct PartsGuard {                                      // one collection's unfiltered lists, one per index shard
    std::vector<lime_lists *> l;
    ~PartsGuard() { release(); }
    void release() { for (lime_lists *&x : l) { lime_lists_free(x); x = nullptr; } }
};
}

// lime_classify_sample_dev (one shard: the calls it always made) and lime_classify_sample_shards_dev
int lime_host::classify_sample_at(const char *who, lime_ctx *c, uint32_t n_mates, const lime_docs *const *mates, uint32_t n_shards,
                                  const lime_gindex *const *shards, const lime_taxonomy *tx, uint32_t alpha, uint32_t norm, float beta, int use_ebwt,
                                  int binary, uint32_t lcp_cap, lime_verdict_t *verdicts, uint64_t counts[4], lime_stats_t *stats, void *stream,
                                  uint64_t read_base)
{
    uint64_t local[4];
    if (!counts) counts = local;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (!c) return fail(LIME_ERR_ARG, "%s: ctx is NULL", who);
    if (n_mates != 1 && n_mates != 2) return fail(LIME_ERR_ARG, "%s: n_mates is %u; a sample has 1 (single-end) or 2 (paired-end) read sets", who, n_mates);
    if (!mates || !shards || (n_shards == 1 && !shards[0]) || !tx || !verdicts) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    int rc = sample_check_shards(who, c, n_shards, shards); if (rc) return rc;
    for (uint32_t m = 0; m < n_mates; ++m) {
        if (!mates[m]) return fail(LIME_ERR_ARG, "%s: read set %u is NULL", who, m);
        if (mates[m]->ctx != c) return fail(LIME_ERR_ARG, "%s: read set %u belongs to another context", who, m);
        if (!mates[m]->n_docs) return fail(LIME_ERR_ARG, "%s: read set %u holds no documents", who, m);
        if (mates[m]->n_docs != mates[0]->n_docs)
            return fail(LIME_ERR_ARG, "%s: the read sets hold different numbers of reads (%u in set 0, %u in set %u)", who, mates[0]->n_docs, mates[m]->n_docs, m);
    }
    uint32_t n_refs = 0, cap = 0;
    if ((rc = sample_check_rules(who, n_shards, shards, tx, alpha, lcp_cap, &n_refs, &cap))) return rc;
    if ((rc = check_ctx(c, who))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_reads = mates[0]->n_docs, n_coll = 2 * n_mates;
    std::vector<uint32_t> id_base(n_shards), n_part(n_shards);
    for (uint32_t s = 0, at = 0; s < n_shards; ++s) { id_base[s] = at; n_part[s] = shards[s]->n_docs; at += shards[s]->n_docs; }

    // LIME_NORM_PER_READ: every mate's norms from its documents' lengths, before anything else is made (F and RC of a mate share them: a
    // reverse complement has its read's length); the lists are then made unfiltered and the test follows per read, for one shard or many
    const bool per_read = norm == LIME_NORM_PER_READ;
    DevBuf d_norms[2];
    for (uint32_t m = 0; m < n_mates && per_read; ++m) {
        if ((rc = d_norms[m].alloc((size_t)n_reads + 16))) return rc;
        uint32_t n_long = 0, first = 0;
        uint64_t len = 0;
        if ((rc = docs_norms_impl(c, mates[m], alpha, (uint8_t *)d_norms[m].p, st, &n_long, &first, &len))) return rc;
        if (n_long)
            return fail(LIME_ERR_ARG, "%s: read set %u: read %llu holds %llu symbols; a read normalised by its own length holds at most 255 (the cells are bytes)",
                        who, m, (unsigned long long)(read_base + first), (unsigned long long)len);
    }
    const bool whole = n_shards == 1 && !per_read;                          // the one list of a collection is made in one step
    const uint32_t list_norm = per_read ? 1u : norm;                        // (unfiltered lists: their own norm plays no part)

    ListsGuard lg;
    for (uint32_t k = 0; k < n_coll; ++k) {                                 // the script's order: F, F_RC, R, R_RC
        const lime_docs *src = mates[k >> 1];
        DocsGuard rev;                                                      // (the reverse complement goes back at the end of the round)
        if (k & 1u) {
            if ((rc = lime_docs_revcomp(c, src, stream, &rev.d))) return rc;
            src = rev.d;
        }
        PartsGuard parts;
        parts.l.assign(n_shards, nullptr);
        for (uint32_t s = 0; s < n_shards; ++s) {
            const lime_gindex *gi = shards[s];
            const uint64_t n = src->n_text + src->n_docs + gi->n();
            DevBuf ebwt, lcp, da;
            if ((use_ebwt && (rc = ebwt.alloc((size_t)n))) || (rc = lcp.alloc((size_t)n * 4)) || (rc = da.alloc((size_t)n * 4)))
                return fail(rc, "%s: no device memory for the arrays of %llu positions: %s", who, (unsigned long long)n, lime_last_error());
            if ((rc = lime_merge_index_dev(c, src->text.p, src->doc_off.p, src->n_docs, src->n_text, gi, cap, (uint8_t *)ebwt.p, (uint32_t *)lcp.p,
                                           (uint32_t *)da.p, stream)))
                return rc;
            // one shard: the list itself.  More: every non-zero row (beta -1: pass[0] holds and such rows are empty); the test follows on the whole row
            lime_lists **dst = whole ? &lg.l[k] : &parts.l[s];
            if ((rc = lime_fused_choose_lists_dev(c, (const uint32_t *)lcp.p, (const uint32_t *)da.p, (const uint8_t *)ebwt.p, n, n_reads, gi->n_docs, alpha,
                                                  list_norm, whole ? beta : -1.0f, dst, stats ? &stats[(size_t)s * n_coll + k] : nullptr, stream)))
                return rc;
            HIP_TRY(hipStreamSynchronize(st));                              // (the arrays go back when the round ends)
        }
        if (per_read) {
            if ((rc = lime_lists_concat_norms_dev(c, n_shards, parts.l.data(), id_base.data(), n_part.data(), (const uint8_t *)d_norms[k >> 1].p, beta,
                                                  &lg.l[k], stream)))
                return rc;
        } else if (n_shards > 1) {
            if ((rc = lime_lists_concat_dev(c, n_shards, parts.l.data(), id_base.data(), n_part.data(), beta, &lg.l[k], stream))) return rc;
        }
    }
    return lime_classify_lists_dev(c, n_coll, lg.l, n_refs, tx, binary, verdicts, counts, stream);
}

extern "C" int lime_classify_sample_dev(lime_ctx *c, uint32_t n_mates, const lime_docs *const *mates, const lime_gindex *gi,
                                        const lime_taxonomy *tx, uint32_t alpha, uint32_t norm, float beta, int use_ebwt, int binary,
                                        uint32_t lcp_cap, lime_verdict_t *verdicts, uint64_t counts[4], lime_stats_t *stats, void *stream)
{
    return classify_sample_at("lime_classify_sample_dev", c, n_mates, mates, 1, &gi, tx, alpha, norm, beta, use_ebwt, binary, lcp_cap, verdicts, counts,
                              stats, stream, 0);
}

extern "C" int lime_classify_sample_shards_dev(lime_ctx *c, uint32_t n_mates, const lime_docs *const *mates, uint32_t n_shards,
                                               const lime_gindex *const *shards, const lime_taxonomy *tx, uint32_t alpha, uint32_t norm, float beta,
                                               int use_ebwt, int binary, uint32_t lcp_cap, lime_verdict_t *verdicts, uint64_t counts[4],
                                               lime_stats_t *stats, void *stream)
{
    return classify_sample_at("lime_classify_sample_shards_dev", c, n_mates, mates, n_shards, shards, tx, alpha, norm, beta, use_ebwt, binary, lcp_cap,
                              verdicts, counts, stats, stream, 0);
}

// ---- the genomes cut into index shards (pure host code) ------------------------------------------------------------------------
extern "C" int lime_gindex_shard_plan(const uint64_t *doc_off, uint32_t n_docs, uint64_t max_positions, uint32_t *first_doc, uint32_t cap,
                                      uint32_t *n_shards)
{
    const char *who = "lime_gindex_shard_plan";
    if (n_shards) *n_shards = 0;
    if (!doc_off || !first_doc || !n_shards) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (!max_positions) return fail(LIME_ERR_ARG, "%s: max_positions is 0", who);
    if (!cap) return fail(LIME_ERR_ARG, "%s: first_doc holds no entry", who);
    uint32_t ns = 0;
    uint64_t used = 0;
    first_doc[0] = 0;
    for (uint32_t d = 0; d < n_docs; ++d) {
        if (doc_off[d + 1] < doc_off[d]) return fail(LIME_ERR_ARG, "%s: doc_off decreases at genome %u", who, d);
        const uint64_t pos = doc_off[d + 1] - doc_off[d] + 1;              // its symbols and its terminator
        if (pos > max_positions)
            return fail(LIME_ERR_ARG, "%s: genome %u holds %llu positions, more than the %llu a shard may hold (a genome is not cut)", who, d,
                        (unsigned long long)pos, (unsigned long long)max_positions);
        if (d == 0 || used + pos > max_positions) {                         // this genome opens a shard
            if ((uint64_t)ns + 2 > cap)
                return fail(LIME_ERR_ARG, "%s: more than %u shards: first_doc holds %u entries (n_shards + 1 are written)", who, cap - 1, cap);
            first_doc[ns++] = d;
            used = 0;
        }
        used += pos;
    }
    first_doc[ns] = n_docs;
    *n_shards = ns;
    return LIME_OK;
}
