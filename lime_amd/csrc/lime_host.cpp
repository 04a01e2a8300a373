// lime_host.cpp -- readers/writers of the reference's on-disk formats.
// Pure host code, no device work; shared by the drop-in executables and the Python mirror.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <string>
#include <vector>

#include "lime_hip.h"

namespace lime_host __attribute__((visibility("hidden"))) {
int fail(int code, const char *fmt, ...);                 // lime_api.cpp: sets what lime_last_error() returns
int filter_check(const char *who, const lime_filter_t *f);        // below; lime_ctx.h declares it for the device side
int overlap_check(const char *who, uint32_t min_overlap, uint32_t max_err_pct);       // the same
}

namespace {
struct File {
    FILE *f;
    File(const char *path, const char *mode) : f(fopen(path, mode)) {}
    ~File() { if (f) fclose(f); }
    int close() { int r = f ? fclose(f) : -1; f = nullptr; return r; }
};
struct PairSim { float sim; uint32_t id; };   // pair_sim, Tools.h:95-98 (8 bytes)
}

// fileFasta.<alpha>.clrs: raw ElementCluster records (ClusterLCP.cpp:229-235)
extern "C" int lime_write_clrs(const char *path, const lime_cluster_t *clusters, uint64_t n)
{
    File o(path, "wb");
    if (!o.f) return LIME_ERR_IO;
    if (n && fwrite(clusters, sizeof(lime_cluster_t), n, o.f) != n) return LIME_ERR_IO;
    return o.close() ? LIME_ERR_IO : LIME_OK;
}

// 28-byte aux file, written field by field (ClusterLCP.cpp:304-308)
extern "C" int lime_write_aux(const char *path, uint32_t n_reads, uint32_t n_refs, uint32_t alpha,
                              uint64_t max_len, uint64_t n_clusters)
{
    File o(path, "wb");
    if (!o.f) return LIME_ERR_IO;
    size_t ok = fwrite(&n_reads, 4, 1, o.f) + fwrite(&n_refs, 4, 1, o.f) + fwrite(&alpha, 4, 1, o.f) +
                fwrite(&max_len, 8, 1, o.f) + fwrite(&n_clusters, 8, 1, o.f);
    if (ok != 5) return LIME_ERR_IO;
    return o.close() ? LIME_ERR_IO : LIME_OK;
}

extern "C" int lime_read_aux(const char *path, uint32_t *n_reads, uint32_t *n_refs, uint32_t *alpha,
                             uint64_t *max_len, uint64_t *n_clusters)
{
    File i(path, "rb");
    if (!i.f) return LIME_ERR_IO;
    size_t ok = fread(n_reads, 4, 1, i.f) + fread(n_refs, 4, 1, i.f) + fread(alpha, 4, 1, i.f) +
                fread(max_len, 8, 1, i.f) + fread(n_clusters, 8, 1, i.f);
    return ok == 5 ? LIME_OK : LIME_ERR_IO;
}

static uint8_t row_maximum(const uint8_t *row, uint32_t n)
{
    uint8_t m = 0;
    for (uint32_t j = 0; j < n; ++j) if (row[j] > m) m = row[j];
    return m;
}

// fileFasta.res.txt (BIN=0): ClusterBWT_DA.cpp:404-441.  A read is written iff
// float(max)/norm > beta (strict, in float); every read terminates its line.
extern "C" int lime_write_res_txt(const char *path, const uint8_t *sim, const uint8_t *row_max,
                                  uint32_t n_reads, uint32_t n_refs, uint32_t norm, float beta)
{
    if (norm == LIME_NORM_PER_READ) return LIME_ERR_ARG;      // (the .res files are written with one norm)
    File o(path, "w");
    if (!o.f) return LIME_ERR_IO;
    std::vector<char> buf(1 << 16);
    setvbuf(o.f, buf.data(), _IOFBF, buf.size());
    for (uint32_t r = 0; r < n_reads; ++r) {
        const uint8_t *row = sim + (size_t)r * n_refs;
        const uint8_t m = row_max ? row_max[r] : row_maximum(row, n_refs);
        const float top = static_cast<float>(m) / norm;
        if (top > beta) {
            fprintf(o.f, "%.5f", top);
            for (uint32_t j = 0; j < n_refs; ++j)
                if (row[j]) fprintf(o.f, "\t%u\t%.5f", j, static_cast<float>(row[j]) / norm);
        }
        fputc('\n', o.f);
    }
    return o.close() ? LIME_ERR_IO : LIME_OK;
}

// fileFasta.res.bin + .res.pos (BIN=1): ClusterBWT_DA.cpp:376-436.  .bin = 8-byte records:
// record 0 sentinel {0,0}; per passing read a header {max/norm, count} then count pairs
// {cell/norm, idRef}; .pos = one u64 per read: record index of its header, 0 if none.
extern "C" int lime_write_res_bin(const char *path_bin, const char *path_pos, const uint8_t *sim,
                                  const uint8_t *row_max, uint32_t n_reads, uint32_t n_refs,
                                  uint32_t norm, float beta)
{
    if (norm == LIME_NORM_PER_READ) return LIME_ERR_ARG;      // (the .res files are written with one norm)
    File ob(path_bin, "wb"), op(path_pos, "wb");
    if (!ob.f || !op.f) return LIME_ERR_IO;
    std::vector<PairSim> recs;
    std::vector<uint64_t> pos;
    recs.reserve(1 << 15); pos.reserve(1 << 15);
    uint64_t total = 1;
    PairSim sentinel = {0.0f, 0u};
    if (fwrite(&sentinel, sizeof sentinel, 1, ob.f) != 1) return LIME_ERR_IO;
    for (uint32_t r = 0; r < n_reads; ++r) {
        const uint8_t *row = sim + (size_t)r * n_refs;
        const uint8_t m = row_max ? row_max[r] : row_maximum(row, n_refs);
        const float top = static_cast<float>(m) / norm;
        if (top > beta) {
            const size_t hdr = recs.size();
            recs.push_back(PairSim{top, 0u});
            uint32_t cnt = 0;
            for (uint32_t j = 0; j < n_refs; ++j)
                if (row[j]) { recs.push_back(PairSim{static_cast<float>(row[j]) / norm, j}); ++cnt; }
            recs[hdr].id = cnt;
            pos.push_back(total);
            total += 1u + cnt;
        } else {
            pos.push_back(0);
        }
        if (recs.size() >= (1u << 15)) {
            if (fwrite(recs.data(), sizeof(PairSim), recs.size(), ob.f) != recs.size()) return LIME_ERR_IO;
            recs.clear();
        }
        if (pos.size() >= (1u << 15)) {
            if (fwrite(pos.data(), 8, pos.size(), op.f) != pos.size()) return LIME_ERR_IO;
            pos.clear();
        }
    }
    if (!recs.empty() && fwrite(recs.data(), sizeof(PairSim), recs.size(), ob.f) != recs.size()) return LIME_ERR_IO;
    if (!pos.empty() && fwrite(pos.data(), 8, pos.size(), op.f) != pos.size()) return LIME_ERR_IO;
    int e1 = ob.close(), e2 = op.close();
    return (e1 || e2) ? LIME_ERR_IO : LIME_OK;
}

// ---- the same two outputs from the compact form (row_max, row_off, pairs) -----------------
extern "C" int lime_write_res_txt_pairs(const char *path, const uint8_t *row_max, const uint64_t *row_off,
                                        const lime_pair_t *pairs, uint32_t n_reads, uint32_t norm, float beta)
{
    if (norm == LIME_NORM_PER_READ) return LIME_ERR_ARG;      // (the .res files are written with one norm)
    File o(path, "w");
    if (!o.f) return LIME_ERR_IO;
    std::vector<char> buf(1 << 16);
    setvbuf(o.f, buf.data(), _IOFBF, buf.size());
    for (uint32_t r = 0; r < n_reads; ++r) {
        const float top = static_cast<float>(row_max[r]) / norm;
        if (top > beta) {
            fprintf(o.f, "%.5f", top);
            for (uint64_t k = row_off[r]; k < row_off[r + 1]; ++k)
                fprintf(o.f, "\t%u\t%.5f", pairs[k].id_ref, static_cast<float>(static_cast<uint8_t>(pairs[k].sim)) / norm);
        }
        fputc('\n', o.f);
    }
    return o.close() ? LIME_ERR_IO : LIME_OK;
}

extern "C" int lime_write_res_bin_pairs(const char *path_bin, const char *path_pos, const uint8_t *row_max,
                                        const uint64_t *row_off, const lime_pair_t *pairs, uint32_t n_reads,
                                        uint32_t norm, float beta)
{
    if (norm == LIME_NORM_PER_READ) return LIME_ERR_ARG;      // (the .res files are written with one norm)
    File ob(path_bin, "wb"), op(path_pos, "wb");
    if (!ob.f || !op.f) return LIME_ERR_IO;
    std::vector<PairSim> recs;
    std::vector<uint64_t> pos;
    recs.reserve(1 << 15); pos.reserve(1 << 15);
    uint64_t total = 1;
    PairSim sentinel = {0.0f, 0u};
    if (fwrite(&sentinel, sizeof sentinel, 1, ob.f) != 1) return LIME_ERR_IO;
    for (uint32_t r = 0; r < n_reads; ++r) {
        const float top = static_cast<float>(row_max[r]) / norm;
        if (top > beta) {
            const uint32_t cnt = (uint32_t)(row_off[r + 1] - row_off[r]);
            recs.push_back(PairSim{top, cnt});
            for (uint64_t k = row_off[r]; k < row_off[r + 1]; ++k)
                recs.push_back(PairSim{static_cast<float>(static_cast<uint8_t>(pairs[k].sim)) / norm, pairs[k].id_ref});
            pos.push_back(total);
            total += 1u + cnt;
        } else {
            pos.push_back(0);
        }
        if (recs.size() >= (1u << 15)) {
            if (fwrite(recs.data(), sizeof(PairSim), recs.size(), ob.f) != recs.size()) return LIME_ERR_IO;
            recs.clear();
        }
        if (pos.size() >= (1u << 15)) {
            if (fwrite(pos.data(), 8, pos.size(), op.f) != pos.size()) return LIME_ERR_IO;
            pos.clear();
        }
    }
    if (!recs.empty() && fwrite(recs.data(), sizeof(PairSim), recs.size(), ob.f) != recs.size()) return LIME_ERR_IO;
    if (!pos.empty() && fwrite(pos.data(), 8, pos.size(), op.f) != pos.size()) return LIME_ERR_IO;
    int e1 = ob.close(), e2 = op.close();
    return (e1 || e2) ? LIME_ERR_IO : LIME_OK;
}

// ---- FASTA in: the documents of lime_build_index ---------------------------------------------
// '>' lines are headers and start a record; every other line's bytes, CR and LF dropped, are the record's symbols as they are (no case
// folding; lines in front of the first header belong to no record and are skipped).  rc: every record reversed and complemented
// (the script's `seqtk seq -r`): A<->T, C<->G, U->A, R<->Y, K<->M, B<->V, D<->H in both cases; S, W, N and every other byte stay.
static void complement_table(uint8_t comp[256])
{
    for (int b = 0; b < 256; ++b) comp[b] = (uint8_t)b;
    const char *from = "ATCGURYKMBVDH", *to = "TAGCAYRMKVBHD";
    for (int k = 0; from[k]; ++k) { comp[(uint8_t)from[k]] = (uint8_t)to[k]; comp[(uint8_t)(from[k] | 0x20)] = (uint8_t)(to[k] | 0x20); }
}

extern "C" int lime_fasta_read(const char *path, int rc, uint8_t **text, uint64_t **doc_off, uint32_t *n_docs)
{
    if (!path || !text || !doc_off || !n_docs) return LIME_ERR_ARG;
    *text = nullptr; *doc_off = nullptr; *n_docs = 0;
    File in(path, "rb");
    if (!in.f) return LIME_ERR_IO;
    uint8_t comp[256];
    complement_table(comp);
    std::vector<uint8_t> sym;
    std::vector<uint64_t> off;
    std::vector<char> buf(1 << 20);
    bool line_start = true, in_header = false;
    auto close_record = [&]() {
        if (rc && !off.empty()) {
            uint8_t *a = sym.data() + off.back(), *b = sym.data() + sym.size();
            for (uint8_t *x = a, *y = b; x < y; ) { --y; const uint8_t u = comp[*x], v = comp[*y]; *x++ = v; *y = u; }
        }
    };
    size_t got;
    while ((got = fread(buf.data(), 1, buf.size(), in.f)) > 0) {
        for (size_t i = 0; i < got; ++i) {
            const uint8_t ch = (uint8_t)buf[i];
            if (ch == '\n') { line_start = true; in_header = false; continue; }
            if (line_start) {
                line_start = false;
                if (ch == '>') {
                    close_record();
                    if (off.size() >= 0xFFFFFFFFull) return LIME_ERR_ARG;
                    off.push_back(sym.size()); in_header = true; continue;
                }
            }
            if (in_header || ch == '\r' || off.empty()) continue;
            sym.push_back(ch);
        }
    }
    if (ferror(in.f)) return LIME_ERR_IO;
    close_record();
    off.push_back(sym.size());
    const uint32_t nd = (uint32_t)(off.size() - 1);                        // (no record: doc_off = {0})
    uint8_t *t = static_cast<uint8_t *>(malloc(sym.size() ? sym.size() : 1));
    uint64_t *o = static_cast<uint64_t *>(malloc(off.size() * 8));
    if (!t || !o) { free(t); free(o); return LIME_ERR_NOMEM; }
    if (!sym.empty()) memcpy(t, sym.data(), sym.size());
    memcpy(o, off.data(), off.size() * 8);
    *text = t; *doc_off = o; *n_docs = nd;
    return LIME_OK;
}

// ---- FASTQ in ----------------------------------------------------------------------------------
// Four-line records, read line by line: '@' header, the sequence, '+' separator, the quality string.  The sequence line's bytes, CR
// dropped, are the record's symbols as they are; the quality string only has to be as long as the sequence.  A line ends at its LF
// or at the end of the file; what follows the last LF is a line only if it has a byte.  The first offending line is refused
// (include/lime_hip.h lists the four reasons and their texts).  rc as in lime_fasta_read.
// qual != NULL (lime_fastq_read_qual): the quality lines' bytes, CR dropped, too
static int fastq_read_impl(const char *who, const char *path, int rc, uint8_t **text, uint8_t **qual, uint64_t **doc_off, uint32_t *n_docs)
{
    *text = nullptr; *doc_off = nullptr; *n_docs = 0;
    if (qual) *qual = nullptr;
    std::vector<uint8_t> qsym;
    File in(path, "rb");
    if (!in.f) return lime_host::fail(LIME_ERR_IO, "%s: cannot open %s", who, path);
    uint8_t comp[256];
    complement_table(comp);
    std::vector<uint8_t> sym, line;
    std::vector<uint64_t> off;
    std::vector<char> buf(1 << 20);
    uint64_t n_lines = 0;                                  // complete lines so far
    size_t seq_len = 0;
    // one line without its LF; -> 0, or the code that was reported
    auto take_line = [&]() -> int {
        const uint64_t no = ++n_lines;                     // this line's number, from 1
        size_t len = 0;                                    // its bytes that are not CR
        for (uint8_t ch : line) len += ch != '\r';
        switch ((no - 1) & 3u) {
        case 0:
            if (line.empty() || line[0] != '@') return lime_host::fail(LIME_ERR_ARG, "%s: line %llu: record does not start with '@'", who, (unsigned long long)no);
            if (off.size() >= 0xFFFFFFFFull) return lime_host::fail(LIME_ERR_ARG, "%s: more than 2^32 - 1 records", who);
            off.push_back(sym.size());
            break;
        case 1:
            for (uint8_t ch : line) if (ch != '\r') sym.push_back(ch);
            seq_len = len;
            if (rc) {
                uint8_t *a = sym.data() + off.back(), *b = sym.data() + sym.size();
                for (uint8_t *x = a, *y = b; x < y; ) { --y; const uint8_t u = comp[*x], v = comp[*y]; *x++ = v; *y = u; }
            }
            break;
        case 2:
            if (line.empty() || line[0] != '+') return lime_host::fail(LIME_ERR_ARG, "%s: line %llu: separator line does not start with '+'", who, (unsigned long long)no);
            break;
        default:
            if (len != seq_len) return lime_host::fail(LIME_ERR_ARG, "%s: line %llu: quality length differs from sequence length", who, (unsigned long long)no);
            if (qual) for (uint8_t ch : line) if (ch != '\r') qsym.push_back(ch);
            break;
        }
        line.clear();
        return 0;
    };
    size_t got;
    bool open_line = false;                                // bytes since the last LF?
    while ((got = fread(buf.data(), 1, buf.size(), in.f)) > 0) {
        for (size_t i = 0; i < got; ++i) {
            const uint8_t ch = (uint8_t)buf[i];
            if (ch != '\n') { line.push_back(ch); open_line = true; continue; }
            const int e = take_line(); if (e) return e;
            open_line = false;
        }
    }
    if (ferror(in.f)) return lime_host::fail(LIME_ERR_IO, "%s: cannot read %s", who, path);
    if (open_line) { const int e = take_line(); if (e) return e; }
    if (n_lines & 3u) return lime_host::fail(LIME_ERR_ARG, "%s: line %llu: truncated record", who, (unsigned long long)n_lines);
    off.push_back(sym.size());
    const uint32_t nd = (uint32_t)(off.size() - 1);
    uint8_t *t = static_cast<uint8_t *>(malloc(sym.size() ? sym.size() : 1));
    uint64_t *o = static_cast<uint64_t *>(malloc(off.size() * 8));
    uint8_t *q = qual ? static_cast<uint8_t *>(malloc(qsym.size() ? qsym.size() : 1)) : nullptr;
    if (!t || !o || (qual && !q)) { free(t); free(o); free(q); return lime_host::fail(LIME_ERR_NOMEM, "%s: out of host memory", who); }
    if (!sym.empty()) memcpy(t, sym.data(), sym.size());
    if (q && !qsym.empty()) memcpy(q, qsym.data(), qsym.size());
    memcpy(o, off.data(), off.size() * 8);
    *text = t; *doc_off = o; *n_docs = nd;
    if (qual) *qual = q;
    return LIME_OK;
}

extern "C" int lime_fastq_read(const char *path, int rc, uint8_t **text, uint64_t **doc_off, uint32_t *n_docs)
{
    const char *who = "lime_fastq_read";
    if (!path || !text || !doc_off || !n_docs) return lime_host::fail(LIME_ERR_ARG, "%s: NULL argument", who);
    return fastq_read_impl(who, path, rc, text, nullptr, doc_off, n_docs);
}

extern "C" int lime_fastq_read_qual(const char *path, uint8_t **text, uint8_t **qual, uint64_t **doc_off, uint32_t *n_docs)
{
    const char *who = "lime_fastq_read_qual";
    if (!path || !text || !qual || !doc_off || !n_docs) return lime_host::fail(LIME_ERR_ARG, "%s: NULL argument", who);
    return fastq_read_impl(who, path, 0, text, qual, doc_off, n_docs);
}

// ---- the quality trim: the loop form of the rule (include/lime_hip.h), the oracle of lime_docs_trim_dev ------------------------
extern "C" int lime_quality_trim(const uint8_t *text, const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t q5, uint32_t q3,
                                 uint8_t **out_text, uint64_t **out_doc_off, lime_trim_info_t *info)
{
    const char *who = "lime_quality_trim";
    if (out_text) *out_text = nullptr;
    if (out_doc_off) *out_doc_off = nullptr;
    if (info) memset(info, 0, sizeof *info);
    if (!doc_off || !out_text || !out_doc_off) return lime_host::fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (q5 > 93 || q3 > 93) return lime_host::fail(LIME_ERR_ARG, "%s: cutoffs %u,%u; a Phred+33 quality is 0 .. 93", who, q5, q3);
    if (doc_off[0] != 0) return lime_host::fail(LIME_ERR_ARG, "%s: doc_off does not start at 0", who);
    for (uint32_t r = 0; r < n_docs; ++r)
        if (doc_off[r + 1] < doc_off[r]) return lime_host::fail(LIME_ERR_ARG, "%s: doc_off decreases at read %u", who, r);
    if (doc_off[n_docs] && (!text || !qual)) return lime_host::fail(LIME_ERR_ARG, "%s: NULL array", who);
    std::vector<uint8_t> sym;
    std::vector<uint64_t> off;
    off.reserve((size_t)n_docs + 1);
    lime_trim_info_t ti = {n_docs, 0, 0, doc_off[n_docs], 0};
    for (uint32_t r = 0; r < n_docs; ++r) {
        const uint64_t a = doc_off[r], L = doc_off[r + 1] - a;
        const uint8_t *b = qual + a;
        uint64_t lo = 0, hi = L;
        if (q3) {
            int64_t s = 0, lowest = 0;
            for (uint64_t i = L; i-- > 0; ) {
                s += (int64_t)b[i] - 33 - (int64_t)q3;
                if (s > 0) break;
                if (s < lowest) { lowest = s; hi = i; }
            }
        }
        if (q5) {
            int64_t s = 0, highest = 0;
            for (uint64_t i = 0; i < L; ++i) {
                s += (int64_t)q5 - ((int64_t)b[i] - 33);
                if (s < 0) break;
                if (s > highest) { highest = s; lo = i + 1; }
            }
        }
        off.push_back(sym.size());
        const uint64_t len = lo < hi ? hi - lo : 0;
        if (len) sym.insert(sym.end(), text + a + lo, text + a + hi);
        ti.n_changed += len != L;
        ti.n_empty += L != 0 && len == 0;
    }
    off.push_back(sym.size());
    ti.symbols_out = sym.size();
    uint8_t *t = static_cast<uint8_t *>(malloc(sym.size() ? sym.size() : 1));
    uint64_t *o = static_cast<uint64_t *>(malloc(off.size() * 8));
    if (!t || !o) { free(t); free(o); return lime_host::fail(LIME_ERR_NOMEM, "%s: out of host memory", who); }
    if (!sym.empty()) memcpy(t, sym.data(), sym.size());
    memcpy(o, off.data(), off.size() * 8);
    *out_text = t; *out_doc_off = o;
    if (info) *info = ti;
    return LIME_OK;
}

// ---- the adapter trim: the loop form of the rule (include/lime_hip.h), the oracle of lime_docs_trim_adapter_dev -----------------
extern "C" int lime_adapter_trim(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const uint8_t *adapter, uint32_t m, uint32_t min_overlap,
                                 uint32_t max_err_pct, uint8_t **out_text, uint64_t **out_doc_off, lime_trim_info_t *info)
{
    const char *who = "lime_adapter_trim";
    if (out_text) *out_text = nullptr;
    if (out_doc_off) *out_doc_off = nullptr;
    if (info) memset(info, 0, sizeof *info);
    if (!doc_off || !adapter || !out_text || !out_doc_off) return lime_host::fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (!m || m > 64) return lime_host::fail(LIME_ERR_ARG, "%s: an adapter of %u symbols; it holds 1 .. 64", who, m);
    uint8_t ad[64];
    for (uint32_t j = 0; j < m; ++j) {
        ad[j] = adapter[j] & 0xDF;
        if (ad[j] != 'A' && ad[j] != 'C' && ad[j] != 'G' && ad[j] != 'T')
            return lime_host::fail(LIME_ERR_ARG, "%s: adapter symbol %u is byte %u; an adapter holds A, C, G and T only", who, j, (unsigned)adapter[j]);
    }
    if (!min_overlap || min_overlap > m)
        return lime_host::fail(LIME_ERR_ARG, "%s: a minimum overlap of %u with an adapter of %u symbols; it is 1 .. %u", who, min_overlap, m, m);
    if (max_err_pct > 50) return lime_host::fail(LIME_ERR_ARG, "%s: an error rate of %u percent; it is 0 .. 50", who, max_err_pct);
    if (doc_off[0] != 0) return lime_host::fail(LIME_ERR_ARG, "%s: doc_off does not start at 0", who);
    for (uint32_t r = 0; r < n_docs; ++r)
        if (doc_off[r + 1] < doc_off[r]) return lime_host::fail(LIME_ERR_ARG, "%s: doc_off decreases at read %u", who, r);
    if (doc_off[n_docs] && !text) return lime_host::fail(LIME_ERR_ARG, "%s: NULL array", who);
    std::vector<uint8_t> sym;
    std::vector<uint64_t> off;
    off.reserve((size_t)n_docs + 1);
    lime_trim_info_t ti = {n_docs, 0, 0, doc_off[n_docs], 0};
    for (uint32_t r = 0; r < n_docs; ++r) {
        const uint64_t a = doc_off[r], L = doc_off[r + 1] - a;
        const uint8_t *s = text + a;
        uint64_t keep = L;
        for (uint64_t p = 0; p < L; ++p) {
            const uint32_t k = L - p < m ? (uint32_t)(L - p) : m;
            if (k < min_overlap) break;                  // (k only falls from here on)
            uint32_t mm = 0;
            for (uint32_t j = 0; j < k; ++j) mm += (s[p + j] & 0xDF) != ad[j];
            if (mm <= (k * max_err_pct) / 100) { keep = p; break; }
        }
        off.push_back(sym.size());
        if (keep) sym.insert(sym.end(), s, s + keep);
        ti.n_changed += keep != L;
        ti.n_empty += L != 0 && keep == 0;
    }
    off.push_back(sym.size());
    ti.symbols_out = sym.size();
    uint8_t *t = static_cast<uint8_t *>(malloc(sym.size() ? sym.size() : 1));
    uint64_t *o = static_cast<uint64_t *>(malloc(off.size() * 8));
    if (!t || !o) { free(t); free(o); return lime_host::fail(LIME_ERR_NOMEM, "%s: out of host memory", who); }
    if (!sym.empty()) memcpy(t, sym.data(), sym.size());
    memcpy(o, off.data(), off.size() * 8);
    *out_text = t; *out_doc_off = o;
    if (info) *info = ti;
    return LIME_OK;
}

// ---- the read filter: the loop form of the rule (include/lime_hip.h), the oracle of lime_docs_filter_dev -------------------------
// the refusals of the parameters, shared with lime_docs_filter_dev and lime_seq_reader_set_filter
int lime_host::filter_check(const char *who, const lime_filter_t *f)
{
    if (!f) return fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (f->polyx_mask > 15) return fail(LIME_ERR_ARG, "%s: a poly-X mask of %u; bits 0 .. 3 are A, C, G and T", who, f->polyx_mask);
    if (f->polyx_mask && (!f->polyx_min || f->polyx_min > 255))
        return fail(LIME_ERR_ARG, "%s: a shortest poly-X tail of %u symbols; it is 1 .. 255", who, f->polyx_min);
    if (f->min_complexity > 100) return fail(LIME_ERR_ARG, "%s: a complexity of %u percent; it is 0 .. 100", who, f->min_complexity);
    if (!f->polyx_mask && !f->max_len && !f->min_len && f->max_n == LIME_FILTER_OFF && !f->min_complexity)
        return fail(LIME_ERR_ARG, "%s: nothing asked: no poly-X base, no length cap, no shortest length, no N limit and no complexity", who);
    return LIME_OK;
}

namespace {
inline uint32_t class_of(uint8_t b)                       // 0 .. 3: A C G T; 4: other
{
    switch (b & 0xDF) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return 4; }
}
}

extern "C" int lime_read_filter(const uint8_t *text, const uint64_t *doc_off, uint32_t n_docs, const lime_filter_t *f, uint8_t **out_text,
                                uint64_t **out_doc_off, lime_filter_info_t *info)
{
    const char *who = "lime_read_filter";
    if (out_text) *out_text = nullptr;
    if (out_doc_off) *out_doc_off = nullptr;
    if (info) memset(info, 0, sizeof *info);
    if (!doc_off || !f || !out_text || !out_doc_off) return lime_host::fail(LIME_ERR_ARG, "%s: NULL argument", who);
    int rc = lime_host::filter_check(who, f); if (rc) return rc;
    if (doc_off[0] != 0) return lime_host::fail(LIME_ERR_ARG, "%s: doc_off does not start at 0", who);
    for (uint32_t r = 0; r < n_docs; ++r)
        if (doc_off[r + 1] < doc_off[r]) return lime_host::fail(LIME_ERR_ARG, "%s: doc_off decreases at read %u", who, r);
    if (doc_off[n_docs] && !text) return lime_host::fail(LIME_ERR_ARG, "%s: NULL array", who);
    std::vector<uint8_t> sym;
    std::vector<uint64_t> off;
    off.reserve((size_t)n_docs + 1);
    lime_filter_info_t fi = {n_docs, 0, 0, 0, 0, 0, doc_off[n_docs], 0};
    for (uint32_t r = 0; r < n_docs; ++r) {
        const uint64_t a = doc_off[r], L = doc_off[r + 1] - a;
        const uint8_t *s = text + a;
        off.push_back(sym.size());
        if (!L) continue;                                // (counted nowhere)
        uint64_t best = 0;                               // t*
        for (uint32_t X = 0; X < 4; ++X) {
            if (!(f->polyx_mask >> X & 1u)) continue;
            uint64_t mm = 0;
            for (uint64_t t = 1; t <= L; ++t) {
                const bool is_x = class_of(s[L - t]) == X;
                mm += !is_x;
                if (is_x && t >= f->polyx_min && 8 * mm <= t && t > best) best = t;
            }
        }
        uint64_t n = L - best;
        fi.n_polyx += best != 0;
        if (f->max_len && n > f->max_len) { n = f->max_len; ++fi.n_capped; }
        if (n < f->min_len) { ++fi.n_short; continue; }
        uint64_t n_other = 0, d = 0;
        for (uint64_t j = 0; j < n; ++j) n_other += class_of(s[j]) == 4;
        for (uint64_t j = 0; j + 1 < n; ++j) d += class_of(s[j]) != class_of(s[j + 1]);
        if (f->max_n != LIME_FILTER_OFF && n_other > f->max_n) { ++fi.n_many_n; continue; }
        if (n >= 2 && 100 * d < (uint64_t)f->min_complexity * (n - 1)) { ++fi.n_low_complexity; continue; }
        sym.insert(sym.end(), s, s + n);
    }
    off.push_back(sym.size());
    fi.symbols_out = sym.size();
    uint8_t *t = static_cast<uint8_t *>(malloc(sym.size() ? sym.size() : 1));
    uint64_t *o = static_cast<uint64_t *>(malloc(off.size() * 8));
    if (!t || !o) { free(t); free(o); return lime_host::fail(LIME_ERR_NOMEM, "%s: out of host memory", who); }
    if (!sym.empty()) memcpy(t, sym.data(), sym.size());
    memcpy(o, off.data(), off.size() * 8);
    *out_text = t; *out_doc_off = o;
    if (info) *info = fi;
    return LIME_OK;
}

// ---- the overlap cut: the loop form of the rule (include/lime_hip.h), the oracle of lime_docs_trim_overlap_dev -------------------
int lime_host::overlap_check(const char *who, uint32_t min_overlap, uint32_t max_err_pct)
{
    if (!min_overlap) return fail(LIME_ERR_ARG, "%s: a minimum overlap of 0; it is 1 or more", who);
    if (max_err_pct > 50) return fail(LIME_ERR_ARG, "%s: an error rate of %u percent; it is 0 .. 50", who, max_err_pct);
    return LIME_OK;
}

namespace {
// I* of the mates a[0 .. La), b[0 .. Lb): the largest admissible I in [O, La + Lb - O], 0 without one
uint64_t overlap_insert(const uint8_t *a, uint64_t La, const uint8_t *b, uint64_t Lb, uint64_t O, uint64_t E)
{
    if (La + Lb < 2 * O) return 0;
    for (uint64_t I = La + Lb - O; I >= O; --I) {
        const uint64_t j0 = I > Lb ? I - Lb : 0, j1 = La < I ? La : I;
        if (j1 < j0 + O) continue;                       // n(I) < O (an empty or a short mate)
        const uint64_t n = j1 - j0;
        uint64_t same = 0;
        for (uint64_t j = j0; j < j1; ++j) {
            const uint32_t ca = class_of(a[j]), cb = class_of(b[I - 1 - j]);
            same += ca < 4 && cb == 3 - ca;              // (A C G T are 0 1 2 3: the complement is 3 - class)
        }
        if (n - same <= (n * E) / 100) return I;
    }
    return 0;
}

template <class T> T *to_malloc(const std::vector<T> &v)         // the vector's copy in a block of at least one byte, NULL without memory
{
    T *p = static_cast<T *>(malloc(v.empty() ? 1 : v.size() * sizeof(T)));
    if (p && !v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
}

extern "C" int lime_pair_overlap_trim(const uint8_t *text1, const uint64_t *doc_off1, const uint8_t *text2, const uint64_t *doc_off2, uint32_t n_docs,
                                      uint32_t min_overlap, uint32_t max_err_pct, uint8_t **out_text1, uint64_t **out_doc_off1, uint8_t **out_text2,
                                      uint64_t **out_doc_off2, uint32_t **insert, lime_overlap_info_t *info)
{
    const char *who = "lime_pair_overlap_trim";
    if (out_text1) *out_text1 = nullptr;
    if (out_doc_off1) *out_doc_off1 = nullptr;
    if (out_text2) *out_text2 = nullptr;
    if (out_doc_off2) *out_doc_off2 = nullptr;
    if (insert) *insert = nullptr;
    if (info) memset(info, 0, sizeof *info);
    if (!doc_off1 || !doc_off2 || !out_text1 || !out_doc_off1 || !out_text2 || !out_doc_off2) return lime_host::fail(LIME_ERR_ARG, "%s: NULL argument", who);
    int rc = lime_host::overlap_check(who, min_overlap, max_err_pct); if (rc) return rc;
    const uint8_t *text[2] = {text1, text2};
    const uint64_t *doc_off[2] = {doc_off1, doc_off2};
    for (int m = 0; m < 2; ++m) {
        if (doc_off[m][0] != 0) return lime_host::fail(LIME_ERR_ARG, "%s: doc_off of mate %d does not start at 0", who, m + 1);
        for (uint32_t r = 0; r < n_docs; ++r)
            if (doc_off[m][r + 1] < doc_off[m][r]) return lime_host::fail(LIME_ERR_ARG, "%s: doc_off of mate %d decreases at read %u", who, m + 1, r);
        if (doc_off[m][n_docs] && !text[m]) return lime_host::fail(LIME_ERR_ARG, "%s: NULL array", who);
    }
    std::vector<uint8_t> sym[2];
    std::vector<uint64_t> off[2];
    std::vector<uint32_t> ins;
    off[0].reserve((size_t)n_docs + 1); off[1].reserve((size_t)n_docs + 1); ins.reserve(n_docs);
    lime_overlap_info_t oi = {n_docs, 0, 0, doc_off1[n_docs] + doc_off2[n_docs], 0};
    for (uint32_t r = 0; r < n_docs; ++r) {
        const uint64_t La = doc_off1[r + 1] - doc_off1[r], Lb = doc_off2[r + 1] - doc_off2[r];
        const uint8_t *a = text1 + doc_off1[r], *b = text2 + doc_off2[r];
        const uint64_t I = overlap_insert(a, La, b, Lb, min_overlap, max_err_pct);
        const uint64_t ka = I && I < La ? I : La, kb = I && I < Lb ? I : Lb;
        off[0].push_back(sym[0].size()); off[1].push_back(sym[1].size());
        if (ka) sym[0].insert(sym[0].end(), a, a + ka);
        if (kb) sym[1].insert(sym[1].end(), b, b + kb);
        ins.push_back((uint32_t)I);
        oi.n_overlap += I != 0;
        oi.n_cut += ka != La || kb != Lb;
    }
    off[0].push_back(sym[0].size()); off[1].push_back(sym[1].size());
    oi.symbols_out = sym[0].size() + sym[1].size();
    uint8_t *t1 = to_malloc(sym[0]), *t2 = to_malloc(sym[1]);
    uint64_t *o1 = to_malloc(off[0]), *o2 = to_malloc(off[1]);
    uint32_t *in = insert ? to_malloc(ins) : nullptr;
    if (!t1 || !t2 || !o1 || !o2 || (insert && !in)) {
        free(t1); free(t2); free(o1); free(o2); free(in);
        return lime_host::fail(LIME_ERR_NOMEM, "%s: out of host memory", who);
    }
    *out_text1 = t1; *out_doc_off1 = o1; *out_text2 = t2; *out_doc_off2 = o2;
    if (insert) *insert = in;
    if (info) *info = oi;
    return LIME_OK;
}

// the format of a sequence file by its first byte: '@' is FASTQ (1), anything else FASTA (0) -- an empty file and text in front of the
// first FASTA header included
extern "C" int lime_seq_format(const char *path, int *format)
{
    if (!path || !format) return lime_host::fail(LIME_ERR_ARG, "lime_seq_format: NULL argument");
    File in(path, "rb");
    if (!in.f) return lime_host::fail(LIME_ERR_IO, "lime_seq_format: cannot open %s", path);
    const int ch = fgetc(in.f);
    if (ch == EOF && ferror(in.f)) return lime_host::fail(LIME_ERR_IO, "lime_seq_format: cannot read %s", path);
    *format = ch == '@';
    return LIME_OK;
}

// ---- per-position read statistics: the loop form of the rule (include/lime_hip.h), the oracle of lime_docs_qc_dev ----------------
extern "C" int lime_read_qc(const uint8_t *text, const uint8_t *qual, const uint64_t *doc_off, uint32_t n_docs, uint32_t n_pos, uint64_t *tables)
{
    const char *who = "lime_read_qc";
    if (!doc_off || !tables) return lime_host::fail(LIME_ERR_ARG, "%s: NULL array", who);
    if (!n_pos || n_pos > LIME_QC_MAX_POS) return lime_host::fail(LIME_ERR_ARG, "%s: %u positions; there are 1 .. %u", who, n_pos, LIME_QC_MAX_POS);
    if (doc_off[0] != 0) return lime_host::fail(LIME_ERR_ARG, "%s: doc_off does not start at 0", who);
    for (uint32_t r = 0; r < n_docs; ++r)
        if (doc_off[r + 1] < doc_off[r]) return lime_host::fail(LIME_ERR_ARG, "%s: doc_off decreases at read %u", who, r);
    if (doc_off[n_docs] && !text) return lime_host::fail(LIME_ERR_ARG, "%s: NULL array", who);
    uint64_t *len_hist = tables + 8u * ((size_t)n_pos + 1u), *gc_hist = len_hist + n_pos + 1u, *mq_hist = gc_hist + 101;
    for (uint32_t r = 0; r < n_docs; ++r) {
        const uint64_t a = doc_off[r], L = doc_off[r + 1] - a;
        uint64_t gc = 0, acgt = 0, qs = 0;
        for (uint64_t p = 0; p < L; ++p) {
            uint64_t *row = tables + 8u * (p < n_pos ? p : n_pos);
            const uint32_t c = class_of(text[a + p]);
            ++row[c];
            acgt += c < 4u;
            gc += c == 1u || c == 2u;
            if (qual) {
                const uint32_t q = qual[a + p];
                row[5] += q; row[6] += q >= 53u; row[7] += q >= 63u;
                qs += q;
            }
        }
        ++len_hist[L < n_pos ? L : n_pos];
        if (acgt) ++gc_hist[100u * gc / acgt];
        if (qual && L) ++mq_hist[qs / L];
    }
    return LIME_OK;
}

// ---- the report of the statistics as JSON (include/lime_hip.h: lime_qc_report_write) ----
namespace {
void qc_json_string(std::string &o, const char *s)
{
    o += '"';
    for (; *s; ++s) {
        const unsigned char ch = (unsigned char)*s;
        if (ch == '"' || ch == '\\') { o += '\\'; o += (char)ch; }
        else if (ch < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", ch); o += b; }
        else o += (char)ch;
    }
    o += '"';
}
void qc_json_u64(std::string &o, uint64_t v)
{
    char b[24];
    snprintf(b, sizeof b, "%llu", (unsigned long long)v);
    o += b;
}
// "key": [t[0], t[stride], ... n numbers]
void qc_json_array(std::string &o, const char *key, const uint64_t *t, size_t n, size_t stride)
{
    o += '"'; o += key; o += "\": [";
    for (size_t k = 0; k < n; ++k) { if (k) o += ", "; qc_json_u64(o, t[k * stride]); }
    o += ']';
}
void qc_json_section(std::string &o, const uint64_t *t, uint32_t n_pos, bool with_qual)
{
    const size_t rows = (size_t)n_pos + 1u;
    const uint64_t *len_hist = t + 8u * rows, *gc_hist = len_hist + rows, *mq_hist = gc_hist + 101;
    uint64_t reads = 0, symbols = 0, gc = 0, q20 = 0, q30 = 0;
    for (size_t p = 0; p < rows; ++p) {
        reads += len_hist[p];
        for (int c = 0; c < 5; ++c) symbols += t[8u * p + c];
        gc += t[8u * p + 1] + t[8u * p + 2];
        q20 += t[8u * p + 6]; q30 += t[8u * p + 7];
    }
    o += "{\"reads\": "; qc_json_u64(o, reads);
    o += ", \"empty\": "; qc_json_u64(o, len_hist[0]);
    o += ", \"symbols\": "; qc_json_u64(o, symbols);
    o += ", \"gc\": "; qc_json_u64(o, gc);
    o += ",\n    \"bases\": {";
    static const char *const names[5] = {"A", "C", "G", "T", "other"};
    for (int c = 0; c < 5; ++c) { if (c) o += ",\n      "; qc_json_array(o, names[c], t + c, rows, 8); }
    o += "},\n    "; qc_json_array(o, "length_hist", len_hist, rows, 1);
    o += ",\n    "; qc_json_array(o, "gc_hist", gc_hist, 101, 1);
    if (with_qual) {
        o += ",\n    \"q20\": "; qc_json_u64(o, q20);
        o += ", \"q30\": "; qc_json_u64(o, q30);
        o += ",\n    "; qc_json_array(o, "qual_sum", t + 5, rows, 8);
        o += ",\n    "; qc_json_array(o, "qual_ge20", t + 6, rows, 8);
        o += ",\n    "; qc_json_array(o, "qual_ge30", t + 7, rows, 8);
        o += ",\n    "; qc_json_array(o, "mean_qual_hist", mq_hist, 256, 1);
    }
    o += '}';
}
}

extern "C" int lime_qc_report_write(const char *path, uint32_t n_files, const char *const *names, const int *formats, uint32_t n_pos,
                                    const uint64_t *const *before, const uint64_t *const *after)
{
    const char *who = "lime_qc_report_write";
    if (!path || !names || !formats || !before || !after) return lime_host::fail(LIME_ERR_ARG, "%s: NULL argument", who);
    if (!n_files) return lime_host::fail(LIME_ERR_ARG, "%s: no file to report on", who);
    if (!n_pos || n_pos > LIME_QC_MAX_POS) return lime_host::fail(LIME_ERR_ARG, "%s: %u positions; there are 1 .. %u", who, n_pos, LIME_QC_MAX_POS);
    for (uint32_t k = 0; k < n_files; ++k) {
        if (!names[k] || !before[k] || !after[k]) return lime_host::fail(LIME_ERR_ARG, "%s: NULL argument (file %u)", who, k);
        if (formats[k] != 0 && formats[k] != 1) return lime_host::fail(LIME_ERR_ARG, "%s: format %d of file %u; 0 is FASTA, 1 FASTQ", who, formats[k], k);
    }
    std::string o = "{\"lime_qc_report\": 1, \"positions\": ";
    qc_json_u64(o, n_pos);
    o += ", \"files\": [";
    for (uint32_t k = 0; k < n_files; ++k) {
        o += k ? ",\n  {\"file\": " : "\n  {\"file\": ";
        qc_json_string(o, names[k]);
        o += formats[k] ? ", \"format\": \"fastq\"" : ", \"format\": \"fasta\"";
        o += ",\n   \"before\": "; qc_json_section(o, before[k], n_pos, formats[k] == 1);
        o += ",\n   \"after\": "; qc_json_section(o, after[k], n_pos, false);
        o += '}';
    }
    o += "]}\n";
    const std::string tmp = std::string(path) + ".tmp" + std::to_string((long)getpid());
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return lime_host::fail(LIME_ERR_IO, "%s: cannot write %s", who, path);
    const bool wrote = fwrite(o.data(), 1, o.size(), f) == o.size();
    const bool closed = fclose(f) == 0;
    if (!wrote || !closed || rename(tmp.c_str(), path) != 0) {
        remove(tmp.c_str());
        return lime_host::fail(LIME_ERR_IO, "%s: cannot write %s", who, path);
    }
    return LIME_OK;
}
