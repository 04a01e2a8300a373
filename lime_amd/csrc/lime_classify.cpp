// lime_classify.cpp -- the read-assignment step that consumes the hot path's .res files
// (reference: src/Classify.cpp).  Host code: the work is a few float compares per
// read over lists the GPU already compacted.  Written from the reference's behaviour, not its text:
// every read's lists are first loaded into one in-memory form (from .res.bin/.res.pos or .res.txt),
// then one routine decides.  Decision rules and their reference lines:
//   U  no file holds a record for the read                                   (Classify.cpp:503-509)
//   1  files whose maximum is within ERROR of the best; their genomes within ERROR of the file's
//      maximum form the candidate set; one taxon at the chosen rank -> C     (:511-547)
//   2  else compare the candidates' per-strand sums (files 0+3 and 1+2 for paired-end): if one
//      strand wins by more than ERROR and its best candidates share one taxon -> C (:549-640)
//   3  else the same sums over ALL genomes; genomes within ERROR of the best: one taxon -> C,
//      otherwise (HIGHER) the lowest higher rank they share -> H, or A        (:642-690, :168-302)
// float arithmetic, the 0.02 tolerance and the text/binary difference (text values are the %.5f
// roundings) are kept as they are.  read_taxonomy, value_tables, decide and write_verdict (lime_classify.h) are shared with
// the device path (lime_choose.cpp: lime_classify_lists_dev), lime_classify_mem runs decide over lists held in memory.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <fstream>
#include <iostream>
#include <new>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "lime_hip.h"
#include "lime_classify.h"

namespace lime_cls {

// ';'-separated lineage file, first line a header (Classify.cpp:32-85).  As in the reference a last
// line without a newline is not taken, and an empty field at the chosen rank is skipped.
bool read_taxonomy(const std::string &path, int rank, bool higher, uint32_t n_targ, Taxonomy &tx, std::string &err)
{
    std::ifstream f(path.c_str());
    if (!f.is_open()) { err = "Error opening file " + path + "."; return false; }
    std::string col[7];
    auto next_line = [&]() {
        for (int s = 0; s < 6; ++s) std::getline(f, col[s], ';');
        std::getline(f, col[6], '\n');
    };
    next_line();
    tx.rank_name = col[rank];
    if (higher) tx.higher.assign(N_RANKS, std::vector<uint32_t>(n_targ, 0u));
    uint32_t line = 0;
    next_line();
    while (f.good()) {
        if (rank > 0) {
            if (!col[rank].empty()) tx.at_rank.push_back((uint32_t)atoi(col[rank].c_str()));
        } else {
            tx.at_rank.push_back(line);
        }
        if (higher && line < n_targ)
            for (int i = (rank > 0 ? rank - 1 : 0); i < N_RANKS; ++i)
                if (!col[i + 1].empty()) tx.higher[i][line] = (uint32_t)atoi(col[i + 1].c_str());
        ++line;
        next_line();
    }
    return true;
}

void value_tables(uint32_t norm, float beta, int binary, float vals[256], float tops[256])
{
    for (uint32_t k = 0; k < 256u; ++k) {
        const float v = static_cast<float>(static_cast<uint8_t>(k)) / norm;       // the writers' expression (lime_host.cpp)
        float seen = v;
        if (!binary) {                                                           // fprintf("%.5f") -> TxtSource's `>> float`
            char buf[64];
            snprintf(buf, sizeof buf, "%.5f", v);
            std::istringstream is(buf);
            if (!(is >> seen)) seen = 0.0f;
        }
        vals[k] = seen;
        tops[k] = v > beta ? seen : 0.0f;
    }
}

} // namespace lime_cls

namespace {
using namespace lime_cls;

// ---- sources of the per-read lists ---------------------------------------------------------
struct BinSource {                               // .res.bin + .res.pos (ClusterBWT_DA.cpp:376-436)
    FILE *bin = nullptr, *pos = nullptr;
    ~BinSource() { if (bin) fclose(bin); if (pos) fclose(pos); }
    bool open(const std::string &base) { bin = fopen((base + ".bin").c_str(), "rb"); pos = fopen((base + ".pos").c_str(), "rb"); return bin && pos; }
    bool read(uint64_t r, ReadLists &out)
    {
        out.clear();
        uint64_t p = 0;
        if (fseeko(pos, (off_t)(r * 8u), SEEK_SET) != 0 || fread(&p, 8, 1, pos) != 1) return false;
        if (!p) return true;
        struct { float sim; uint32_t id; } rec;
        if (fseeko(bin, (off_t)(p * 8u), SEEK_SET) != 0 || fread(&rec, 8, 1, bin) != 1) return false;
        out.top = rec.sim;
        const uint32_t n = rec.id;
        out.cells.resize(n);
        for (uint32_t k = 0; k < n; ++k) {
            if (fread(&rec, 8, 1, bin) != 1) return false;
            out.cells[k].sim = rec.sim; out.cells[k].ref = rec.id;
        }
        return true;
    }
};

struct TxtSource {                               // .res.txt, one line per read (ClusterBWT_DA.cpp:414-441)
    std::ifstream f;
    bool open(const std::string &base) { f.open((base + ".txt").c_str()); return f.is_open(); }
    bool read(uint64_t, ReadLists &out)
    {
        out.clear();
        std::string line;
        std::getline(f, line);
        std::istringstream is(line);
        if (!(is >> out.top)) { out.top = 0.0f; return true; }
        for (;;) {
            Cell c;
            if (!(is >> c.ref)) break;
            if (!(is >> c.sim)) c.sim = 0.0f;
            out.cells.push_back(c);
        }
        return true;
    }
};

} // namespace

namespace lime_cls {

// value of genome g in a read's list (first match), 0 if absent
static float value_of(const ReadLists &l, uint32_t g)
{
    for (const Cell &c : l.cells) if (c.ref == g) return c.sim;
    return 0.0f;
}

static lime_verdict_t verdict(char type, uint32_t taxon, float sim, uint8_t rule)
{
    lime_verdict_t v;
    memset(&v, 0, sizeof v);
    v.taxon = taxon; v.sim = sim; v.type = (uint8_t)type; v.rule = rule;
    return v;
}

lime_verdict_t decide(const ReadLists *L, uint32_t n_files, uint32_t n_targ, const Taxonomy &tx, int rank, bool higher,
               std::vector<float> (&all)[2])
{
    // which files hold the read, and the best file maximum
    float best = 0.0f;
    bool any = false;
    for (uint32_t i = 0; i < n_files; ++i)
        if (L[i].top) { if (!any || L[i].top > best) best = L[i].top; any = true; }
    if (!any) return verdict('U', 0u, 0.0f, 0);

    // rule 1: candidates = genomes close to the maximum of every file that is close to the best
    std::vector<uint32_t> cand;
    for (uint32_t i = 0; i < n_files; ++i) {
        if (!L[i].top || !(best - L[i].top < TOL)) continue;
        for (const Cell &c : L[i].cells) {
            if (!(L[i].top - c.sim < TOL)) continue;
            bool seen = false;
            for (uint32_t g : cand) if (g == c.ref) { seen = true; break; }
            if (!seen) cand.push_back(c.ref);
        }
    }
    std::set<uint32_t> taxa;
    for (uint32_t g : cand) taxa.insert(tx.at_rank[g]);
    if (taxa.size() == 1) return verdict('C', *taxa.begin(), best, 1);

    // rule 2: per-strand sums of the candidates
    {
        float top2[2] = {0.0f, 0.0f};
        std::vector<float> s0(cand.size()), s1(cand.size());
        for (size_t e = 0; e < cand.size(); ++e) {
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (uint32_t i = 0; i < n_files; ++i) v[i] = value_of(L[i], cand[e]);
            s0[e] = n_files == 4 ? v[0] + v[3] : v[0];
            s1[e] = n_files == 4 ? v[1] + v[2] : v[1];
            if (top2[0] < s0[e]) top2[0] = s0[e];
            if (top2[1] < s1[e]) top2[1] = s1[e];
        }
        const std::vector<float> *win = nullptr;
        float wtop = 0.0f;
        if (top2[0] > top2[1] + TOL) { win = &s0; wtop = top2[0]; }
        else if (top2[1] > top2[0] + TOL) { win = &s1; wtop = top2[1]; }
        if (win) {
            taxa.clear();
            for (size_t e = 0; e < cand.size(); ++e) if ((*win)[e] == wtop) taxa.insert(tx.at_rank[cand[e]]);
            if (taxa.size() == 1) return verdict('C', *taxa.begin(), wtop, 2);
        }
    }

    // rule 3: the same sums over all genomes
    for (int k = 0; k < 2; ++k) all[k].assign(n_targ, 0.0f);
    {
        std::vector<float> f2, f3;
        if (n_files == 4) { f2.assign(n_targ, 0.0f); f3.assign(n_targ, 0.0f); }
        for (uint32_t i = 0; i < n_files; ++i)
            for (const Cell &c : L[i].cells) {
                if (c.ref >= n_targ) continue;
                if (i == 0) all[0][c.ref] += c.sim;
                else if (i == 1) all[1][c.ref] += c.sim;
                else if (i == 2) f2[c.ref] += c.sim;
                else f3[c.ref] += c.sim;
            }
        if (n_files == 4) for (uint32_t j = 0; j < n_targ; ++j) { all[0][j] += f3[j]; all[1][j] += f2[j]; }
    }
    float hi[2] = {0.0f, 0.0f};
    for (int k = 0; k < 2; ++k) for (uint32_t j = 0; j < n_targ; ++j) if (hi[k] < all[k][j]) hi[k] = all[k][j];
    std::vector<uint32_t> gens;                  // ascending genome index (the reference's std::set order)
    float h;
    if (hi[0] > hi[1]) { h = hi[0]; for (uint32_t j = 0; j < n_targ; ++j) if (h - all[0][j] < TOL) gens.push_back(j); }
    else if (hi[0] < hi[1]) { h = hi[1]; for (uint32_t j = 0; j < n_targ; ++j) if (h - all[1][j] < TOL) gens.push_back(j); }
    else { h = hi[0]; for (uint32_t j = 0; j < n_targ; ++j) if ((h - all[0][j] < TOL) || (h - all[1][j] < TOL)) gens.push_back(j); }
    if (gens.empty()) return verdict('A', 0u, 0.0f, 3);
    bool one = true;
    for (uint32_t g : gens) if (tx.at_rank[g] != tx.at_rank[gens[0]]) one = false;
    if (one) return verdict('C', tx.at_rank[gens[0]], h, 3);
    if (higher && rank >= 1) {
        for (int idx = rank - 1; idx < N_RANKS; ++idx) {
            const uint32_t t = tx.higher[idx][gens[0]];
            bool same = true;
            for (uint32_t g : gens) if (tx.higher[idx][g] != t) { same = false; break; }
            if (same && t != 0u) return verdict('H', t, h, 3);
        }
    }
    return verdict('A', 0u, 0.0f, 3);
}

void write_verdict(std::ostream &out, uint64_t r, const lime_verdict_t &v, uint64_t counts[4])
{
    switch (v.type) {
    case 'U': out << "U," << r << ",NA,0\n"; ++counts[1]; break;
    case 'A': out << "A," << r << ",NA,0\n"; ++counts[2]; break;
    case 'C': out << "C," << r << "," << v.taxon << "," << v.sim << "\n"; ++counts[0]; break;
    default:  out << "H," << r << "," << v.taxon << "," << v.sim << "\n"; ++counts[3]; break;
    }
}

} // namespace lime_cls

namespace {
using namespace lime_cls;

template <typename Source>
int run(uint32_t n_files, const char *const *inputs, uint32_t n_reads, uint32_t n_targ, const Taxonomy &tx, int rank,
        bool higher, std::ofstream &out, uint64_t counts[4], std::string &err)
{
    std::vector<Source> src(n_files);
    for (uint32_t i = 0; i < n_files; ++i)
        if (!src[i].open(inputs[i])) { err = std::string("Error opening ") + inputs[i]; return LIME_ERR_IO; }
    ReadLists L[4];
    std::vector<float> all[2];
    for (uint32_t r = 0; r < n_reads; ++r) {
        for (uint32_t i = 0; i < n_files; ++i)
            if (!src[i].read(r, L[i])) { err = std::string("Error reading ") + inputs[i]; return LIME_ERR_IO; }
        for (uint32_t i = 0; i < n_files; ++i)
            for (const Cell &c : L[i].cells)
                if (c.ref >= n_targ) { err = std::string("genome index beyond numGenomes in ") + inputs[i]; return LIME_ERR_ARG; }
        write_verdict(out, r, decide(L, n_files, n_targ, tx, rank, higher, all), counts);
    }
    return LIME_OK;
}

thread_local std::string g_cls_err;

} // namespace

extern "C" const char *lime_classify_error(void) { return g_cls_err.c_str(); }

extern "C" int lime_classify(uint32_t n_files, const char *const *inputs, int binary, uint32_t n_reads, uint32_t n_targ,
                             const char *path_out, const char *path_tax, int rank, int higher, uint64_t counts[4])
{
    uint64_t local[4] = {0, 0, 0, 0};
    if (!counts) counts = local;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if ((n_files != 2 && n_files != 4) || !inputs || !path_out || !path_tax || rank < 0 || rank > N_RANKS) {
        g_cls_err = "lime_classify: bad argument";
        return LIME_ERR_ARG;
    }
    Taxonomy tx;
    if (!read_taxonomy(path_tax, rank, higher != 0, n_targ, tx, g_cls_err)) return LIME_ERR_IO;
    if (tx.at_rank.size() != n_targ) {
        std::ostringstream m;
        m << "Number of taxIDs = " << tx.at_rank.size() << " lower than genome number: poor taxonomy information to classify.";
        g_cls_err = m.str();
        return LIME_ERR_ARG;
    }
    std::ofstream out(path_out);
    if (!out.is_open()) { g_cls_err = "ERROR: File Output not Open"; return LIME_ERR_IO; }
    out << "C/U/A/H,IdSeqRead,TaxID,maxSim\n";
    int rc = binary ? run<BinSource>(n_files, inputs, n_reads, n_targ, tx, rank, higher != 0, out, counts, g_cls_err)
                    : run<TxtSource>(n_files, inputs, n_reads, n_targ, tx, rank, higher != 0, out, counts, g_cls_err);
    out.close();
    return rc;
}

// ---- the same decision over lists held in memory, and the pieces the device path shares ------------------------------
extern "C" int lime_taxonomy_load(const char *path, int rank, int higher, uint32_t n_targ, lime_taxonomy **out)
{
    if (!out || !path || rank < 0 || rank > N_RANKS || (higher && rank == 0)) {
        g_cls_err = "lime_taxonomy_load: bad argument (rank 0..6; HIGHER needs a rank of 1 or more)";
        return LIME_ERR_ARG;
    }
    *out = nullptr;
    lime_taxonomy *t = new (std::nothrow) lime_taxonomy();
    if (!t) { g_cls_err = "lime_taxonomy_load: out of host memory"; return LIME_ERR_NOMEM; }
    if (!read_taxonomy(path, rank, higher != 0, n_targ, t->host, g_cls_err)) { delete t; return LIME_ERR_IO; }
    if (t->host.at_rank.size() != n_targ) {
        std::ostringstream m;
        m << "Number of taxIDs = " << t->host.at_rank.size() << " lower than genome number: poor taxonomy information to classify.";
        g_cls_err = m.str();
        delete t;
        return LIME_ERR_ARG;
    }
    t->rank = rank; t->higher = higher != 0; t->n_targ = n_targ;
    *out = t;
    return LIME_OK;
}

extern "C" void lime_taxonomy_free(lime_taxonomy *tx)
{
    if (!tx) return;
    if (tx->release) tx->release(tx);            // (the device copy, if a device classification made one)
    delete tx;
}

extern "C" int lime_write_classification(const char *path, const lime_verdict_t *verdicts, uint32_t n_reads)
{
    if (!path || (n_reads && !verdicts)) { g_cls_err = "lime_write_classification: NULL argument"; return LIME_ERR_ARG; }
    std::ofstream out(path);
    if (!out.is_open()) { g_cls_err = "ERROR: File Output not Open"; return LIME_ERR_IO; }
    out << "C/U/A/H,IdSeqRead,TaxID,maxSim\n";
    uint64_t counts[4] = {0, 0, 0, 0};
    for (uint32_t r = 0; r < n_reads; ++r) write_verdict(out, r, verdicts[r], counts);
    out.close();
    if (out.fail()) { g_cls_err = std::string("Error writing ") + path; return LIME_ERR_IO; }
    return LIME_OK;
}

// ---- the classification file in parts ----
struct lime_classification_writer {
    std::ofstream out;
    std::string path, tmp;
};

extern "C" int lime_classification_writer_open(const char *path, lime_classification_writer **out)
{
    if (!path || !out) { g_cls_err = "lime_classification_writer_open: NULL argument"; return LIME_ERR_ARG; }
    *out = nullptr;
    lime_classification_writer *w = new (std::nothrow) lime_classification_writer();
    if (!w) { g_cls_err = "lime_classification_writer_open: out of host memory"; return LIME_ERR_NOMEM; }
    w->path = path;
    w->tmp = w->path + ".tmp" + std::to_string((long)getpid());
    w->out.open(w->tmp);
    if (!w->out.is_open()) { g_cls_err = "ERROR: File Output not Open"; delete w; return LIME_ERR_IO; }
    w->out << "C/U/A/H,IdSeqRead,TaxID,maxSim\n";
    *out = w;
    return LIME_OK;
}

extern "C" int lime_classification_writer_append(lime_classification_writer *w, uint64_t first_read, const lime_verdict_t *verdicts, uint32_t n)
{
    if (!w || (n && !verdicts)) { g_cls_err = "lime_classification_writer_append: NULL argument"; return LIME_ERR_ARG; }
    uint64_t counts[4] = {0, 0, 0, 0};
    for (uint32_t r = 0; r < n; ++r) write_verdict(w->out, first_read + r, verdicts[r], counts);
    if (w->out.fail()) { g_cls_err = std::string("Error writing ") + w->tmp; return LIME_ERR_IO; }
    return LIME_OK;
}

extern "C" int lime_classification_writer_close(lime_classification_writer *w, int commit)
{
    if (!w) return LIME_OK;
    w->out.close();
    int rc = LIME_OK;
    if (commit && (w->out.fail() || rename(w->tmp.c_str(), w->path.c_str()) != 0)) {
        g_cls_err = std::string("Error writing ") + w->path;
        rc = LIME_ERR_IO;
    }
    if (!commit || rc) (void)remove(w->tmp.c_str());
    delete w;
    return rc;
}

// lime_classify_mem (read_norms == NULL) and lime_classify_mem_norms: list i takes the values of read r from the tables of read_norms[i][r]
// where read_norms[i] is there, else from those of norms[i]; both go through decide()
static int classify_mem_impl(const char *who, uint32_t n_files, const uint8_t *const *row_max, const uint64_t *const *row_off,
                             const lime_pair_t *const *pairs, const uint32_t *norms, const uint8_t *const *read_norms, const float *betas, int binary,
                             uint32_t n_reads, uint32_t n_targ, const lime_taxonomy *tx, lime_verdict_t *verdicts, uint64_t counts[4])
{
    uint64_t local[4] = {0, 0, 0, 0};
    if (!counts) counts = local;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if ((n_files != 2 && n_files != 4) || !row_max || !row_off || !pairs || !norms || !betas || !tx || (n_reads && !verdicts)) {
        g_cls_err = std::string(who) + ": bad argument";
        return LIME_ERR_ARG;
    }
    if (tx->n_targ != n_targ) { g_cls_err = std::string(who) + ": the taxonomy was loaded for another number of genomes"; return LIME_ERR_ARG; }
    float vals[4][256], tops[4][256];
    // per list with a norm per read: the tables of the norms met so far, [norm][2][256]; norm 0 (no read has it) gives no record
    std::vector<float> per[4];
    std::vector<uint8_t> have[4];
    for (uint32_t i = 0; i < n_files; ++i) {
        const bool pr = read_norms && read_norms[i];
        if (n_reads && (!row_max[i] || !row_off[i])) { g_cls_err = std::string(who) + ": bad list"; return LIME_ERR_ARG; }
        if (pr) { per[i].assign((size_t)256 * 512, 0.0f); have[i].assign(256, 0); have[i][0] = 1; continue; }
        if (!norms[i]) { g_cls_err = std::string(who) + ": bad list"; return LIME_ERR_ARG; }
        if (norms[i] == LIME_NORM_PER_READ) { g_cls_err = std::string(who) + ": LIME_NORM_PER_READ is no norm of a list (lime_classify_mem_norms takes the reads' norms)"; return LIME_ERR_ARG; }
        value_tables(norms[i], betas[i], binary, vals[i], tops[i]);
    }
    ReadLists L[4];
    std::vector<float> all[2];
    for (uint32_t r = 0; r < n_reads; ++r) {
        for (uint32_t i = 0; i < n_files; ++i) {
            const float *v = vals[i], *t = tops[i];
            if (read_norms && read_norms[i]) {
                const uint32_t n = read_norms[i][r];
                float *tab = &per[i][(size_t)n * 512];
                if (!have[i][n]) { value_tables(n, betas[i], binary, tab, tab + 256); have[i][n] = 1; }
                v = tab; t = tab + 256;
            }
            L[i].clear();
            L[i].top = t[row_max[i][r]];
            for (uint64_t k = row_off[i][r]; k < row_off[i][r + 1]; ++k) {
                const lime_pair_t p = pairs[i][k];
                if (p.id_ref >= n_targ) { g_cls_err = "genome index beyond numGenomes in list " + std::to_string(i); return LIME_ERR_ARG; }
                L[i].cells.push_back(Cell{v[(uint8_t)p.sim], p.id_ref});
            }
        }
        verdicts[r] = decide(L, n_files, n_targ, tx->host, tx->rank, tx->higher != 0, all);
        switch (verdicts[r].type) { case 'C': ++counts[0]; break; case 'U': ++counts[1]; break; case 'A': ++counts[2]; break; default: ++counts[3]; }
    }
    return LIME_OK;
}

extern "C" int lime_classify_mem(uint32_t n_files, const uint8_t *const *row_max, const uint64_t *const *row_off,
                                 const lime_pair_t *const *pairs, const uint32_t *norms, const float *betas, int binary,
                                 uint32_t n_reads, uint32_t n_targ, const lime_taxonomy *tx, lime_verdict_t *verdicts,
                                 uint64_t counts[4])
{
    return classify_mem_impl("lime_classify_mem", n_files, row_max, row_off, pairs, norms, nullptr, betas, binary, n_reads, n_targ, tx, verdicts, counts);
}

extern "C" int lime_classify_mem_norms(uint32_t n_files, const uint8_t *const *row_max, const uint64_t *const *row_off,
                                       const lime_pair_t *const *pairs, const uint32_t *norms, const uint8_t *const *read_norms,
                                       const float *betas, int binary, uint32_t n_reads, uint32_t n_targ, const lime_taxonomy *tx,
                                       lime_verdict_t *verdicts, uint64_t counts[4])
{
    if (!read_norms) { g_cls_err = "lime_classify_mem_norms: bad argument"; return LIME_ERR_ARG; }
    return classify_mem_impl("lime_classify_mem_norms", n_files, row_max, row_off, pairs, norms, read_norms, betas, binary, n_reads, n_targ, tx, verdicts,
                             counts);
}
