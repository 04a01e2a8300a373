// LiME_fasta -- Preprocessing.sh + LiME_paired.sh for one sample, from FASTA or FASTQ files, as ONE process with nothing on disk in between:
//   LiME_fasta reads_1.fasta [reads_2.fasta] (--refs refs.fasta | --gidx file.gidx) --lineage LineageFile --readlen L --out output
//              [--alpha 16] [--beta 0.25] [--rank 1] [--trlcp k] [--batch-reads N [--window-bytes W]] [--trim-qual (Q | Q5,Q3)]
//              [--trim-adapter SEQ[,SEQ2] [--adapter-overlap O] [--adapter-error E]]
//              [--trim-polyx BASES[,T]] [--max-len K] [--min-len M] [--max-n K] [--min-complexity C] [--trim-overlap O[,E]]
//              [--qc-report FILE [--qc-positions P]]
// Each reads file is FASTA or four-line FASTQ, decided by its first byte ('@': FASTQ; lime_docs_from_file), the mates each on their own;
// --refs is FASTA.  The files' bytes go to the device as they are and are parsed there; per collection (reads_1, its reverse
// complements, reads_2, its reverse complements: the script's `seqtk seq -r`) the reads are merged into the genome index, scanned and
// chosen from in HBM, the lists are classified there (lime_classify_sample_dev) and only the verdicts (12 bytes per read) come back to
// be written as `output`.  --refs parses the genomes with the same device parser and builds their index in the process; --gidx loads
// one that BuildIndex --refs wrote.  --trlcp k: lcp values truncated at k (eGap's option; with --gidx at most the index's).
// --batch-reads N: a sample of any size.  The reads files are read N records at a time (lime_seq_reader, through a raw device window of
// W bytes, default 64 MiB), each batch is classified on its own against the same genome index (lime_classify_sample_stream) and its
// lines are appended to `output`, which is written under a temporary name and renamed at the end: a failure half-way leaves no output
// file.  The verdicts are those of the whole sample; the cluster count and the maximum length printed per collection are PER-BATCH
// figures (the count summed over the batches, the largest of the batches' maxima): a cluster with reads of three batches counts three times.
// --gidx a.gidx --gidx b.gidx ...: a genome database cut into index shards (BuildIndex --refs --shard-positions), in genome order: the
// lineage file's order is the concatenation.  All files are probed (lime_gindex_probe) before a device is opened: shards built with
// different --trlcp or terminators, and a lineage file of another genome count, are refused with a text.  All shards are loaded; per
// collection every shard is merged and scanned on its own and the shards' lists are made into the whole row's on the device
// (lime_classify_sample_shards_dev / lime_classify_sample_stream_shards).  The verdicts are those of one index; the clusters and the
// maximum length printed per collection are PER-SHARD figures in the same way (summed / the largest over the shards).
// --readlen auto: no one read length; every read is normalised by its own (norm = its length + 1 - alpha, LIME_NORM_PER_READ of
// lime_classify_sample_dev): files whose reads differ in length after trimming.  A read of more than 255 symbols ends the run with a text.
// --trim-qual Q: every read is cut at its 3' end by the BWA / cutadapt quality rule with cutoff Q (include/lime_hip.h: lime_quality_trim;
// Phred+33) on the device, before anything else is made of it; --trim-qual Q5,Q3: at both ends.  Every reads file must then be FASTQ, and
// --readlen must be auto: a fixed norm on trimmed reads is the mistake --readlen auto removes.  Each mate is trimmed on its own, the reverse
// complements are made from the trimmed reads, an emptied read stays in its place as an empty read (verdict U), and the 255-symbol limit
// holds for the trimmed length.  Per reads file one line is printed: the reads changed and emptied, the symbols before and after (with
// --batch-reads: summed over the batches).  Nothing else is written.
// --trim-adapter SEQ: every read is cut where the 3' adapter SEQ (1 .. 64 of ACGT) begins in it, by the rule at lime_adapter_trim in
// include/lime_hip.h (mismatches only, the leftmost match; a match is at least --adapter-overlap O symbols long, default 3, with at most
// E percent of them wrong, --adapter-error E, 0 .. 50, default 10), on the device.  SEQ,SEQ2: SEQ2 for reads_2 (the R1 and R2 adapters of a
// kit differ); one SEQ serves every mate.  FASTA and FASTQ reads files are taken; --readlen must be auto, for --trim-qual's reason.  With
// --trim-qual every read is cut by quality first and at its adapter second.  The rest is as for --trim-qual: each mate on its own, the
// reverse complements from the trimmed reads, an emptied read stays in its place, one line of counts per reads file.
// --trim-polyx BASES[,T], --max-len K, --min-len M, --max-n K, --min-complexity C: the read filter, by the rule at lime_read_filter in
// include/lime_hip.h, on the device, behind both trims.  --trim-polyx G (or GA,12): the longest tail of at least T symbols (default 10) of one
// of BASES, with at most one other symbol per eight, is cut: the poly-G tails of two-colour instruments.  --max-len K: what remains is cut
// to K symbols; --max-len 255 is how a file with longer reads runs under --readlen auto.  Then a read of fewer than M symbols, with more than
// K symbols that are no base (N), or with fewer than C percent of its neighbouring symbols different (fastp's complexity) is emptied and
// stays in its place as an empty read (verdict U).  --trim-polyx and --max-len change lengths and need --readlen auto, for --trim-qual's
// reason; the other three only empty reads and are taken with a fixed --readlen L too.  Each mate on its own, the reverse complements from
// the filtered reads, one line of counts per reads file.
// --trim-overlap O[,E]: adapter read-through cut from the two mates' overlap, with no adapter sequence given, by the rule at
// lime_pair_overlap_trim in include/lime_hip.h, on the device: the largest insert length I at which the first I symbols of one mate are the
// reverse complement of the first I symbols of the other, over at least O places (default 30) with at most E percent of them wrong (0 .. 50,
// default 10); both mates keep their first I symbols.  It needs two reads files and --readlen auto (for --trim-qual's reason); FASTA or
// FASTQ.  It runs LAST, behind each mate's quality trim, adapter trim and filter: it is the only stage that needs both mates.  So --min-len
// judges a read before this cut (the floor behind it is O), and a 5' quality cut (--trim-qual Q5,Q3) moves a read's anchor: such a pair is
// judged on the strings as they are and usually has no overlap.  The reverse complements are made from the cut reads.  One line of counts
// for the pair: the pairs with an overlap, the pairs cut, the symbols before and after.
// --qc-report FILE: per-position statistics of the reads, by the rule at lime_read_qc in include/lime_hip.h, counted on the device
// (lime_docs_qc_dev; with --batch-reads lime_seq_reader_set_qc) and written to FILE as JSON (lime_qc_report_write): one entry per reads file, in
// the order given; `before` is the file as parsed (with the quality tables for FASTQ), `after` the mate's reads as they enter
// classification, behind every stage asked for, --trim-overlap included.  --qc-positions P: the positions with a row of their own, 1 .. 512
// (default 256); later ones are pooled.  The report is the same with and without --batch-reads, `output` is what it is without the flag, and
// one line names FILE.  Any reads files, any --gidx / --refs, any --readlen.
// The defaults are the script's constants (LiME_paired.sh:21-23); norm = readLen + 1 - alpha (ClusterBWT_DA.cpp:555).  The reference's
// compile-time switches are environment variables, as for the other drop-ins: LIME_EBWT (default 1), LIME_BIN (default 1), LIME_HIGHER (0).
#include <string.h>
#include <chrono>
#include <iostream>
#include <string>
#include <vector>

#include "cli_common.h"

// "Q" -> (0, Q), "Q5,Q3": digits only, each 0 .. 93
static bool parse_trim(const char *s, unsigned *q5, unsigned *q3)
{
    unsigned v[2] = {0, 0};
    int k = 0, digits = 0;
    for (; *s; ++s) {
        if (*s == ',') { if (!digits || k == 1) return false; k = 1; digits = 0; continue; }
        if (*s < '0' || *s > '9' || digits == 2) return false;
        v[k] = v[k] * 10 + (unsigned)(*s - '0'); ++digits;
    }
    if (!digits || v[0] > 93 || v[1] > 93) return false;
    if (k == 0) { *q5 = 0; *q3 = v[0]; } else { *q5 = v[0]; *q3 = v[1]; }
    return true;
}

static void print_trim(const char *file, unsigned q5, unsigned q3, const lime_trim_info_t &t)
{
    std::cout << file << ": quality trim " << q5 << "," << q3 << ": " << t.n_changed << " of " << t.n_reads << " reads changed, " << t.n_empty << " emptied, "
              << t.symbols_in << " symbols before, " << t.symbols_out << " after." << std::endl;
}

// "SEQ" or "SEQ,SEQ2": 1 .. 64 of ACGTacgt each
static bool parse_adapters(const char *s, std::string ad[2], int *n)
{
    const char *comma = strchr(s, ',');
    ad[0] = comma ? std::string(s, comma) : std::string(s);
    ad[1] = comma ? std::string(comma + 1) : std::string();
    *n = comma ? 2 : 1;
    for (int k = 0; k < *n; ++k) {
        if (ad[k].empty() || ad[k].size() > 64) return false;
        for (char ch : ad[k]) if (!memchr("ACGT", ch & 0xDF, 4)) return false;
    }
    return true;
}

static void print_adapter(const char *file, const std::string &ad, unsigned overlap, unsigned err, const lime_trim_info_t &t)
{
    std::cout << file << ": adapter trim " << ad << " (overlap " << overlap << ", error " << err << "%): " << t.n_changed << " of " << t.n_reads << " reads changed, "
              << t.n_empty << " emptied, " << t.symbols_in << " symbols before, " << t.symbols_out << " after." << std::endl;
}

// digits only, at most nine of them -> *v
static bool parse_u32(const char *s, unsigned *v)
{
    unsigned x = 0;
    int digits = 0;
    for (; *s; ++s) {
        if (*s < '0' || *s > '9' || digits == 9) return false;
        x = x * 10 + (unsigned)(*s - '0'); ++digits;
    }
    *v = x;
    return digits > 0;
}

// "BASES" or "BASES,T": BASES 1 or more of ACGTacgt, T 1 .. 255 (default 10)
static bool parse_polyx(const char *s, lime_filter_t *f)
{
    unsigned mask = 0, t = 10;
    const char *comma = strchr(s, ',');
    for (const char *p = s; *p && p != comma; ++p) {
        const char *at = static_cast<const char *>(memchr("ACGT", *p & 0xDF, 4));
        if (!at) return false;
        mask |= 1u << (at - "ACGT");
    }
    if (!mask || (comma && (!parse_u32(comma + 1, &t) || !t || t > 255))) return false;
    f->polyx_mask = mask; f->polyx_min = t;
    return true;
}

static void print_filter(const char *file, const lime_filter_t &f, const lime_filter_info_t &t)
{
    std::string bases;
    for (int b = 0; b < 4; ++b) if (f.polyx_mask >> b & 1u) bases += "ACGT"[b];
    std::cout << file << ": read filter (poly-X " << (bases.empty() ? "-" : bases) << "," << (f.polyx_mask ? f.polyx_min : 0) << ", max-len " << f.max_len << ", min-len " << f.min_len << ", max-n ";
    if (f.max_n == LIME_FILTER_OFF) std::cout << "-"; else std::cout << f.max_n;
    std::cout << ", min-complexity " << f.min_complexity << "%): " << t.n_polyx << " of " << t.n_reads << " reads with a poly-X tail, " << t.n_capped << " capped, " << t.n_short
              << " short, " << t.n_many_n << " with many N, " << t.n_low_complexity << " of low complexity, " << t.symbols_in << " symbols before, " << t.symbols_out
              << " after." << std::endl;
}

// "O" or "O,E": O >= 1, E 0 .. 50 (default 10)
static bool parse_overlap(const char *s, unsigned *o, unsigned *e)
{
    const char *comma = strchr(s, ',');
    const std::string first = comma ? std::string(s, comma) : std::string(s);
    if (!parse_u32(first.c_str(), o) || !*o) return false;
    if (comma && (!parse_u32(comma + 1, e) || *e > 50)) return false;
    return true;
}

static void print_overlap(const char *file1, const char *file2, unsigned overlap, unsigned err, const lime_overlap_info_t &t)
{
    std::cout << file1 << " + " << file2 << ": overlap trim (overlap " << overlap << ", error " << err << "%): " << t.n_overlap << " of " << t.n_pairs
              << " pairs with an overlap, " << t.n_cut << " cut, " << t.symbols_in << " symbols before, " << t.symbols_out << " after." << std::endl;
}

static int env_flag(const char *name, int dflt)
{
    const char *s = getenv(name);
    return s ? atoi(s) != 0 : dflt;
}

namespace {
struct BatchSink {                             // --batch-reads: the writer and the collections' counters over the batches
    lime_classification_writer *w = nullptr;
    uint32_t n_coll = 0;
    uint32_t n_shards = 1;
    uint64_t n_clusters[4] = {0, 0, 0, 0}, max_len[4] = {0, 0, 0, 0};
    bool write_failed = false;                 // the call ended with the writer's error: its text is in lime_classify_error
};
int batch_sink(void *user, uint64_t first_read, const lime_verdict_t *verdicts, uint32_t n, const lime_stats_t *stats)
{
    BatchSink *s = static_cast<BatchSink *>(user);
    for (uint32_t sh = 0; sh < s->n_shards; ++sh)
        for (uint32_t k = 0; k < s->n_coll; ++k) {
            const lime_stats_t &x = stats[(size_t)sh * s->n_coll + k];
            s->n_clusters[k] += x.n_clusters;
            if (x.max_len > s->max_len[k]) s->max_len[k] = x.max_len;
        }
    const int rc = lime_classification_writer_append(s->w, first_read, verdicts, n);
    s->write_failed = rc != LIME_OK;
    return rc;
}
}

int main(int argc, char **argv)
{
    CliClock clk;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<const char *> reads;
    std::vector<const char *> gidx;
    const char *refs = nullptr, *lineage = nullptr, *output = nullptr;
    unsigned alpha = 16, rank = 1, trlcp = 0, batch_reads = 0, q5 = 0, q3 = 0;
    bool trim = false;
    std::string adapters[2];                   // --trim-adapter: [0] for reads_1 (and reads_2 when one is given), [1] for reads_2
    int n_adapters = 0;
    unsigned ad_overlap = 3, ad_err = 10;
    bool have_ad_opt = false;
    lime_filter_t flt = {0, 0, 0, 0, LIME_FILTER_OFF, 0};      // --trim-polyx, --max-len, --min-len, --max-n, --min-complexity
    bool filter = false;
    unsigned ov_overlap = 30, ov_err = 10;     // --trim-overlap
    bool cut_overlap = false;
    const char *qc_report = nullptr;           // --qc-report, --qc-positions
    unsigned qc_pos = 256;
    bool have_qc_pos = false;
    unsigned long long window_bytes = 0;
    bool batched = false, have_window = false;
    float beta = 0.25f;
    unsigned char readLen = 0;                 // dataTypeSim, parsed with %hhu like ClusterBWT_DA (:519-521)
    bool bad = false, have_len = false, len_auto = false;      // --readlen auto: every read by its own length (LIME_NORM_PER_READ)
    for (int i = 1; i < argc; ++i) {
        const bool more = i + 1 < argc;
        if (!strcmp(argv[i], "--refs")) { if (more) refs = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--gidx")) { if (more) gidx.push_back(argv[++i]); else bad = true; }
        else if (!strcmp(argv[i], "--lineage")) { if (more) lineage = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--out")) { if (more) output = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--readlen")) {
            if (more && !strcmp(argv[i + 1], "auto")) { ++i; have_len = true; len_auto = true; }
            else if (more && sscanf(argv[i + 1], "%hhu", &readLen) == 1) { ++i; have_len = true; len_auto = false; }
            else bad = true;
        }
        else if (!strcmp(argv[i], "--alpha")) { if (more && sscanf(argv[i + 1], "%u", &alpha) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--beta")) { if (more && sscanf(argv[i + 1], "%f", &beta) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--rank")) { if (more && sscanf(argv[i + 1], "%u", &rank) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--trlcp")) { if (more && sscanf(argv[i + 1], "%u", &trlcp) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--batch-reads")) { if (more && sscanf(argv[i + 1], "%u", &batch_reads) == 1 && batch_reads) { ++i; batched = true; } else bad = true; }
        else if (!strcmp(argv[i], "--trim-qual")) { if (more && parse_trim(argv[i + 1], &q5, &q3)) { ++i; trim = true; } else bad = true; }
        else if (!strcmp(argv[i], "--trim-adapter")) { if (more && parse_adapters(argv[i + 1], adapters, &n_adapters)) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--adapter-overlap")) { if (more && sscanf(argv[i + 1], "%u", &ad_overlap) == 1 && ad_overlap) { ++i; have_ad_opt = true; } else bad = true; }
        else if (!strcmp(argv[i], "--adapter-error")) { if (more && sscanf(argv[i + 1], "%u", &ad_err) == 1 && ad_err <= 50) { ++i; have_ad_opt = true; } else bad = true; }
        else if (!strcmp(argv[i], "--trim-polyx")) { if (more && parse_polyx(argv[i + 1], &flt)) { ++i; filter = true; } else bad = true; }
        else if (!strcmp(argv[i], "--max-len")) { if (more && parse_u32(argv[i + 1], &flt.max_len) && flt.max_len) { ++i; filter = true; } else bad = true; }
        else if (!strcmp(argv[i], "--min-len")) { if (more && parse_u32(argv[i + 1], &flt.min_len) && flt.min_len) { ++i; filter = true; } else bad = true; }
        else if (!strcmp(argv[i], "--max-n")) { if (more && parse_u32(argv[i + 1], &flt.max_n)) { ++i; filter = true; } else bad = true; }
        else if (!strcmp(argv[i], "--min-complexity")) {
            if (more && parse_u32(argv[i + 1], &flt.min_complexity) && flt.min_complexity && flt.min_complexity <= 100) { ++i; filter = true; } else bad = true;
        }
        else if (!strcmp(argv[i], "--trim-overlap")) { if (more && parse_overlap(argv[i + 1], &ov_overlap, &ov_err)) { ++i; cut_overlap = true; } else bad = true; }
        else if (!strcmp(argv[i], "--qc-report")) { if (more) qc_report = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--qc-positions")) { if (more && parse_u32(argv[i + 1], &qc_pos) && qc_pos && qc_pos <= LIME_QC_MAX_POS) { ++i; have_qc_pos = true; } else bad = true; }
        else if (!strcmp(argv[i], "--window-bytes")) { if (more && sscanf(argv[i + 1], "%llu", &window_bytes) == 1 && window_bytes) { ++i; have_window = true; } else bad = true; }
        else reads.push_back(argv[i]);
    }
    if (have_window && !batched) bad = true;
    if (have_qc_pos && !qc_report) bad = true;
    if (trim && !len_auto) bad = true;             // (a fixed norm on trimmed reads)
    const bool cut_adapter = n_adapters > 0;
    if (cut_adapter && !len_auto) bad = true;      // (the same)
    if (have_ad_opt && !cut_adapter) bad = true;
    if ((flt.polyx_mask || flt.max_len) && !len_auto) bad = true;          // (the same; the three filters only empty reads)
    if (cut_overlap && (!len_auto || reads.size() != 2)) bad = true;       // (the same; and a pair is two files)
    if (n_adapters == 2 && reads.size() != 2) bad = true;
    for (int k = 0; k < n_adapters; ++k) if (ad_overlap > adapters[k].size()) bad = true;
    if (n_adapters == 1) adapters[1] = adapters[0];
    if (reads.empty() || reads.size() > 2 || !refs == gidx.empty() || !lineage || !output || !have_len) bad = true;
    if (bad) {
        std::cerr << "Error usage " << argv[0] << " reads_1.fasta [reads_2.fasta] (--refs refs.fasta | --gidx file.gidx [--gidx next.gidx ...]) --lineage LineageFile --readlen (L | auto) --out output\n"
                  << "           [--alpha 16] [--beta 0.25] [--rank 1] [--trlcp k] [--batch-reads N [--window-bytes W]] [--trim-qual (Q | Q5,Q3)]\n"
                  << "           [--trim-adapter SEQ[,SEQ2] [--adapter-overlap 3] [--adapter-error 10]]\n"
                  << "           [--trim-polyx BASES[,10]] [--max-len K] [--min-len M] [--max-n K] [--min-complexity C] [--trim-overlap O[,E]]\n"
                  << "           [--qc-report FILE [--qc-positions 256]]\n"
                  << "  classifies the reads of one sample (one file: single-end, two: paired-end) against the genomes of refs.fasta, or of an\n"
                  << "  index written by BuildIndex --refs, and writes only `output` (the classification file).  A reads file is FASTA or\n"
                  << "  four-line FASTQ, by its first byte ('@': FASTQ), each mate on its own; refs.fasta is FASTA.  --trlcp k: lcp values\n"
                  << "  truncated at k.  --batch-reads N: a sample of any size, read and classified N reads at a time (through a window of W\n"
                  << "  bytes per file); the verdicts are the whole sample's, the clusters and maximum length printed per collection are\n"
                  << "  per-batch figures (summed / the largest over the batches: a cluster with reads of three batches counts three times).\n"
                  << "  --gidx given several times: the index shards of one genome database (BuildIndex --refs --shard-positions), in genome\n"
                  << "  order (the lineage file's order); the verdicts are those of one index, the clusters and maximum length printed per\n"
                  << "  collection are per-shard figures in the same way (summed / the largest over the shards).\n"
                  << "  --readlen auto: every read is normalised by its own length (norm = its length + 1 - alpha), for reads of different\n"
                  << "  lengths (trimmed FASTQ); a read of more than 255 symbols is refused.\n"
                  << "  --trim-qual Q: every read is cut at its 3' end by the BWA / cutadapt quality rule, cutoff Q (0 .. 93, Phred+33), on the\n"
                  << "  device; Q5,Q3: at both ends.  The reads files must be FASTQ and --readlen must be auto; one line per reads file\n"
                  << "  gives the reads changed and emptied and the symbols before and after.\n"
                  << "  --trim-adapter SEQ: every read is cut where the 3' adapter SEQ (1 .. 64 of ACGT) begins in it: mismatches only, the\n"
                  << "  leftmost match of at least --adapter-overlap O symbols (1 .. the adapter's length) with at most --adapter-error E percent\n"
                  << "  of them wrong (0 .. 50), on the device; SEQ,SEQ2: SEQ2 for reads_2.  FASTA or FASTQ; --readlen must be auto; behind\n"
                  << "  --trim-qual where both are given; one line of counts per reads file.\n"
                  << "  --trim-polyx BASES[,T]: the longest tail of at least T symbols (1 .. 255, default 10) of one of BASES (of ACGT; G for the\n"
                  << "  poly-G tails of two-colour instruments) with at most one other symbol per eight is cut; --max-len K: what remains is cut to K\n"
                  << "  symbols (--max-len 255: how a file with longer reads runs).  Both need --readlen auto.  --min-len M, --max-n K,\n"
                  << "  --min-complexity C (1 .. 100): a read of fewer than M symbols, with more than K symbols that are no base, or with fewer than C\n"
                  << "  percent of its neighbouring symbols different is emptied (verdict U); also with --readlen L.  On the device, behind the\n"
                  << "  trims; FASTA or FASTQ; one line of counts per reads file.\n"
                  << "  --trim-overlap O[,E]: adapter read-through cut from the mates' overlap, no adapter given: the largest insert length I at which\n"
                  << "  the first I symbols of one mate are the reverse complement of the other's, over at least O places (30) with at most E percent\n"
                  << "  of them wrong (0 .. 50, default 10); both mates keep I symbols.  Two reads files and --readlen auto; FASTA or FASTQ.  It runs\n"
                  << "  last, behind each mate's trims and filter: --min-len judges a read before this cut (the floor behind it is O), and a 5'\n"
                  << "  quality cut moves a read's anchor, so such a pair usually has no overlap.  One line of counts for the pair.\n"
                  << "  --qc-report FILE: per-position statistics of every reads file as parsed (`before`) and as it enters classification, behind\n"
                  << "  the stages (`after`), counted on the device and written to FILE as JSON: bases, qualities (FASTQ, before), lengths, GC.\n"
                  << "  --qc-positions P: the positions with a row of their own, 1 .. 512 (default 256); later ones are pooled.\n"
                  << "  LIME_EBWT, LIME_BIN, LIME_HIGHER as for ClusterBWT_DA / Classify." << std::endl;
        exit(1);
    }
    const int EBWT = env_flag("LIME_EBWT", 1), BIN = env_flag("LIME_BIN", 1), HIGHER = env_flag("LIME_HIGHER", 0);
    const uint32_t norm = len_auto ? LIME_NORM_PER_READ : (uint32_t)(readLen + 1 - alpha);        // ClusterBWT_DA.cpp:555
    const uint32_t n_mates = (uint32_t)reads.size();
    const uint32_t n_shards = refs ? 1u : (uint32_t)gidx.size();
    if (n_shards > 1) {                        // the shards must agree and the lineage must hold their genomes: known before a device is opened
        uint64_t total = 0;
        uint32_t cap0 = 0; uint8_t term0 = 0;
        for (uint32_t s = 0; s < n_shards; ++s) {
            uint32_t nd = 0, cap = 0; uint8_t term = 0;
            if (lime_gindex_probe(gidx[s], &nd, nullptr, &cap, &term) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(1); }
            if (s == 0) { cap0 = cap; term0 = term; }
            else if (cap != cap0 || term != term0) {
                std::cerr << "Error: " << gidx[s] << " was built with --trlcp " << cap << " and terminator " << (unsigned)term << ", " << gidx[0] << " with --trlcp "
                          << cap0 << " and terminator " << (unsigned)term0 << ": the shards of one database are built alike." << std::endl;
                exit(1);
            }
            total += nd;
        }
        if (total > 0xFFFFFFFFull) { std::cerr << "Error: the index shards hold " << total << " genomes; ids are 32 bits." << std::endl; exit(1); }
        lime_taxonomy *probe = nullptr;
        if (lime_taxonomy_load(lineage, (int)rank, env_flag("LIME_HIGHER", 0), (uint32_t)total, &probe) != LIME_OK) {
            std::cerr << "Error: " << lineage << " does not describe the " << total << " genomes of the " << n_shards << " index shards: " << lime_classify_error() << std::endl;
            exit(1);
        }
        lime_taxonomy_free(probe);
    }

    int formats[2] = {0, 0};
    std::vector<uint64_t> qc_before[2], qc_after[2];     // --qc-report: the tables of each reads file
    for (uint32_t m = 0; m < n_mates && (trim || qc_report); ++m) {      // known before a device is opened, like the shards' headers
        int &format = formats[m];
        if (lime_seq_format(reads[m], &format) != LIME_OK) { std::cerr << "Error reading " << reads[m] << ": " << lime_last_error() << std::endl; return -LIME_ERR_IO; }
        if (qc_report) { qc_before[m].assign(LIME_QC_WORDS(qc_pos), 0); qc_after[m].assign(LIME_QC_WORDS(qc_pos), 0); }
        if (trim && format != 1) { std::cerr << "Error reading " << reads[m] << ": --trim-qual needs the qualities of a FASTQ file; this one is FASTA." << std::endl; return 1; }
    }

    lime_ctx *ctx = nullptr;
    if (lime_init(pick_device(), &ctx) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(EXIT_FAILURE); }
    clk.mark("lime_init (HIP runtime)");
    lime_docs *mates[2] = {nullptr, nullptr};
    lime_seq_reader *readers[2] = {nullptr, nullptr};
    uint64_t numReads = 0;
    for (uint32_t m = 0; m < n_mates && batched; ++m) {
        const int rc = lime_seq_reader_open(ctx, reads[m], window_bytes, &readers[m]);
        if (rc != LIME_OK) { std::cerr << "Error reading " << reads[m] << ": " << lime_last_error() << std::endl; return rc == LIME_ERR_IO ? -LIME_ERR_IO : 1; }
        if (trim && lime_seq_reader_set_trim(readers[m], q5, q3) != LIME_OK) { std::cerr << "Error reading " << reads[m] << ": " << lime_last_error() << std::endl; return 1; }
        if (cut_adapter && lime_seq_reader_set_adapter(readers[m], (const uint8_t *)adapters[m].data(), (uint32_t)adapters[m].size(), ad_overlap, ad_err) != LIME_OK) {
            std::cerr << "Error reading " << reads[m] << ": " << lime_last_error() << std::endl; return 1;
        }
        if (filter && lime_seq_reader_set_filter(readers[m], &flt) != LIME_OK) { std::cerr << "Error reading " << reads[m] << ": " << lime_last_error() << std::endl; return 1; }
        if (qc_report && lime_seq_reader_set_qc(readers[m], qc_pos) != LIME_OK) { std::cerr << "Error reading " << reads[m] << ": " << lime_last_error() << std::endl; return 1; }
    }
    if (batched && cut_overlap && lime_seq_reader_set_overlap(readers[0], readers[1], ov_overlap, ov_err) != LIME_OK) {
        std::cerr << "Error reading " << reads[0] << ": " << lime_last_error() << std::endl; return 1;
    }
    for (uint32_t m = 0; m < n_mates && !batched; ++m) {
        int rc;
        if (trim) {                                // the raw reads with their qualities, then the trimmed reads alone
            lime_docs *raw = nullptr;
            lime_trim_info_t ti;
            if ((rc = lime_docs_from_fastq_qual(ctx, reads[m], &raw)) == LIME_OK) {
                if (qc_report) rc = lime_docs_qc_dev(ctx, raw, qc_pos, nullptr, qc_before[m].data());
                if (rc == LIME_OK) rc = lime_docs_trim_dev(ctx, raw, q5, q3, nullptr, &mates[m], &ti);
                lime_docs_free(raw);
                if (rc == LIME_OK) print_trim(reads[m], q5, q3, ti);
            }
        } else if (qc_report && formats[m] == 1) {  // the report's quality tables: the reads keep their qualities, which no later step looks at
            if ((rc = lime_docs_from_fastq_qual(ctx, reads[m], &mates[m])) == LIME_OK) rc = lime_docs_qc_dev(ctx, mates[m], qc_pos, nullptr, qc_before[m].data());
        } else {
            rc = lime_docs_from_file(ctx, reads[m], &mates[m]);
            if (rc == LIME_OK && qc_report) rc = lime_docs_qc_dev(ctx, mates[m], qc_pos, nullptr, qc_before[m].data());
        }
        if (rc == LIME_OK && cut_adapter) {        // the reads as parsed or as the quality trim left them, then cut at their adapters
            lime_docs *whole = mates[m];
            lime_trim_info_t ti;
            mates[m] = nullptr;
            rc = lime_docs_trim_adapter_dev(ctx, whole, (const uint8_t *)adapters[m].data(), (uint32_t)adapters[m].size(), ad_overlap, ad_err, nullptr, &mates[m], &ti);
            lime_docs_free(whole);
            if (rc == LIME_OK) print_adapter(reads[m], adapters[m], ad_overlap, ad_err, ti);
        }
        if (rc == LIME_OK && filter) {             // what the trims left, filtered
            lime_docs *whole = mates[m];
            lime_filter_info_t fi;
            mates[m] = nullptr;
            rc = lime_docs_filter_dev(ctx, whole, &flt, nullptr, &mates[m], &fi);
            lime_docs_free(whole);
            if (rc == LIME_OK) print_filter(reads[m], flt, fi);
        }
        if (rc != LIME_OK) { std::cerr << "Error reading " << reads[m] << ": " << lime_last_error() << std::endl; return rc == LIME_ERR_IO ? -LIME_ERR_IO : 1; }
    }
    if (!batched && cut_overlap) {                 // last: what each mate's stages left, cut at the mates' overlap
        lime_docs *whole[2] = {mates[0], mates[1]};
        lime_overlap_info_t oi;
        mates[0] = mates[1] = nullptr;
        const int rc = lime_docs_trim_overlap_dev(ctx, whole[0], whole[1], ov_overlap, ov_err, nullptr, nullptr, &mates[0], &mates[1], &oi);
        lime_docs_free(whole[0]); lime_docs_free(whole[1]);
        if (rc != LIME_OK) { std::cerr << "Error reading " << reads[0] << ": " << lime_last_error() << std::endl; return 1; }
        print_overlap(reads[0], reads[1], ov_overlap, ov_err, oi);
    }
    for (uint32_t m = 0; m < n_mates && !batched && qc_report; ++m)     // the reads as they enter classification
        if (lime_docs_qc_dev(ctx, mates[m], qc_pos, nullptr, qc_after[m].data()) != LIME_OK) { std::cerr << "Error reading " << reads[m] << ": " << lime_last_error() << std::endl; return 1; }
    if (!batched) { uint32_t nd = 0; lime_docs_info(mates[0], &nd, nullptr); numReads = nd; }
    clk.mark(batched ? "readers" : "reads (parsed on the device)");
    lime_gindex *gi = nullptr;
    std::vector<lime_gindex *> shards;
    if (refs) {
        lime_docs *g = nullptr;
        const int rc = lime_docs_from_fasta(ctx, refs, &g);
        if (rc != LIME_OK) { std::cerr << "Error reading " << refs << ": " << lime_last_error() << std::endl; return rc == LIME_ERR_IO ? -LIME_ERR_IO : 1; }
        uint32_t nd = 0; uint64_t nt = 0;
        const uint8_t *d_text = nullptr; const uint64_t *d_off = nullptr;
        lime_docs_info(g, &nd, &nt);
        lime_docs_device(g, &d_text, &d_off);
        if (lime_gindex_build_dev(ctx, d_text, d_off, nd, nt, 0, trlcp, nullptr, &gi) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(1); }
        lime_docs_free(g);
    } else {
        for (uint32_t s = 0; s < n_shards; ++s) {
            if (lime_gindex_load(ctx, gidx[s], &gi) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(1); }
            shards.push_back(gi);
        }
        gi = shards[0];
    }
    if (shards.empty()) shards.push_back(gi);
    uint32_t numTarg = 0;
    for (lime_gindex *x : shards) { uint32_t nd = 0; lime_gindex_info(x, &nd, nullptr, nullptr, nullptr); numTarg += nd; }
    clk.mark("genome index");
    if (batched) std::cout << "numGenomes: " << numTarg << std::endl;        // (numReads is known after the last batch)
    else std::cout << "numReads: " << numReads << "\nnumGenomes: " << numTarg << std::endl;

    lime_taxonomy *tx = nullptr;
    std::cout << "Reading " << lineage << std::endl;
    if (lime_taxonomy_load(lineage, (int)rank, HIGHER, numTarg, &tx) != LIME_OK) { std::cerr << lime_classify_error() << std::endl; exit(1); }
    uint64_t counts[4] = {0, 0, 0, 0};
    if (batched) {
        BatchSink sink;
        sink.n_coll = 2 * n_mates; sink.n_shards = n_shards;
        if (lime_classification_writer_open(output, &sink.w) != LIME_OK) { std::cerr << lime_classify_error() << std::endl; exit(1); }
        std::cerr << "Start comparing..." << std::endl;
        uint64_t n_batches = 0;
        const int rc = n_shards == 1 ? lime_classify_sample_stream(ctx, n_mates, readers, gi, tx, alpha, norm, beta, EBWT, BIN, refs ? 0 : trlcp, batch_reads, batch_sink,
                                                                   &sink, counts, &numReads, &n_batches, nullptr)
                                     : lime_classify_sample_stream_shards(ctx, n_mates, readers, n_shards, shards.data(), tx, alpha, norm, beta, EBWT, BIN, trlcp,
                                                                          batch_reads, batch_sink, &sink, counts, &numReads, &n_batches, nullptr);
        if (rc != LIME_OK) {
            std::cerr << "Error: " << (sink.write_failed ? lime_classify_error() : lime_last_error()) << std::endl;
            lime_classification_writer_close(sink.w, 0);
            lime_shutdown(ctx);
            return 1;
        }
        std::cout << "numReads: " << numReads << " (" << n_batches << " batches of at most " << batch_reads << ")" << std::endl;
        for (uint32_t k = 0; k < 2 * n_mates; ++k)
            std::cout << reads[k >> 1] << (k & 1u ? " (reverse complements)" : "") << ": " << sink.n_clusters[k] << " clusters summed over the batches"
                      << (n_shards > 1 ? " and shards" : "") << ", maximum length " << sink.max_len[k] << " in a batch" << (n_shards > 1 ? " and shard" : "") << "." << std::endl;
        for (uint32_t m = 0; m < n_mates && trim; ++m) {
            lime_trim_info_t ti;
            lime_seq_reader_trim_info(readers[m], &ti);
            print_trim(reads[m], q5, q3, ti);
        }
        for (uint32_t m = 0; m < n_mates && cut_adapter; ++m) {
            lime_trim_info_t ti;
            lime_seq_reader_adapter_info(readers[m], &ti);
            print_adapter(reads[m], adapters[m], ad_overlap, ad_err, ti);
        }
        for (uint32_t m = 0; m < n_mates && filter; ++m) {
            lime_filter_info_t fi;
            lime_seq_reader_filter_info(readers[m], &fi);
            print_filter(reads[m], flt, fi);
        }
        if (cut_overlap) {
            lime_overlap_info_t oi;
            lime_seq_reader_overlap_info(readers[0], &oi);
            print_overlap(reads[0], reads[1], ov_overlap, ov_err, oi);
        }
        for (uint32_t m = 0; m < n_mates && qc_report; ++m) {
            lime_seq_reader_qc(readers[m], 0, qc_before[m].data());
            lime_seq_reader_qc(readers[m], 1, qc_after[m].data());
        }
        clk.mark("batches: reads, collections, classification");
        if (lime_classification_writer_close(sink.w, 1) != LIME_OK) { std::cerr << lime_classify_error() << std::endl; exit(1); }
        clk.mark("output file");
    } else {
        std::vector<lime_verdict_t> verdicts(numReads ? numReads : 1);
        std::vector<lime_stats_t> stats((size_t)n_shards * 4);
        std::cerr << "Start comparing..." << std::endl;
        const int rc = n_shards == 1 ? lime_classify_sample_dev(ctx, n_mates, mates, gi, tx, alpha, norm, beta, EBWT, BIN, refs ? 0 : trlcp, verdicts.data(), counts,
                                                                stats.data(), nullptr)
                                     : lime_classify_sample_shards_dev(ctx, n_mates, mates, n_shards, shards.data(), tx, alpha, norm, beta, EBWT, BIN, trlcp, verdicts.data(),
                                                                       counts, stats.data(), nullptr);
        if (rc != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(1); }
        for (uint32_t k = 0; k < 2 * n_mates; ++k) {
            uint64_t nc = 0, ml = 0;
            for (uint32_t s = 0; s < n_shards; ++s) { const lime_stats_t &x = stats[(size_t)s * 2 * n_mates + k]; nc += x.n_clusters; if (x.max_len > ml) ml = x.max_len; }
            if (n_shards == 1)
                std::cout << reads[k >> 1] << (k & 1u ? " (reverse complements)" : "") << ": " << nc << " clusters, maximum length " << ml << "." << std::endl;
            else
                std::cout << reads[k >> 1] << (k & 1u ? " (reverse complements)" : "") << ": " << nc << " clusters summed over the shards, maximum length " << ml
                          << " in a shard." << std::endl;
        }
        clk.mark("collections, classification");
        if (lime_write_classification(output, verdicts.data(), (uint32_t)numReads) != LIME_OK) { std::cerr << lime_classify_error() << std::endl; exit(1); }
        clk.mark("output file");
    }
    if (qc_report) {
        const uint64_t *before[2] = {qc_before[0].data(), qc_before[1].data()}, *after[2] = {qc_after[0].data(), qc_after[1].data()};
        if (lime_qc_report_write(qc_report, n_mates, reads.data(), formats, qc_pos, before, after) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(1); }
        std::cout << "Read statistics (" << qc_pos << " positions, before and after the stages): " << qc_report << std::endl;
    }
    lime_shutdown(ctx);
    lime_taxonomy_free(tx);
    std::cout << "Classification process at level " << rank << " completed.\nNumber of successfully classified reads: "
              << counts[0] << "/" << numReads << ";" << std::endl;
    if (HIGHER) std::cout << "\tClassified at higher taxonomic ranks: " << counts[3] << "." << std::endl;
    std::cout << "\tAmbiguously classified reads: " << counts[2] << "." << std::endl;
    std::cout << "\tNot classified reads: " << counts[1] << "." << std::endl;
    fprintf(stdout, "Time: %.6lf\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
