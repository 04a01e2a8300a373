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

struct StageOptions {                          // the read-preparation stages asked for
    bool trim = false; unsigned q5 = 0, q3 = 0;                                // --trim-qual
    std::string adapters[2]; int n_adapters = 0;   // --trim-adapter: [0] for reads_1 (and reads_2 when one is given), [1] for reads_2
    unsigned ad_overlap = 3, ad_err = 10; bool have_ad_opt = false, cut_adapter = false;
    lime_filter_t flt = {0, 0, 0, 0, LIME_FILTER_OFF, 0}; bool filter = false; // --trim-polyx, --max-len, --min-len, --max-n, --min-complexity
    unsigned ov_overlap = 30, ov_err = 10; bool cut_overlap = false;           // --trim-overlap
    const char *qc_report = nullptr; unsigned qc_pos = 256; bool have_qc_pos = false;      // --qc-report, --qc-positions
};

struct Options {                               // the command line
    std::vector<const char *> reads, gidx;
    const char *refs = nullptr, *lineage = nullptr, *output = nullptr;
    unsigned alpha = 16, rank = 1, trlcp = 0, batch_reads = 0;
    unsigned long long window_bytes = 0;
    bool batched = false, len_auto = false;    // --readlen auto: every read by its own length (LIME_NORM_PER_READ)
    float beta = 0.25f;
    unsigned char readLen = 0;                 // dataTypeSim, parsed with %hhu like ClusterBWT_DA (:519-521)
    StageOptions st;
    int EBWT = env_flag("LIME_EBWT", 1), BIN = env_flag("LIME_BIN", 1), HIGHER = env_flag("LIME_HIGHER", 0);       // the reference's compile-time switches
    uint32_t norm() const { return len_auto ? LIME_NORM_PER_READ : (uint32_t)(readLen + 1 - alpha); }                // ClusterBWT_DA.cpp:555
    uint32_t n_mates() const { return (uint32_t)reads.size(); }
    uint32_t n_shards() const { return refs ? 1u : (uint32_t)gidx.size(); }
};

// "Error reading FILE: text" and the program's end: with -LIME_ERR_IO where the file could not be read, with 1 for every refusal
[[noreturn]] void reading_failed(const char *file, int rc, const char *text = lime_last_error())
{
    std::cerr << "Error reading " << file << ": " << text << std::endl;
    exit(rc == LIME_ERR_IO ? -LIME_ERR_IO : 1);
}

// "Error: text" (or the text alone) and the program's end with 1
[[noreturn]] void die(const std::string &text, const char *lead = "Error: ") { std::cerr << lead << text << std::endl; exit(1); }
}

// the command line -> the options; a line that cannot be taken prints the usage and ends the program with 1
static Options parse_args(int argc, char **argv)
{
    Options o;
    StageOptions &s = o.st;
    bool bad = false, have_len = false, have_window = false;
    for (int i = 1; i < argc; ++i) {
        const bool more = i + 1 < argc;
        if (!strcmp(argv[i], "--refs")) { if (more) o.refs = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--gidx")) { if (more) o.gidx.push_back(argv[++i]); else bad = true; }
        else if (!strcmp(argv[i], "--lineage")) { if (more) o.lineage = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--out")) { if (more) o.output = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--readlen")) {
            if (more && !strcmp(argv[i + 1], "auto")) { ++i; have_len = true; o.len_auto = true; }
            else if (more && sscanf(argv[i + 1], "%hhu", &o.readLen) == 1) { ++i; have_len = true; o.len_auto = false; }
            else bad = true;
        }
        else if (!strcmp(argv[i], "--alpha")) { if (more && sscanf(argv[i + 1], "%u", &o.alpha) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--beta")) { if (more && sscanf(argv[i + 1], "%f", &o.beta) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--rank")) { if (more && sscanf(argv[i + 1], "%u", &o.rank) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--trlcp")) { if (more && sscanf(argv[i + 1], "%u", &o.trlcp) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--batch-reads")) { if (more && sscanf(argv[i + 1], "%u", &o.batch_reads) == 1 && o.batch_reads) { ++i; o.batched = true; } else bad = true; }
        else if (!strcmp(argv[i], "--trim-qual")) { if (more && parse_trim(argv[i + 1], &s.q5, &s.q3)) { ++i; s.trim = true; } else bad = true; }
        else if (!strcmp(argv[i], "--trim-adapter")) { if (more && parse_adapters(argv[i + 1], s.adapters, &s.n_adapters)) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--adapter-overlap")) { if (more && sscanf(argv[i + 1], "%u", &s.ad_overlap) == 1 && s.ad_overlap) { ++i; s.have_ad_opt = true; } else bad = true; }
        else if (!strcmp(argv[i], "--adapter-error")) { if (more && sscanf(argv[i + 1], "%u", &s.ad_err) == 1 && s.ad_err <= 50) { ++i; s.have_ad_opt = true; } else bad = true; }
        else if (!strcmp(argv[i], "--trim-polyx")) { if (more && parse_polyx(argv[i + 1], &s.flt)) { ++i; s.filter = true; } else bad = true; }
        else if (!strcmp(argv[i], "--max-len")) { if (more && parse_u32(argv[i + 1], &s.flt.max_len) && s.flt.max_len) { ++i; s.filter = true; } else bad = true; }
        else if (!strcmp(argv[i], "--min-len")) { if (more && parse_u32(argv[i + 1], &s.flt.min_len) && s.flt.min_len) { ++i; s.filter = true; } else bad = true; }
        else if (!strcmp(argv[i], "--max-n")) { if (more && parse_u32(argv[i + 1], &s.flt.max_n)) { ++i; s.filter = true; } else bad = true; }
        else if (!strcmp(argv[i], "--min-complexity")) {
            if (more && parse_u32(argv[i + 1], &s.flt.min_complexity) && s.flt.min_complexity && s.flt.min_complexity <= 100) { ++i; s.filter = true; } else bad = true;
        }
        else if (!strcmp(argv[i], "--trim-overlap")) { if (more && parse_overlap(argv[i + 1], &s.ov_overlap, &s.ov_err)) { ++i; s.cut_overlap = true; } else bad = true; }
        else if (!strcmp(argv[i], "--qc-report")) { if (more) s.qc_report = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--qc-positions")) { if (more && parse_u32(argv[i + 1], &s.qc_pos) && s.qc_pos && s.qc_pos <= LIME_QC_MAX_POS) { ++i; s.have_qc_pos = true; } else bad = true; }
        else if (!strcmp(argv[i], "--window-bytes")) { if (more && sscanf(argv[i + 1], "%llu", &o.window_bytes) == 1 && o.window_bytes) { ++i; have_window = true; } else bad = true; }
        else o.reads.push_back(argv[i]);
    }
    if (have_window && !o.batched) bad = true;
    if (s.have_qc_pos && !s.qc_report) bad = true;
    if (s.trim && !o.len_auto) bad = true;         // (a fixed norm on trimmed reads)
    s.cut_adapter = s.n_adapters > 0;
    if (s.cut_adapter && !o.len_auto) bad = true;  // (the same)
    if (s.have_ad_opt && !s.cut_adapter) bad = true;
    if ((s.flt.polyx_mask || s.flt.max_len) && !o.len_auto) bad = true;        // (the same; the three filters only empty reads)
    if (s.cut_overlap && (!o.len_auto || o.reads.size() != 2)) bad = true;     // (the same; and a pair is two files)
    if (s.n_adapters == 2 && o.reads.size() != 2) bad = true;
    for (int k = 0; k < s.n_adapters; ++k) if (s.ad_overlap > s.adapters[k].size()) bad = true;
    if (s.n_adapters == 1) s.adapters[1] = s.adapters[0];
    if (o.reads.empty() || o.reads.size() > 2 || !o.refs == o.gidx.empty() || !o.lineage || !o.output || !have_len) bad = true;
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
    return o;
}

namespace {
struct StageInfo { lime_trim_info_t trim; lime_filter_info_t filter; };        // a mate stage's counts: the member of its kind

// One stage of one mate, both modes side by side: is it asked for, set it on a reader (--batch-reads), run it on whole documents, its counts
// from a reader, its line.  THE TABLE'S ORDER IS THE STAGES' ORDER, the one of lime_seq_reader (include/lime_hip.h): a new stage is one entry
struct MateStage {
    bool StageOptions::*on;
    int (*set)(lime_seq_reader *, const StageOptions &, uint32_t m);
    int (*run)(lime_ctx *, const StageOptions &, uint32_t m, const lime_docs *in, lime_docs **out, StageInfo *);
    int (*fetch)(const lime_seq_reader *, StageInfo *);
    void (*print)(const char *file, const StageOptions &, uint32_t m, const StageInfo &);
};
const MateStage MATE_STAGES[] = {
    {   // --trim-qual: the raw reads with their qualities, then the trimmed reads alone
        &StageOptions::trim,
        [](lime_seq_reader *r, const StageOptions &s, uint32_t) { return lime_seq_reader_set_trim(r, s.q5, s.q3); },
        [](lime_ctx *c, const StageOptions &s, uint32_t, const lime_docs *in, lime_docs **out, StageInfo *i) {
            return lime_docs_trim_dev(c, in, s.q5, s.q3, nullptr, out, &i->trim); },
        [](const lime_seq_reader *r, StageInfo *i) { return lime_seq_reader_trim_info(r, &i->trim); },
        [](const char *file, const StageOptions &s, uint32_t, const StageInfo &i) { print_trim(file, s.q5, s.q3, i.trim); } },
    {   // --trim-adapter: the reads as parsed or as the quality trim left them, cut at their mate's adapter
        &StageOptions::cut_adapter,
        [](lime_seq_reader *r, const StageOptions &s, uint32_t m) {
            return lime_seq_reader_set_adapter(r, (const uint8_t *)s.adapters[m].data(), (uint32_t)s.adapters[m].size(), s.ad_overlap, s.ad_err); },
        [](lime_ctx *c, const StageOptions &s, uint32_t m, const lime_docs *in, lime_docs **out, StageInfo *i) {
            return lime_docs_trim_adapter_dev(c, in, (const uint8_t *)s.adapters[m].data(), (uint32_t)s.adapters[m].size(), s.ad_overlap, s.ad_err, nullptr, out, &i->trim); },
        [](const lime_seq_reader *r, StageInfo *i) { return lime_seq_reader_adapter_info(r, &i->trim); },
        [](const char *file, const StageOptions &s, uint32_t m, const StageInfo &i) { print_adapter(file, s.adapters[m], s.ad_overlap, s.ad_err, i.trim); } },
    {   // the read filter: what the trims left, filtered
        &StageOptions::filter,
        [](lime_seq_reader *r, const StageOptions &s, uint32_t) { return lime_seq_reader_set_filter(r, &s.flt); },
        [](lime_ctx *c, const StageOptions &s, uint32_t, const lime_docs *in, lime_docs **out, StageInfo *i) {
            return lime_docs_filter_dev(c, in, &s.flt, nullptr, out, &i->filter); },
        [](const lime_seq_reader *r, StageInfo *i) { return lime_seq_reader_filter_info(r, &i->filter); },
        [](const char *file, const StageOptions &s, uint32_t, const StageInfo &i) { print_filter(file, s.flt, i.filter); } },
};

struct Sample {                                // the reads: whole documents, or readers with --batch-reads
    lime_docs *mates[2] = {nullptr, nullptr}; lime_seq_reader *readers[2] = {nullptr, nullptr};
    int formats[2] = {0, 0}; uint64_t numReads = 0;
    std::vector<uint64_t> qc_before[2], qc_after[2];     // --qc-report: the tables of each reads file
};

struct Index { std::vector<lime_gindex *> shards; uint32_t numTarg = 0; lime_taxonomy *tx = nullptr; };    // the genome index, whole or in shards
}

// the shards must agree and the lineage must hold their genomes: known before a device is opened
static void probe_shards(const Options &o)
{
    uint64_t total = 0;
    uint32_t cap0 = 0; uint8_t term0 = 0;
    for (uint32_t s = 0; s < o.n_shards(); ++s) {
        uint32_t nd = 0, cap = 0; uint8_t term = 0;
        if (lime_gindex_probe(o.gidx[s], &nd, nullptr, &cap, &term) != LIME_OK) die(lime_last_error());
        if (s == 0) { cap0 = cap; term0 = term; }
        else if (cap != cap0 || term != term0)
            die(std::string(o.gidx[s]) + " was built with --trlcp " + std::to_string(cap) + " and terminator " + std::to_string((unsigned)term) + ", " + o.gidx[0] +
                " with --trlcp " + std::to_string(cap0) + " and terminator " + std::to_string((unsigned)term0) + ": the shards of one database are built alike.");
        total += nd;
    }
    if (total > 0xFFFFFFFFull) die("the index shards hold " + std::to_string(total) + " genomes; ids are 32 bits.");
    lime_taxonomy *probe = nullptr;
    if (lime_taxonomy_load(o.lineage, (int)o.rank, env_flag("LIME_HIGHER", 0), (uint32_t)total, &probe) != LIME_OK)
        die(std::string(o.lineage) + " does not describe the " + std::to_string(total) + " genomes of the " + std::to_string(o.n_shards()) + " index shards: " +
            lime_classify_error());
    lime_taxonomy_free(probe);
}

// the reads files' formats, where a stage asks for them: known before a device is opened, like the shards' headers
static void probe_reads(const Options &o, Sample &sm)
{
    const StageOptions &s = o.st;
    for (uint32_t m = 0; m < o.n_mates() && (s.trim || s.qc_report); ++m) {
        const int rc = lime_seq_format(o.reads[m], &sm.formats[m]);
        if (rc != LIME_OK) reading_failed(o.reads[m], rc);
        if (s.qc_report) { sm.qc_before[m].assign(LIME_QC_WORDS(s.qc_pos), 0); sm.qc_after[m].assign(LIME_QC_WORDS(s.qc_pos), 0); }
        if (s.trim && sm.formats[m] != 1) reading_failed(o.reads[m], LIME_ERR_ARG, "--trim-qual needs the qualities of a FASTQ file; this one is FASTA.");
    }
}

// --batch-reads: a reader per reads file with every stage set on it, in the table's order; the pair's overlap cut last
static void open_readers(lime_ctx *ctx, const Options &o, Sample &sm)
{
    const StageOptions &s = o.st;
    for (uint32_t m = 0; m < o.n_mates(); ++m) {
        int rc = lime_seq_reader_open(ctx, o.reads[m], o.window_bytes, &sm.readers[m]);
        for (const MateStage &stage : MATE_STAGES)
            if (rc == LIME_OK && (s.*stage.on)) rc = stage.set(sm.readers[m], s, m);
        if (rc == LIME_OK && s.qc_report) rc = lime_seq_reader_set_qc(sm.readers[m], s.qc_pos);
        if (rc != LIME_OK) reading_failed(o.reads[m], rc);
    }
    if (s.cut_overlap) {
        const int rc = lime_seq_reader_set_overlap(sm.readers[0], sm.readers[1], s.ov_overlap, s.ov_err);
        if (rc != LIME_OK) reading_failed(o.reads[0], rc);
    }
}

// the whole files: parsed, counted as parsed, each mate's stages in the table's order with a line each, the overlap cut last, counted again
static void read_whole(lime_ctx *ctx, const Options &o, Sample &sm)
{
    const StageOptions &s = o.st;
    for (uint32_t m = 0; m < o.n_mates(); ++m) {
        lime_docs *&d = sm.mates[m];
        // with the qualities for the quality trim and for the report's quality tables (the reads then keep them: no later step looks at them)
        int rc = s.trim || (s.qc_report && sm.formats[m] == 1) ? lime_docs_from_fastq_qual(ctx, o.reads[m], &d) : lime_docs_from_file(ctx, o.reads[m], &d);
        if (rc == LIME_OK && s.qc_report) rc = lime_docs_qc_dev(ctx, d, s.qc_pos, nullptr, sm.qc_before[m].data());
        for (const MateStage &stage : MATE_STAGES) {
            if (rc != LIME_OK || !(s.*stage.on)) continue;
            lime_docs *in = d;
            StageInfo info;
            d = nullptr;
            rc = stage.run(ctx, s, m, in, &d, &info);
            lime_docs_free(in);
            if (rc == LIME_OK) stage.print(o.reads[m], s, m, info);
        }
        if (rc != LIME_OK) reading_failed(o.reads[m], rc);
    }
    if (s.cut_overlap) {
        lime_docs *whole[2] = {sm.mates[0], sm.mates[1]};
        lime_overlap_info_t oi;
        sm.mates[0] = sm.mates[1] = nullptr;
        const int rc = lime_docs_trim_overlap_dev(ctx, whole[0], whole[1], s.ov_overlap, s.ov_err, nullptr, nullptr, &sm.mates[0], &sm.mates[1], &oi);
        lime_docs_free(whole[0]); lime_docs_free(whole[1]);
        if (rc != LIME_OK) reading_failed(o.reads[0], rc);
        print_overlap(o.reads[0], o.reads[1], s.ov_overlap, s.ov_err, oi);
    }
    for (uint32_t m = 0; m < o.n_mates() && s.qc_report; ++m) {
        const int rc = lime_docs_qc_dev(ctx, sm.mates[m], s.qc_pos, nullptr, sm.qc_after[m].data());
        if (rc != LIME_OK) reading_failed(o.reads[m], rc);
    }
    uint32_t nd = 0;
    lime_docs_info(sm.mates[0], &nd, nullptr);
    sm.numReads = nd;
}

// the genome index: built from --refs in the process, or every --gidx loaded
static void load_index(lime_ctx *ctx, const Options &o, Index &ix)
{
    lime_gindex *gi = nullptr;
    if (o.refs) {
        lime_docs *g = nullptr;
        const int rc = lime_docs_from_fasta(ctx, o.refs, &g);
        if (rc != LIME_OK) reading_failed(o.refs, rc);
        uint32_t nd = 0; uint64_t nt = 0;
        const uint8_t *d_text = nullptr; const uint64_t *d_off = nullptr;
        lime_docs_info(g, &nd, &nt);
        lime_docs_device(g, &d_text, &d_off);
        if (lime_gindex_build_dev(ctx, d_text, d_off, nd, nt, 0, o.trlcp, nullptr, &gi) != LIME_OK) die(lime_last_error());
        lime_docs_free(g);
        ix.shards.push_back(gi);
    } else {
        for (const char *file : o.gidx) {
            if (lime_gindex_load(ctx, file, &gi) != LIME_OK) die(lime_last_error());
            ix.shards.push_back(gi);
        }
    }
    for (lime_gindex *x : ix.shards) { uint32_t nd = 0; lime_gindex_info(x, &nd, nullptr, nullptr, nullptr); ix.numTarg += nd; }
}

// --batch-reads: the sample batch by batch into the output file, then the collections' lines, each stage's line for every mate, the pair's
static void classify_batched(lime_ctx *ctx, const Options &o, const Index &ix, Sample &sm, uint64_t counts[4], CliClock &clk)
{
    const StageOptions &s = o.st;
    const uint32_t n_mates = o.n_mates(), n_shards = o.n_shards();
    BatchSink sink;
    sink.n_coll = 2 * n_mates; sink.n_shards = n_shards;
    if (lime_classification_writer_open(o.output, &sink.w) != LIME_OK) die(lime_classify_error(), "");
    std::cerr << "Start comparing..." << std::endl;
    uint64_t n_batches = 0;
    const int rc = n_shards == 1 ? lime_classify_sample_stream(ctx, n_mates, sm.readers, ix.shards[0], ix.tx, o.alpha, o.norm(), o.beta, o.EBWT, o.BIN, o.refs ? 0 : o.trlcp,
                                                               o.batch_reads, batch_sink, &sink, counts, &sm.numReads, &n_batches, nullptr)
                                 : lime_classify_sample_stream_shards(ctx, n_mates, sm.readers, n_shards, ix.shards.data(), ix.tx, o.alpha, o.norm(), o.beta, o.EBWT, o.BIN,
                                                                      o.trlcp, o.batch_reads, batch_sink, &sink, counts, &sm.numReads, &n_batches, nullptr);
    if (rc != LIME_OK) {
        std::cerr << "Error: " << (sink.write_failed ? lime_classify_error() : lime_last_error()) << std::endl;
        lime_classification_writer_close(sink.w, 0);
        lime_shutdown(ctx);
        exit(1);
    }
    std::cout << "numReads: " << sm.numReads << " (" << n_batches << " batches of at most " << o.batch_reads << ")" << std::endl;
    for (uint32_t k = 0; k < 2 * n_mates; ++k)
        std::cout << o.reads[k >> 1] << (k & 1u ? " (reverse complements)" : "") << ": " << sink.n_clusters[k] << " clusters summed over the batches"
                  << (n_shards > 1 ? " and shards" : "") << ", maximum length " << sink.max_len[k] << " in a batch" << (n_shards > 1 ? " and shard" : "") << "." << std::endl;
    for (const MateStage &stage : MATE_STAGES)
        for (uint32_t m = 0; m < n_mates && (s.*stage.on); ++m) {
            StageInfo info;
            stage.fetch(sm.readers[m], &info);
            stage.print(o.reads[m], s, m, info);
        }
    if (s.cut_overlap) {
        lime_overlap_info_t oi;
        lime_seq_reader_overlap_info(sm.readers[0], &oi);
        print_overlap(o.reads[0], o.reads[1], s.ov_overlap, s.ov_err, oi);
    }
    for (uint32_t m = 0; m < n_mates && s.qc_report; ++m) {
        lime_seq_reader_qc(sm.readers[m], 0, sm.qc_before[m].data());
        lime_seq_reader_qc(sm.readers[m], 1, sm.qc_after[m].data());
    }
    clk.mark("batches: reads, collections, classification");
    if (lime_classification_writer_close(sink.w, 1) != LIME_OK) die(lime_classify_error(), "");
    clk.mark("output file");
}

// the whole sample in one call, the collections' lines, the output file
static void classify_whole(lime_ctx *ctx, const Options &o, const Index &ix, const Sample &sm, uint64_t counts[4], CliClock &clk)
{
    const uint32_t n_mates = o.n_mates(), n_shards = o.n_shards();
    std::vector<lime_verdict_t> verdicts(sm.numReads ? sm.numReads : 1);
    std::vector<lime_stats_t> stats((size_t)n_shards * 4);
    std::cerr << "Start comparing..." << std::endl;
    const int rc = n_shards == 1 ? lime_classify_sample_dev(ctx, n_mates, sm.mates, ix.shards[0], ix.tx, o.alpha, o.norm(), o.beta, o.EBWT, o.BIN, o.refs ? 0 : o.trlcp,
                                                            verdicts.data(), counts, stats.data(), nullptr)
                                 : lime_classify_sample_shards_dev(ctx, n_mates, sm.mates, n_shards, ix.shards.data(), ix.tx, o.alpha, o.norm(), o.beta, o.EBWT, o.BIN, o.trlcp,
                                                                   verdicts.data(), counts, stats.data(), nullptr);
    if (rc != LIME_OK) die(lime_last_error());
    for (uint32_t k = 0; k < 2 * n_mates; ++k) {
        uint64_t nc = 0, ml = 0;
        for (uint32_t s = 0; s < n_shards; ++s) { const lime_stats_t &x = stats[(size_t)s * 2 * n_mates + k]; nc += x.n_clusters; if (x.max_len > ml) ml = x.max_len; }
        std::cout << o.reads[k >> 1] << (k & 1u ? " (reverse complements)" : "") << ": " << nc << (n_shards == 1 ? " clusters" : " clusters summed over the shards")
                  << ", maximum length " << ml << (n_shards == 1 ? "." : " in a shard.") << std::endl;
    }
    clk.mark("collections, classification");
    if (lime_write_classification(o.output, verdicts.data(), (uint32_t)sm.numReads) != LIME_OK) die(lime_classify_error(), "");
    clk.mark("output file");
}

int main(int argc, char **argv)
{
    CliClock clk;
    const auto t0 = std::chrono::steady_clock::now();
    const Options o = parse_args(argc, argv);
    const StageOptions &s = o.st;
    if (o.n_shards() > 1) probe_shards(o);
    Sample sm;
    probe_reads(o, sm);
    lime_ctx *ctx = nullptr;
    if (lime_init(pick_device(), &ctx) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(EXIT_FAILURE); }
    clk.mark("lime_init (HIP runtime)");
    if (o.batched) open_readers(ctx, o, sm);
    else read_whole(ctx, o, sm);
    clk.mark(o.batched ? "readers" : "reads (parsed on the device)");
    Index ix;
    load_index(ctx, o, ix);
    clk.mark("genome index");
    if (o.batched) std::cout << "numGenomes: " << ix.numTarg << std::endl;        // (numReads is known after the last batch)
    else std::cout << "numReads: " << sm.numReads << "\nnumGenomes: " << ix.numTarg << std::endl;
    std::cout << "Reading " << o.lineage << std::endl;
    if (lime_taxonomy_load(o.lineage, (int)o.rank, o.HIGHER, ix.numTarg, &ix.tx) != LIME_OK) die(lime_classify_error(), "");
    uint64_t counts[4] = {0, 0, 0, 0};
    if (o.batched) classify_batched(ctx, o, ix, sm, counts, clk);
    else classify_whole(ctx, o, ix, sm, counts, clk);
    if (s.qc_report) {
        const uint64_t *before[2] = {sm.qc_before[0].data(), sm.qc_before[1].data()}, *after[2] = {sm.qc_after[0].data(), sm.qc_after[1].data()};
        if (lime_qc_report_write(s.qc_report, o.n_mates(), o.reads.data(), sm.formats, s.qc_pos, before, after) != LIME_OK) die(lime_last_error());
        std::cout << "Read statistics (" << s.qc_pos << " positions, before and after the stages): " << s.qc_report << std::endl;
    }
    lime_shutdown(ctx);
    lime_taxonomy_free(ix.tx);
    std::cout << "Classification process at level " << o.rank << " completed.\nNumber of successfully classified reads: "
              << counts[0] << "/" << sm.numReads << ";" << std::endl;
    if (o.HIGHER) std::cout << "\tClassified at higher taxonomic ranks: " << counts[3] << "." << std::endl;
    std::cout << "\tAmbiguously classified reads: " << counts[2] << "." << std::endl;
    std::cout << "\tNot classified reads: " << counts[1] << "." << std::endl;
    fprintf(stdout, "Time: %.6lf\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
