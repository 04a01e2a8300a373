// LiME_fasta -- Preprocessing.sh + LiME_paired.sh for one sample, from FASTA or FASTQ files, as ONE process with nothing on disk in between:
//   LiME_fasta reads_1.fasta [reads_2.fasta] (--refs refs.fasta | --gidx file.gidx) --lineage LineageFile --readlen L --out output
//              [--alpha 16] [--beta 0.25] [--rank 1] [--trlcp k]
// Each reads file is FASTA or four-line FASTQ, decided by its first byte ('@': FASTQ; lime_docs_from_file), the mates each on their own;
// --refs is FASTA.  The files' bytes go to the device as they are and are parsed there; per collection (reads_1, its reverse
// complements, reads_2, its reverse complements: the script's `seqtk seq -r`) the reads are merged into the genome index, scanned and
// chosen from in HBM, the lists are classified there (lime_classify_sample_dev) and only the verdicts (12 bytes per read) come back to
// be written as `output`.  --refs parses the genomes with the same device parser and builds their index in the process; --gidx loads
// one that BuildIndex --refs wrote.  --trlcp k: lcp values truncated at k (eGap's option; with --gidx at most the index's).
// The defaults are the script's constants (LiME_paired.sh:21-23); norm = readLen + 1 - alpha (ClusterBWT_DA.cpp:555).  The reference's
// compile-time switches are environment variables, as for the other drop-ins: LIME_EBWT (default 1), LIME_BIN (default 1), LIME_HIGHER (0).
#include <string.h>
#include <chrono>
#include <iostream>
#include <string>
#include <vector>

#include "cli_common.h"

static int env_flag(const char *name, int dflt)
{
    const char *s = getenv(name);
    return s ? atoi(s) != 0 : dflt;
}

int main(int argc, char **argv)
{
    CliClock clk;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<const char *> reads;
    const char *refs = nullptr, *gidx = nullptr, *lineage = nullptr, *output = nullptr;
    unsigned alpha = 16, rank = 1, trlcp = 0;
    float beta = 0.25f;
    unsigned char readLen = 0;                 // dataTypeSim, parsed with %hhu like ClusterBWT_DA (:519-521)
    bool bad = false, have_len = false;
    for (int i = 1; i < argc; ++i) {
        const bool more = i + 1 < argc;
        if (!strcmp(argv[i], "--refs")) { if (more) refs = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--gidx")) { if (more) gidx = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--lineage")) { if (more) lineage = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--out")) { if (more) output = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--readlen")) { if (more && sscanf(argv[i + 1], "%hhu", &readLen) == 1) { ++i; have_len = true; } else bad = true; }
        else if (!strcmp(argv[i], "--alpha")) { if (more && sscanf(argv[i + 1], "%u", &alpha) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--beta")) { if (more && sscanf(argv[i + 1], "%f", &beta) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--rank")) { if (more && sscanf(argv[i + 1], "%u", &rank) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--trlcp")) { if (more && sscanf(argv[i + 1], "%u", &trlcp) == 1) ++i; else bad = true; }
        else reads.push_back(argv[i]);
    }
    if (reads.empty() || reads.size() > 2 || !refs == !gidx || !lineage || !output || !have_len) bad = true;
    if (bad) {
        std::cerr << "Error usage " << argv[0] << " reads_1.fasta [reads_2.fasta] (--refs refs.fasta | --gidx file.gidx) --lineage LineageFile --readlen L --out output\n"
                  << "           [--alpha 16] [--beta 0.25] [--rank 1] [--trlcp k]\n"
                  << "  classifies the reads of one sample (one file: single-end, two: paired-end) against the genomes of refs.fasta, or of an\n"
                  << "  index written by BuildIndex --refs, and writes only `output` (the classification file).  A reads file is FASTA or\n"
                  << "  four-line FASTQ, by its first byte ('@': FASTQ), each mate on its own; refs.fasta is FASTA.  --trlcp k: lcp values\n"
                  << "  truncated at k.  LIME_EBWT, LIME_BIN, LIME_HIGHER as for ClusterBWT_DA / Classify." << std::endl;
        exit(1);
    }
    const int EBWT = env_flag("LIME_EBWT", 1), BIN = env_flag("LIME_BIN", 1), HIGHER = env_flag("LIME_HIGHER", 0);
    const uint32_t norm = (uint32_t)(readLen + 1 - alpha);        // ClusterBWT_DA.cpp:555
    const uint32_t n_mates = (uint32_t)reads.size();

    lime_ctx *ctx = nullptr;
    if (lime_init(pick_device(), &ctx) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(EXIT_FAILURE); }
    clk.mark("lime_init (HIP runtime)");
    lime_docs *mates[2] = {nullptr, nullptr};
    uint32_t numReads = 0;
    for (uint32_t m = 0; m < n_mates; ++m) {
        const int rc = lime_docs_from_file(ctx, reads[m], &mates[m]);
        if (rc != LIME_OK) { std::cerr << "Error reading " << reads[m] << ": " << lime_last_error() << std::endl; return rc == LIME_ERR_IO ? -LIME_ERR_IO : 1; }
    }
    lime_docs_info(mates[0], &numReads, nullptr);
    clk.mark("reads (parsed on the device)");
    lime_gindex *gi = nullptr;
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
    } else if (lime_gindex_load(ctx, gidx, &gi) != LIME_OK) {
        std::cerr << "Error: " << lime_last_error() << std::endl; exit(1);
    }
    uint32_t numTarg = 0;
    lime_gindex_info(gi, &numTarg, nullptr, nullptr, nullptr);
    clk.mark("genome index");
    std::cout << "numReads: " << numReads << "\nnumGenomes: " << numTarg << std::endl;

    lime_taxonomy *tx = nullptr;
    std::cout << "Reading " << lineage << std::endl;
    if (lime_taxonomy_load(lineage, (int)rank, HIGHER, numTarg, &tx) != LIME_OK) { std::cerr << lime_classify_error() << std::endl; exit(1); }
    std::vector<lime_verdict_t> verdicts(numReads ? numReads : 1);
    uint64_t counts[4] = {0, 0, 0, 0};
    lime_stats_t stats[4];
    std::cerr << "Start comparing..." << std::endl;
    if (lime_classify_sample_dev(ctx, n_mates, mates, gi, tx, alpha, norm, beta, EBWT, BIN, refs ? 0 : trlcp, verdicts.data(), counts, stats, nullptr) != LIME_OK) {
        std::cerr << "Error: " << lime_last_error() << std::endl; exit(1);
    }
    for (uint32_t k = 0; k < 2 * n_mates; ++k)
        std::cout << reads[k >> 1] << (k & 1u ? " (reverse complements)" : "") << ": " << stats[k].n_clusters << " clusters, maximum length " << stats[k].max_len
                  << "." << std::endl;
    clk.mark("collections, classification");
    if (lime_write_classification(output, verdicts.data(), numReads) != LIME_OK) { std::cerr << lime_classify_error() << std::endl; exit(1); }
    clk.mark("output file");
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
