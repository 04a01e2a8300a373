// LiME_paired -- the reference's LiME_paired.sh (:44-79: four ClusterLCP, four ClusterBWT_DA, Classify 4) as ONE process:
//   LiME_paired File1_F File1_RC File2_F File2_RC output numReads numGenomes LineageFile readLen threads
// Each collection's <File>.lcp / .da / .ebwt goes through the device once (scan + clusterAnalyze + clusterChoose,
// lime_fused_choose_lists); its (idRef, sim) lists stay in HBM, the four are classified there (lime_classify_lists_dev) and only
// the verdicts (12 bytes per read) come back to be written as `output`.  Unlike the script it writes NO intermediate files:
// no .clrs, no .out, no .res.bin / .res.pos / .res.txt.  The script's constants: alpha 16, beta 0.25, taxRank 1
// (LiME_paired.sh:21-23).  The reference's compile-time switches are environment variables, as for the other drop-ins:
// LIME_EBWT (default 1), LIME_BIN (default 1: the values Classify's BIN=1 build reads; 0: the .res.txt ones), LIME_HIGHER (default 0).
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
    if (argc != 11) {
        std::cerr << "Error usage " << argv[0] << " File1_F File1_RC File2_F File2_RC output numReads numGenomes LineageFile readLen threads\n"
                  << "  reads <File>.lcp, <File>.da and <File>.ebwt of the four collections and writes only `output` (the classification\n"
                  << "  file); no .clrs, .out or .res.* files are written.  alpha 16, beta 0.25, taxRank 1 as in LiME_paired.sh;\n"
                  << "  LIME_EBWT, LIME_BIN, LIME_HIGHER as for ClusterBWT_DA / Classify." << std::endl;
        exit(1);
    }
    const uint32_t ALPHA = 16, RANK = 1;
    const float BETA = 0.25f;
    const int EBWT = env_flag("LIME_EBWT", 1), BIN = env_flag("LIME_BIN", 1), HIGHER = env_flag("LIME_HIGHER", 0);
    const char *files[4] = {argv[1], argv[2], argv[3], argv[4]};
    const std::string fileOutput = argv[5], fileTax = argv[8];
    unsigned numReads = 0, numTarg = 0;
    sscanf(argv[6], "%u", &numReads);
    sscanf(argv[7], "%u", &numTarg);
    unsigned char readLen = 0;                 // dataTypeSim, parsed with %hhu like ClusterBWT_DA (:519-521)
    sscanf(argv[9], "%hhu", &readLen);
    int threads = 1;
    sscanf(argv[10], "%d", &threads);
    io_threads_from_argv(threads);
    const uint32_t norm = (uint32_t)(readLen + 1 - ALPHA);        // ClusterBWT_DA.cpp:555

    lime_taxonomy *tx = nullptr;
    std::cout << "Reading " << fileTax << std::endl;
    if (lime_taxonomy_load(fileTax.c_str(), (int)RANK, HIGHER, numTarg, &tx) != LIME_OK) { std::cerr << lime_classify_error() << std::endl; exit(1); }
    lime_ctx *ctx = nullptr;
    if (lime_init(pick_device(), &ctx) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(EXIT_FAILURE); }
    clk.mark("taxonomy, lime_init (HIP runtime)");
    lime_lists *lists[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; ++k) {
        const std::string base = files[k];
        MappedFile lcp, da, bwt;
        if (!lcp.open(base + ".lcp")) { std::cerr << "Error opening " << base << ".lcp." << std::endl; exit(EXIT_FAILURE); }
        if (!da.open(base + ".da")) { std::cerr << "Error opening " << base << ".da." << std::endl; exit(EXIT_FAILURE); }
        if (EBWT && !bwt.open(base + ".ebwt")) { std::cerr << "Error opening " << base << ".ebwt." << std::endl; exit(EXIT_FAILURE); }
        uint64_t n = lcp.bytes / 4;
        if (da.bytes / 4 < n) n = da.bytes / 4;
        if (EBWT && bwt.bytes < n) n = bwt.bytes;
        lime_stats_t s;
        const int rc = lime_fused_choose_lists(ctx, (const uint32_t *)lcp.data, (const uint32_t *)da.data, EBWT ? (const uint8_t *)bwt.data : nullptr, n,
                                               numReads, numTarg, ALPHA, norm, BETA, &lists[k], &s);
        if (rc != LIME_OK) { std::cerr << "Error: " << base << ": " << lime_last_error() << std::endl; exit(1); }
        std::cout << base << ": " << s.n_clusters << " clusters, maximum length " << s.max_len << "." << std::endl;
        clk.mark("collection");
    }
    std::vector<lime_verdict_t> verdicts(numReads ? numReads : 1);
    uint64_t counts[4] = {0, 0, 0, 0};
    std::cerr << "Start comparing..." << std::endl;
    if (lime_classify_lists_dev(ctx, 4, lists, numTarg, tx, BIN, verdicts.data(), counts, nullptr) != LIME_OK) {
        std::cerr << lime_last_error() << std::endl; exit(1);
    }
    clk.mark("classification");
    if (lime_write_classification(fileOutput.c_str(), verdicts.data(), numReads) != LIME_OK) { std::cerr << lime_classify_error() << std::endl; exit(1); }
    clk.mark("output file");
    for (int k = 0; k < 4; ++k) lime_lists_free(lists[k]);
    lime_shutdown(ctx);
    lime_taxonomy_free(tx);
    std::cout << "Classification process at level " << RANK << " completed.\nNumber of successfully classified reads: "
              << counts[0] << "/" << numReads << ";" << std::endl;
    if (HIGHER) std::cout << "\tClassified at higher taxonomic ranks: " << counts[3] << "." << std::endl;
    std::cout << "\tAmbiguously classified reads: " << counts[2] << "." << std::endl;
    std::cout << "\tNot classified reads: " << counts[1] << "." << std::endl;
    fprintf(stdout, "Time: %.6lf\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return 0;
}
