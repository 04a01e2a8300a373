// BuildIndex -- the preprocessing the reference leaves to BCR_LCP_GSA / eGSA / eGap (Preprocessing.sh), from FASTA files, on the GPU:
//   BuildIndex reads.fasta refs.fasta outBase [--rc] [--trlcp k]
// writes outBase.ebwt (u8), outBase.lcp and outBase.da (u32, little-endian, no header: what ClusterLCP / ClusterBWT_DA / LiME_paired
// read) of the collection reads + genomes and prints numReads and numGenomes.  --rc reverse-complements the READS only (the script's
// `seqtk seq -r`): four runs (reads_1, reads_1 --rc, reads_2, reads_2 --rc) give the four collections of LiME_paired.  --trlcp k stores
// min(lcp, k) (eGap's option; k >= alpha changes no result downstream).  A thin shell over lime_fasta_read / lime_build_index.
// The reads file may be four-line FASTQ instead (first byte '@': lime_seq_format, then lime_fastq_read); refs.fasta is FASTA.
// The genome database indexed once and every read set merged into it (the script's eGSA once, eGap four times):
//   BuildIndex --refs refs.fasta outBase [--trlcp k]               writes outBase.gidx (lime_gindex_build / _save), prints numGenomes
//   BuildIndex reads.fasta --gidx file.gidx outBase [--rc] [--trlcp k]   the one-step form's three files and output (lime_merge_index)
// A genome database of any size, cut into index shards (lime_gindex_shard_plan: consecutive genomes while a shard's positions, symbols +
// one terminator per genome, stay <= P; a genome is never cut):
//   BuildIndex --refs refs.fasta outBase --shard-positions P [--trlcp k]   writes outBase.000.gidx, outBase.001.gidx, ... and prints each
// name with its genomes and positions.  The file is read on the host and the shards are built and saved one at a time, so device memory
// holds one shard and refs.fasta may hold more than 2^32 - 1 positions.  LiME_fasta takes the shards with one --gidx each, in this order.
#include <string.h>
#include <algorithm>
#include <iostream>
#include <string>
#include <vector>

#include "cli_common.h"

static bool write_file(const std::string &path, const void *data, size_t bytes)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = !bytes || fwrite(data, 1, bytes, f) == bytes;
    return (fclose(f) == 0) && ok;
}

// the positional reads file: FASTA or four-line FASTQ by its first byte
static int read_reads(const char *path, int rc_reads, uint8_t **text, uint64_t **off, uint32_t *nd)
{
    int format = 0;
    int rc = lime_seq_format(path, &format);
    if (rc == LIME_OK) rc = format == 1 ? lime_fastq_read(path, rc_reads, text, off, nd) : lime_fasta_read(path, rc_reads, text, off, nd);
    if (rc == LIME_OK) return 0;
    std::cerr << "Error reading " << path << "." << std::endl;
    if (format == 1 && rc == LIME_ERR_ARG) std::cerr << lime_last_error() << std::endl;
    return rc == LIME_ERR_IO ? -LIME_ERR_IO : 1;
}

// the two forms around a genome index file: refs.fasta -> outBase.gidx, and reads.fasta + file.gidx -> the three files
static int two_step(CliClock &clk, bool refs_only, const char *gidx, const char *fasta, const std::string &base, int rc_reads, unsigned trlcp,
                    unsigned long long shard_positions)
{
    uint8_t *text = nullptr;
    uint64_t *off = nullptr;
    uint32_t nd = 0;
    if (refs_only) {
        const int rc = lime_fasta_read(fasta, 0, &text, &off, &nd);
        if (rc != LIME_OK) { std::cerr << "Error reading " << fasta << "." << std::endl; return rc == LIME_ERR_IO ? -LIME_ERR_IO : 1; }
    } else {
        const int rc = read_reads(fasta, rc_reads, &text, &off, &nd);
        if (rc) return rc;
    }
    clk.mark("sequence file");
    lime_ctx *ctx = nullptr;
    if (lime_init(pick_device(), &ctx) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(EXIT_FAILURE); }
    clk.mark("lime_init (HIP runtime)");
    lime_gindex *gi = nullptr;
    if (refs_only && shard_positions) {
        std::vector<uint32_t> first((size_t)nd + 2);
        uint32_t n_shards = 0;
        if (lime_gindex_shard_plan(off, nd, shard_positions, first.data(), (uint32_t)std::min<uint64_t>((uint64_t)nd + 2, 0xFFFFFFFFull), &n_shards) != LIME_OK) {
            std::cerr << "Error: " << lime_last_error() << std::endl; return 1;
        }
        std::cout << "numGenomes: " << nd << "\nsymbols: " << off[nd] + nd << "\nshards: " << n_shards << std::endl;
        for (uint32_t s = 0; s < n_shards; ++s) {                       // one shard at a time on the device
            const uint32_t d0 = first[s], cnt = first[s + 1] - d0;
            std::vector<uint64_t> soff((size_t)cnt + 1);
            for (uint32_t k = 0; k <= cnt; ++k) soff[k] = off[d0 + k] - off[d0];
            char num[16];
            snprintf(num, sizeof num, ".%03u", s);
            const std::string name = base + num + ".gidx";
            if (lime_gindex_build(ctx, text + off[d0], soff.data(), cnt, 0, trlcp, &gi) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(1); }
            if (lime_gindex_save(gi, name.c_str()) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; return -LIME_ERR_IO; }
            lime_gindex_free(gi);
            gi = nullptr;
            std::cout << name << ": " << cnt << " genomes, " << soff[cnt] + cnt << " positions" << std::endl;
        }
        clk.mark("index shards");
        lime_shutdown(ctx);
        lime_free(text); lime_free(off);
        return 0;
    }
    if (refs_only) {
        if (lime_gindex_build(ctx, text, off, nd, 0, trlcp, &gi) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(1); }
        clk.mark("index");
        if (lime_gindex_save(gi, (base + ".gidx").c_str()) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; return -LIME_ERR_IO; }
        clk.mark("output file");
        lime_shutdown(ctx);
        std::cout << "numGenomes: " << nd << "\nsymbols: " << off[nd] + nd << std::endl;
        lime_free(text); lime_free(off);
        return 0;
    }
    if (lime_gindex_load(ctx, gidx, &gi) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(1); }
    clk.mark("genome index");
    uint32_t n_refs = 0;
    lime_gindex_info(gi, &n_refs, nullptr, nullptr, nullptr);
    if ((uint64_t)nd + n_refs > 0xFFFFFFFFull) { std::cerr << "Error: too many sequences." << std::endl; return 1; }
    const uint64_t n = lime_merge_size(gi, off, nd);
    std::vector<uint8_t> ebwt(n ? n : 1);
    std::vector<uint32_t> lcp(n ? n : 1), da(n ? n : 1);
    if (lime_merge_index(ctx, text, off, nd, gi, trlcp, ebwt.data(), lcp.data(), da.data()) != LIME_OK) {
        std::cerr << "Error: " << lime_last_error() << std::endl; exit(1);
    }
    clk.mark("merge");
    lime_shutdown(ctx);
    lime_free(text); lime_free(off);
    if (!write_file(base + ".ebwt", ebwt.data(), n) || !write_file(base + ".lcp", lcp.data(), n * 4) || !write_file(base + ".da", da.data(), n * 4)) {
        std::cerr << "Error writing " << base << ".ebwt / .lcp / .da." << std::endl;
        return -LIME_ERR_IO;
    }
    clk.mark("output files");
    std::cout << "numReads: " << nd << "\nnumGenomes: " << n_refs << "\nsymbols: " << n << std::endl;
    return 0;
}

int main(int argc, char **argv)
{
    CliClock clk;
    std::vector<const char *> pos;
    int rc_reads = 0;
    unsigned trlcp = 0;
    unsigned long long shard_positions = 0;
    bool bad = false, refs_only = false, sharded = false;
    const char *gidx = nullptr;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--rc")) rc_reads = 1;
        else if (!strcmp(argv[i], "--refs")) refs_only = true;
        else if (!strcmp(argv[i], "--gidx")) { if (i + 1 < argc) gidx = argv[++i]; else bad = true; }
        else if (!strcmp(argv[i], "--trlcp")) { if (i + 1 < argc && sscanf(argv[i + 1], "%u", &trlcp) == 1) ++i; else bad = true; }
        else if (!strcmp(argv[i], "--shard-positions")) { if (i + 1 < argc && sscanf(argv[i + 1], "%llu", &shard_positions) == 1 && shard_positions) { ++i; sharded = true; } else bad = true; }
        else pos.push_back(argv[i]);
    }
    if (sharded && !refs_only) bad = true;
    if ((refs_only && (gidx || rc_reads)) || pos.size() != ((refs_only || gidx) ? 2u : 3u)) bad = true;
    if (bad) {
        std::cerr << "Error usage " << argv[0] << " reads.fasta refs.fasta outBase [--rc] [--trlcp k]\n"
                  << "  writes outBase.ebwt, outBase.lcp, outBase.da of the collection reads + genomes; --rc: the reads' reverse complements;\n"
                  << "  --trlcp k: lcp values truncated at k.  reads.fasta may be four-line FASTQ (first byte '@'); refs.fasta is FASTA.\n"
                  << "or " << argv[0] << " --refs refs.fasta outBase [--trlcp k]\n"
                  << "  writes outBase.gidx, the index of the genomes alone;\n"
                  << "or " << argv[0] << " --refs refs.fasta outBase --shard-positions P [--trlcp k]\n"
                  << "  writes outBase.000.gidx, outBase.001.gidx, ...: consecutive genomes while a shard's positions (symbols + one terminator\n"
                  << "  per genome) stay <= P, built one at a time (LiME_fasta takes them with one --gidx each, in this order);\n"
                  << "or " << argv[0] << " reads.fasta --gidx file.gidx outBase [--rc] [--trlcp k]\n"
                  << "  writes the three files from the reads and a genome index (--trlcp: at most the index's)." << std::endl;
        exit(1);
    }
    if (refs_only || gidx) return two_step(clk, refs_only, gidx, pos[0], pos[1], rc_reads, trlcp, shard_positions);
    const std::string base = pos[2];
    uint8_t *text[2] = {nullptr, nullptr};
    uint64_t *off[2] = {nullptr, nullptr};
    uint32_t nd[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        if (k == 0) { const int rc = read_reads(pos[0], rc_reads, &text[0], &off[0], &nd[0]); if (rc) return rc; continue; }
        const int rc = lime_fasta_read(pos[k], 0, &text[k], &off[k], &nd[k]);
        if (rc != LIME_OK) { std::cerr << "Error reading " << pos[k] << "." << std::endl; return rc == LIME_ERR_IO ? -LIME_ERR_IO : 1; }
    }
    clk.mark("sequence files");
    if ((uint64_t)nd[0] + nd[1] > 0xFFFFFFFFull) { std::cerr << "Error: too many sequences." << std::endl; return 1; }
    const uint32_t n_docs = nd[0] + nd[1];
    const uint64_t n_reads_sym = off[0][nd[0]], n_text = n_reads_sym + off[1][nd[1]];
    std::vector<uint8_t> all(n_text ? n_text : 1);
    if (n_reads_sym) memcpy(all.data(), text[0], n_reads_sym);
    if (n_text > n_reads_sym) memcpy(all.data() + n_reads_sym, text[1], n_text - n_reads_sym);
    std::vector<uint64_t> doc_off((size_t)n_docs + 1);
    for (uint32_t k = 0; k <= nd[0]; ++k) doc_off[k] = off[0][k];
    for (uint32_t k = 0; k <= nd[1]; ++k) doc_off[nd[0] + k] = n_reads_sym + off[1][k];
    for (int k = 0; k < 2; ++k) { lime_free(text[k]); lime_free(off[k]); }
    const uint64_t n = lime_index_size(doc_off.data(), n_docs);
    std::vector<uint8_t> ebwt(n ? n : 1);
    std::vector<uint32_t> lcp(n ? n : 1), da(n ? n : 1);
    lime_ctx *ctx = nullptr;
    if (lime_init(pick_device(), &ctx) != LIME_OK) { std::cerr << "Error: " << lime_last_error() << std::endl; exit(EXIT_FAILURE); }
    clk.mark("lime_init (HIP runtime)");
    if (lime_build_index(ctx, all.data(), doc_off.data(), n_docs, 0, trlcp, ebwt.data(), lcp.data(), da.data()) != LIME_OK) {
        std::cerr << "Error: " << lime_last_error() << std::endl; exit(1);
    }
    clk.mark("index");
    lime_shutdown(ctx);
    if (!write_file(base + ".ebwt", ebwt.data(), n) || !write_file(base + ".lcp", lcp.data(), n * 4) || !write_file(base + ".da", da.data(), n * 4)) {
        std::cerr << "Error writing " << base << ".ebwt / .lcp / .da." << std::endl;
        return -LIME_ERR_IO;
    }
    clk.mark("output files");
    std::cout << "numReads: " << nd[0] << "\nnumGenomes: " << nd[1] << "\nsymbols: " << n << std::endl;
    return 0;
}
