// lime_classify.h -- what the read-assignment step's host code (lime_classify.cpp, HIP-free: bin/Classify is built from it
// with g++ alone) shares with the device path (lime_choose.cpp, lime_classify_kernel.hip): the lineage parser, the value
// tables, decide() and the classification file's line writer.  Not part of the public ABI (include/lime_hip.h is).
#pragma once
#include <stdint.h>

#include <ostream>
#include <string>
#include <vector>

#include "lime_hip.h"

namespace lime_cls {

const float TOL = static_cast<float>(0.02);      // ERROR, src/Tools.h:37
const int N_RANKS = 6;                           // species .. phylum (RANK, Classify.cpp:24)

struct Cell { float sim; uint32_t ref; };
struct ReadLists {                               // one read in one .res file
    float top = 0.0f;                            // the file's maximum for the read (0: no record)
    std::vector<Cell> cells;
    void clear() { top = 0.0f; cells.clear(); }
};

struct Taxonomy {
    std::vector<uint32_t> at_rank;               // genome -> taxon at the chosen rank (rank 0: genome index)
    std::vector<std::vector<uint32_t>> higher;   // [rank-1 .. 5][genome], 0 = unknown (HIGHER)
    std::string rank_name;
};

bool read_taxonomy(const std::string &path, int rank, bool higher, uint32_t n_targ, Taxonomy &tx, std::string &err);
// the value a .res reader sees for a count k of a row normalised by norm: binary != 0 the float the writer stores
// (float(k) / norm), else that float printed with %.5f and read back with `>> float` (.res.txt); tops as the cells,
// 0 where the writer's test `float(k) / norm > beta` writes no record
void value_tables(uint32_t norm, float beta, int binary, float vals[256], float tops[256]);
// the decision of one read over its n_files lists (rules U, 1, 2, 3 / H / A; Classify.cpp:503-690); all[] is scratch
lime_verdict_t decide(const ReadLists *L, uint32_t n_files, uint32_t n_targ, const Taxonomy &tx, int rank, bool higher,
                      std::vector<float> (&all)[2]);
// one line of the classification file, and the counts {C, U, A, H}
void write_verdict(std::ostream &out, uint64_t r, const lime_verdict_t &v, uint64_t counts[4]);

} // namespace lime_cls

// the opaque lime_taxonomy of the ABI: the parsed lineage file and, once a device classification has used it, its device
// copy (at_rank[n_targ] then, with HIGHER, higher[6][n_targ]) -- owned by the device side, which sets `release`
struct lime_taxonomy {
    lime_cls::Taxonomy host;
    int rank = 0, higher = 0;
    uint32_t n_targ = 0;
    int dev = -1;
    void *d_tab = nullptr;
    void (*release)(lime_taxonomy *) = nullptr;
};
